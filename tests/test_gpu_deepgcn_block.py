"""GPU suite: DeepGCN's fused blocks -- `deepgcn.ResDynBlock` (ReLU and the residual in the EdgeConv output kernel,
apn_ec_out_res / apn_ec_bwd_prep_act) and the head `deepgcn.GraphConv` (ReLU, no residual) -- against the float64
restatement (tests/deepgcn_reference.py), the composed fp32 block measured beside them on the same idx.

The bar (the project's own, tests/test_gpu_edge_conv.py): per tensor, the fused block's relative L2 distance to float64
may be at most 4 x the composed fp32 block's on the same input, with a floor of 2e-6.  Inputs: of 8 seeded inputs per
shape the one whose float64 evaluation keeps its pool winners and activation gates farthest from switching -- a
criterion of the reference alone.  idx = the dilated kNN graph of the input (csrc/knn.hip), computed once."""
import gc

import pytest
import torch

import deepgcn_reference as R

pytestmark = pytest.mark.gpu
RELU = {'act': 'relu'}
LEAKY = {'act': 'leakyrelu', 'negative_slope': 0.2}
#         B, N,   C,  H,  K,  dilation of the graph
SHAPES = [(2, 100, 4, 64, 16, 2),          # the head: ReLU, no residual
          (3, 77, 64, 64, 1, 1),
          (4, 256, 64, 64, 16, 4),         # residual
          (2, 128, 128, 128, 9, 3)]        # residual


def _block(dev, C, H, K, d, fused, flip=False, act=RELU):
    """C == H: a ResDynBlock; else the head's GraphConv."""
    from adaptpoint_amd.deepgcn import GraphConv, ResDynBlock
    from adaptpoint_amd.pointnext import fill_parameters_by_name
    kw = dict(norm_args={'norm': 'bn'}, act_args=dict(act), fused=fused)
    blk = fill_parameters_by_name(ResDynBlock(C, 'edge', K, d, **kw) if C == H else GraphConv(C, H, 'edge', bias=False, **kw))
    if flip:
        R.flip_every_third_gamma(blk.body.gconv if C == H else blk.gconv)
    return blk.to(dev)


def _graph(x, K, d):
    from adaptpoint_amd.layers import knn_dilated
    rows = x.detach().transpose(1, 2).contiguous()
    return knn_dilated(rows, rows, K, d)


def _step(blk, x, w, idx, need_x=True):
    """forward + backward of (out * w).sum(): {out, dx, grads, buffers}; the block's gradients are cleared first."""
    blk.zero_grad(set_to_none=True)
    x = x.detach().clone().requires_grad_(need_x)
    out = blk(x.unsqueeze(-1), idx).squeeze(-1)
    if out.requires_grad:
        (out * w).sum().backward()
    return {'out': out.detach(), 'dx': x.grad,
            'grads': {n: q.grad for n, q in blk.named_parameters() if q.grad is not None},
            'buffers': {n: b.detach().clone() for n, b in blk.named_buffers()}}


def _errors(res, ref):
    errs = {'out': R.rel(res['out'], ref['out'])}
    if ref.get('dx') is not None:
        errs['dx'] = R.rel(res['dx'], ref['dx'])
    for n, g in ref.get('grads', {}).items():
        errs['grad/' + n] = R.rel(res['grads'][n], g)
    for n, b in ref['buffers'].items():
        if not n.endswith('num_batches_tracked'):
            errs['buf/' + n] = R.rel(res['buffers'][n], b)
    return errs


def _within(fused, composed, what):
    rows = {k: (fused[k], composed[k]) for k in composed}
    print(what, "(fused, composed) distance to float64:", {k: "%.1e / %.1e" % v for k, v in rows.items()})
    bad = {k: v for k, v in rows.items() if not v[0] <= max(4.0 * v[1], 2e-6)}
    assert not bad, (what, bad)


_PICKED = {}


def _pick_inputs(dev, B, N, C, H, K, d, flip=False, act=RELU, seeds=8):
    """The seeded input, of `seeds`, whose float64 evaluation has the largest decision margin: (x, w, idx) -- picked
    once per case and shared, unchanged, by the tests that use it."""
    key = (B, N, C, H, K, d, flip, act['act'])
    if key not in _PICKED:
        best = None
        ref = _block(dev, C, H, K, d, False, flip, act).train()
        for seed in range(seeds):
            x, w = R.block_inputs(B, N, C, H, 10 * N + seed)
            x = x.to(dev)
            idx = _graph(x, K, d)
            m = R.run_res64(ref, x, idx)['margin']
            if best is None or m > best[0]:
                best = (m, seed, x, w.to(dev), idx)
        print(f"B={B} N={N} C={C} H={H} K={K} d={d}: input seed {best[1]} of {seeds}, decision margin {best[0]:.1e}")
        _PICKED[key] = best[2:]
    return _PICKED[key]


def _compare(dev, B, N, C, H, K, d, flip=False, what=None, eval_mode=False, need_x=True, frozen=False, act=RELU):
    from adaptpoint_amd import set_abstraction as SA
    before = dict(SA.FUSED_FALLBACKS)
    x, w, idx = _pick_inputs(dev, B, N, C, H, K, d, flip, act)
    res = {}
    for fused in (False, True):
        blk = _block(dev, C, H, K, d, fused, flip, act).train(not eval_mode)
        if frozen:
            for q in blk.parameters():
                q.requires_grad_(False)
        res[fused] = _step(blk, x, w, idx, need_x=need_x)
    ref = R.run_res64(_block(dev, C, H, K, d, False, flip, act).train(not eval_mode), x, idx, w, training=not eval_mode)
    if frozen:
        ref['grads'] = {}
        assert not res[True]['grads']
    if not need_x:
        ref.pop('dx')
        assert res[True]['dx'] is None
    _within(_errors(res[True], ref), _errors(res[False], ref), what or f"B={B} N={N} C={C} H={H} K={K} d={d}")
    if not eval_mode:
        counters = [int(b) for n, b in res[True]['buffers'].items() if n.endswith('num_batches_tracked')]
        assert counters == [1]
    assert SA.FUSED_FALLBACKS == before, "the fused block fell back"
    return res


RES = (4, 256, 64, 64, 16, 4)


@pytest.mark.parametrize("B,N,C,H,K,d", SHAPES)
def test_fused_block_against_float64(dev, B, N, C, H, K, d):
    """Output, dL/dx, every parameter gradient and the BatchNorm buffers, training mode."""
    _compare(dev, B, N, C, H, K, d)


def test_relu_really_gates_and_the_residual_is_added(dev):
    """The fused output is not the block without its residual, and ReLU's zeros are there: out - x >= 0 with zeros."""
    x, w, idx = _pick_inputs(dev, *RES)
    with torch.no_grad():
        out = _block(dev, 64, 64, 16, 4, True).train()(x.unsqueeze(-1), idx).squeeze(-1)
    body = out - x
    assert (body >= -1e-6 * x.abs().max()).all() and (body == 0).any() and (body > 0.1).any()


def test_negative_gamma_selects_the_minimum(dev):
    _compare(dev, *RES, flip=True, what="every third gamma negative")


def test_eval_mode(dev):
    res = _compare(dev, *RES, eval_mode=True, what="eval mode")
    ref = dict(_block(dev, 64, 64, 16, 4, True).named_buffers())
    for n, b in res[True]['buffers'].items():
        assert torch.equal(b, ref[n]), n                          # running statistics untouched


def test_input_without_gradient_and_frozen_weights(dev):
    _compare(dev, *RES, need_x=False, what="x without gradient")
    _compare(dev, *RES, frozen=True, what="all weights frozen")


def test_leaky_relu_with_a_residual(dev):
    """The new entries at a positive slope."""
    _compare(dev, *RES, act=LEAKY, what="LeakyReLU(0.2) with a residual")


def test_residual_that_is_not_the_input(dev):
    """`edge_conv(..., residual=r)` for a tensor of its own, here a copy of x with other strides: the output is the
    ResDynBlock's bit for bit, the residual's gradient is g, and dL/dx + g is the ResDynBlock's dL/dx."""
    from adaptpoint_amd import edge_conv as EC
    x, w, idx = _pick_inputs(dev, *RES)
    e = _block(dev, 64, 64, 16, 4, True).train().body.gconv
    r = x.transpose(1, 2).contiguous().transpose(1, 2).requires_grad_(True)
    assert not r.is_contiguous()
    xin = x.clone().requires_grad_(True)
    out = EC.edge_conv(xin, EC.edge_index(idx), e.nn[0], e.nn[1], 0.0, residual=r)
    (out * w).sum().backward()
    plain = _step(_block(dev, 64, 64, 16, 4, True).train(), x, w, idx)
    assert torch.equal(out.detach(), plain['out'])
    assert torch.equal(r.grad, w)
    assert torch.equal(xin.grad + w, plain['dx'])


def test_backward_is_bit_identical_from_run_to_run(dev):
    x, w, idx = _pick_inputs(dev, *RES)
    blk = _block(dev, 64, 64, 16, 4, True).train()
    state = {n: b.clone() for n, b in blk.named_buffers()}
    runs = []
    for _ in range(2):
        with torch.no_grad():
            for n, b in blk.named_buffers():
                b.copy_(state[n])
        r = _step(blk, x, w, idx)
        runs.append([r['out'], r['dx']] + [r['grads'][n].clone() for n in sorted(r['grads'])])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_block_replayed_from_a_hipgraph_equals_eager(dev):
    """Forward + backward captured over an `EdgeIndex` built ahead: no memset node; three replays bit-identical to the
    eager run; the BatchNorm buffers advance once per replay."""
    from adaptpoint_amd import graphs
    from adaptpoint_amd.edge_conv import edge_index
    x, w, idx = _pick_inputs(dev, *RES)
    blk = _block(dev, 64, 64, 16, 4, True).train()
    xin = x.clone().requires_grad_(True)
    params = list(blk.parameters())
    index = edge_index(idx)

    def step():
        # (the loss (out * w).sum() as its gradient w handed to autograd: torch's sum would put a memset in the graph)
        out = blk(xin.unsqueeze(-1), index).squeeze(-1)
        return [out.detach()] + list(torch.autograd.grad(out, [xin] + params, w))
    state = {n: b.clone() for n, b in blk.named_buffers()}

    def restore():
        with torch.no_grad():
            for n, b in blk.named_buffers():
                b.copy_(state[n])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                       # warm-up: allocator pools, lazy initialisation
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    restore()
    eager = [t.clone() for t in step()]
    after_one = {n: b.clone() for n, b in blk.named_buffers()}
    torch.cuda.synchronize()
    gc.collect()
    graph, captured, census = graphs.capture(step, leaves=params + [xin], what="the ResDynBlock's graph")
    print("ResDynBlock graph:", census)
    assert not census.get("memset", 0)
    restore()
    for i in range(3):
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(eager, captured):
            assert torch.equal(a, b), i
        if i == 0:
            for n, b in blk.named_buffers():
                assert torch.equal(b, after_one[n]), n
    assert int(blk.body.gconv.nn[1].num_batches_tracked) == int(state['body.gconv.nn.1.num_batches_tracked']) + 3
