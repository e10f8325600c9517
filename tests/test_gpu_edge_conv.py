"""GPU suite: the fused EdgeConv block (csrc/edge_conv.hip through adaptpoint_amd.edge_conv / dgcnn.EdgeConv) against
the float64 restatement (tests/dgcnn_reference.py), the composed fp32 path measured beside it.

The bar (the project's own, tests/test_gpu_invres.py): per tensor, the fused path's relative L2 distance to float64 may
be at most 4 x the composed fp32 block's (existing operators + PyTorch, fused=False) on the same input, with a floor of
2e-6.  Inputs: of 8 seeded inputs per shape the one whose float64 evaluation keeps its pool winners and LeakyReLU gates
farthest from switching (`run_edge64`'s margin) -- a criterion of the reference alone.  All three evaluations use the
same idx, computed once.  Every step runs once."""
import gc

import numpy as np
import pytest
import torch

import dgcnn_reference as R
import golden_inputs as GI

pytestmark = pytest.mark.gpu
SHAPES = [(2, 100, 3, 64, 20), (3, 77, 4, 64, 1), (4, 256, 64, 64, 20), (2, 256, 64, 128, 20), (2, 128, 128, 256, 40),
          (2, 96, 64, 512, 20)]


def _edge(dev, C, H, fused, flip=False):
    from adaptpoint_amd.dgcnn import LEAKY, EdgeConv
    from adaptpoint_amd.pointnext import fill_parameters_by_name
    e = fill_parameters_by_name(EdgeConv(C, H, norm_args={'norm': 'bn'}, act_args=dict(LEAKY), fused=fused))
    return (R.flip_every_third_gamma(e) if flip else e).to(dev)


def _knn(x, K):
    from adaptpoint_amd.layers import knn_query
    rows = x.detach().transpose(1, 2).contiguous()
    return knn_query(rows, rows, K)


def _step(edge, x, w, idx, need_x=True):
    """forward + backward of (out * w).sum(): {out, dx, grads, buffers}; the block's gradients are cleared first."""
    edge.zero_grad(set_to_none=True)
    x = x.detach().clone().requires_grad_(need_x)
    out = edge(x.unsqueeze(-1), idx).squeeze(-1)
    if out.requires_grad:
        (out * w).sum().backward()
    return {'out': out.detach(), 'dx': x.grad,
            'grads': {n: q.grad for n, q in edge.named_parameters() if q.grad is not None},
            'buffers': {n: b.detach().clone() for n, b in edge.named_buffers()}}


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


def _pick_inputs(dev, B, N, C, H, K, flip=False, make_idx=None, seeds=8):
    """The seeded input, of `seeds`, whose float64 evaluation has the largest decision margin: (x, w, idx)."""
    best = None
    ref = _edge(dev, C, H, False, flip).train()
    for seed in range(seeds):
        x = R.edge_inputs(B, N, C, 10 * N + seed).to(dev)
        idx = _knn(x, K) if make_idx is None else make_idx(x)
        m = R.run_edge64(ref, x, idx)['margin']
        if best is None or m > best[0]:
            best = (m, seed, x, idx)
    print(f"B={B} N={N} C={C} H={H} K={K}: input seed {best[1]} of {seeds}, decision margin {best[0]:.1e}")
    w = torch.from_numpy(GI.seeded_normal((B, H, N), 1350 + best[1]).astype(np.float32)).to(dev)
    return best[2], w, best[3]


def _compare(dev, B, N, C, H, K, flip=False, what=None, eval_mode=False, need_x=True, frozen=False, make_idx=None):
    from adaptpoint_amd import set_abstraction as SA
    before = dict(SA.FUSED_FALLBACKS)
    x, w, idx = _pick_inputs(dev, B, N, C, H, K, flip, make_idx)
    res = {}
    for fused in (False, True):
        blk = _edge(dev, C, H, fused, flip).train(not eval_mode)
        if frozen:
            for q in blk.parameters():
                q.requires_grad_(False)
        res[fused] = _step(blk, x, w, idx, need_x=need_x)
    ref = R.run_edge64(_edge(dev, C, H, False, flip).train(not eval_mode), x, idx, w, training=not eval_mode)
    if frozen:
        ref['grads'] = {}
        assert not res[True]['grads']
    if not need_x:
        ref.pop('dx')
        assert res[True]['dx'] is None
    _within(_errors(res[True], ref), _errors(res[False], ref), what or f"B={B} N={N} C={C} H={H} K={K}")
    if not eval_mode:
        assert int(res[True]['buffers']['nn.1.num_batches_tracked']) == 1
    assert SA.FUSED_FALLBACKS == before, "the fused block fell back"
    return res


@pytest.mark.parametrize("B,N,C,H,K", SHAPES)
def test_fused_block_against_float64(dev, B, N, C, H, K):
    """Output, dL/dx, every parameter gradient and the BatchNorm buffers, training mode; idx = the kNN of the input."""
    _compare(dev, B, N, C, H, K)


def test_negative_gamma_selects_the_minimum(dev):
    _compare(dev, 4, 256, 64, 64, 20, flip=True, what="every third gamma negative")


def test_eval_mode(dev):
    res = _compare(dev, 4, 256, 64, 64, 20, eval_mode=True, what="eval mode")
    ref = dict(_edge(dev, 64, 64, True).named_buffers())
    for n, b in res[True]['buffers'].items():
        assert torch.equal(b, ref[n]), n                          # running statistics untouched


def test_input_without_gradient_and_frozen_weights(dev):
    _compare(dev, 4, 256, 64, 64, 20, need_x=False, what="x without gradient")
    _compare(dev, 4, 256, 64, 64, 20, frozen=True, what="all weights frozen")


def _random_half(x, K=20):
    """Rows with repeated neighbours, drawn from the first half of the cloud: the second half is gathered by nobody."""
    B, _, N = x.shape
    g = torch.Generator().manual_seed(N)
    return torch.randint(0, N // 2, (B, N, K), generator=g, dtype=torch.int32).to(x.device)


def test_arbitrary_indices(dev):
    _compare(dev, 2, 100, 64, 64, 20, make_idx=_random_half, what="repeated neighbours, points nobody gathers")
    _compare(dev, 2, 100, 64, 64, 20, what="idx = 0: one reverse list of length N K",
             make_idx=lambda x: torch.zeros(x.shape[0], x.shape[2], 20, dtype=torch.int32, device=x.device))


def _assert_lists_of(tgt, rows, pcnt_poff, plist):
    """pcnt / poff / plist are the reverse lists of the positions whose targets (flat rows) are tgt: a stable argsort."""
    pcnt, poff = pcnt_poff.cpu().numpy()
    order = np.argsort(tgt, kind="stable")                           # positions by the point they gather, ascending
    assert np.array_equal(pcnt, np.bincount(tgt, minlength=rows))
    assert np.array_equal(poff, np.cumsum(pcnt) - pcnt)
    assert np.array_equal(plist.cpu().numpy(), order.astype(np.int32))


def test_reverse_lists_are_the_positions_in_ascending_order(dev):
    """apn_ec_csr against numpy, for a kNN graph, for repeated / missing neighbours and for idx = 0."""
    from adaptpoint_amd.edge_conv import edge_index
    x = R.edge_inputs(3, 150, 64, 7).to(dev)
    for idx in (_knn(x, 20), _random_half(x), torch.zeros(3, 150, 33, dtype=torch.int32, device=dev)):
        B, N, K = idx.shape
        g = edge_index(idx)
        tgt = (idx.cpu().numpy().astype(np.int64) + (np.arange(B) * N)[:, None, None]).reshape(-1)
        _assert_lists_of(tgt, B * N, g.pcnt_poff, g.plist)
        again = edge_index(idx)
        assert torch.equal(again.plist, g.plist) and torch.equal(again.pcnt_poff, g.pcnt_poff)


def test_reverse_lists_where_the_scan_takes_several_points_per_thread(dev):
    """The scan kernel shared by apn_ec_csr and apn_po_csr (csrc/reverse_lists.h) is one workgroup of 1024 threads per
    cloud: clouds of 1025 points (two per thread, two clouds: the second one's base) and one set of 2049 rows (three per
    thread) gathered by 700 x 3 positions, against the same numpy statement."""
    from adaptpoint_amd.edge_conv import edge_index
    from adaptpoint_amd.pointops import build_csr
    B, N, K = 2, 1025, 3
    idx = torch.randint(0, N, (B, N, K), generator=torch.Generator().manual_seed(N), dtype=torch.int32)
    g = edge_index(idx.to(dev))
    tgt = (idx.numpy().astype(np.int64) + (np.arange(B) * N)[:, None, None]).reshape(-1)
    _assert_lists_of(tgt, B * N, g.pcnt_poff, g.plist)
    n, m, k = 2049, 700, 3
    idx = torch.randint(0, n, (m, k), generator=torch.Generator().manual_seed(n), dtype=torch.int32)
    c = build_csr(idx.to(dev), n)
    _assert_lists_of(idx.numpy().astype(np.int64).reshape(-1), n, c.pcnt_poff, c.plist)


def test_backward_is_bit_identical_from_run_to_run(dev):
    blk = _edge(dev, 64, 128, True).train()
    x = R.edge_inputs(4, 256, 64, 5).to(dev)
    w = torch.from_numpy(GI.seeded_normal((4, 128, 256), 1355).astype(np.float32)).to(dev)
    state = {n: b.clone() for n, b in blk.named_buffers()}
    runs = []
    for _ in range(2):
        with torch.no_grad():
            for n, b in blk.named_buffers():
                b.copy_(state[n])
        r = _step(blk, x, w, _knn(x, 20))
        runs.append([r['out'], r['dx']] + [r['grads'][n].clone() for n in sorted(r['grads'])])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_block_replayed_from_a_hipgraph_equals_eager(dev):
    """Forward + backward captured over a graph index built ahead: no memset node; three replays bit-identical to the
    eager run; the BatchNorm buffers advance once per replay."""
    from adaptpoint_amd import graphs
    from adaptpoint_amd.edge_conv import edge_index
    blk = _edge(dev, 64, 64, True).train()
    x = R.edge_inputs(4, 256, 64, 6).to(dev)
    w = torch.from_numpy(GI.seeded_normal((4, 64, 256), 1356).astype(np.float32)).to(dev)
    xin = x.clone().requires_grad_(True)
    params = list(blk.parameters())
    index = edge_index(_knn(x, 20))

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
    graph, captured, census = graphs.capture(step, leaves=params + [xin], what="the EdgeConv block's graph")
    print("EdgeConv block graph:", census)
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
    assert int(blk.nn[1].num_batches_tracked) == int(state['nn.1.num_batches_tracked']) + 3


def test_index_step_replays_from_a_hipgraph_without_a_memset_node(dev):
    """kNN + reverse lists captured (the index step of a block): kernels only."""
    from adaptpoint_amd import graphs
    from adaptpoint_amd.edge_conv import edge_index
    x = R.edge_inputs(2, 200, 64, 8).to(dev)

    def step():
        g = edge_index(_knn(x, 20))
        return [g.idx, g.pcnt_poff, g.plist]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    eager = [t.clone() for t in step()]
    torch.cuda.synchronize()
    gc.collect()
    graph, captured, census = graphs.capture(step, what="the EdgeConv index step's graph")
    assert not census.get("memset", 0)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, captured):
        assert torch.equal(a, b)


def test_uncovered_shape_takes_the_composed_path_with_a_recorded_fallback(dev):
    from adaptpoint_amd import set_abstraction as SA
    x = R.edge_inputs(2, 100, 64, 9).to(dev)
    w = torch.from_numpy(GI.seeded_normal((2, 96, 100), 1359).astype(np.float32)).to(dev)
    idx = _knn(x, 20)
    before = sum(SA.FUSED_FALLBACKS.values())
    res = {fused: _step(_edge(dev, 64, 96, fused).train(), x, w, idx) for fused in (False, True)}
    assert sum(SA.FUSED_FALLBACKS.values()) == before + 1
    assert any("EdgeConv" in k and "96" in k for k in SA.FUSED_FALLBACKS)
    assert R.rel(res[True]['out'], res[False]['out']) < 1e-6 and R.rel(res[True]['dx'], res[False]['dx']) < 1e-6


def test_the_slope_guarded_c_entries_equal_the_general_ones_bit_for_bit(dev):
    """`adaptpoint_amd.edge_conv` launches through apn_ec_out_res / apn_ec_bwd_prep_act only; apn_ec_out and
    apn_ec_bwd_prep stay in the C interface over the same launchers, so each pair called raw on the same operands writes
    the same bits.  N = 65: one point past the 64-point tile; H = 128: two channel tiles; g (B,H,N) is a permuted view
    of a (B,N,H) buffer, passed by its strides."""
    from adaptpoint_amd import _lib
    from adaptpoint_amd.fused import _call
    B, N, H, slope = 2, 65, 128, 0.2
    ext = torch.from_numpy(GI.seeded_normal((B, N, H), 1360).astype(np.float32)).to(dev)
    pack = torch.from_numpy(GI.seeded_normal((4 * H,), 1361).astype(np.float32)).to(dev)
    g = torch.from_numpy(GI.seeded_normal((B, N, H), 1362).astype(np.float32)).to(dev).permute(0, 2, 1)
    assert g.shape == (B, H, N) and not g.is_contiguous()
    gs = g.stride()
    outs = [torch.full((B, H, N), float('nan'), device=dev) for _ in range(2)]
    _call("apn_ec_out", dev, B, N, H, ext.data_ptr(), pack.data_ptr(), slope, outs[0].data_ptr())
    _call("apn_ec_out_res", dev, B, N, H, ext.data_ptr(), pack.data_ptr(), slope, None, 0, 0, 0, outs[1].data_ptr())
    assert not torch.isnan(outs[0]).any() and torch.equal(outs[0], outs[1])
    rows = _lib.load().apn_ec_bwd_prep_rows(B, N)
    assert rows == B * 2
    res = []
    for name in ("apn_ec_bwd_prep", "apn_ec_bwd_prep_act"):
        gsel = torch.full((B, N, H), float('nan'), device=dev)
        partS = torch.full((rows, 2 * H), float('nan'), device=dev)
        _call(name, dev, B, N, H, g.data_ptr(), gs[0], gs[1], gs[2], ext.data_ptr(), pack.data_ptr(), slope,
              gsel.data_ptr(), partS.data_ptr())
        res.append((gsel, partS))
    for a, b in zip(*res):
        assert not torch.isnan(a).any() and torch.equal(a, b)
