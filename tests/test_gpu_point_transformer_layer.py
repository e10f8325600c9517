"""GPU suite of the fused Point Transformer layer (csrc/point_transformer.hip, adaptpoint_amd/pt_layer.py).

Exact cases on the raw apn_pt_* entries: small-integer q, k, v, h and weights with the BatchNorms folded to scale 1 /
shift 0, so that every intermediate is an integer far below 2^24 and the kernels must reproduce the float64 statement
bit for bit whatever their summation order.  Then the layer: fused against composed against float64
(tests/point_transformer_reference.py) on one shared graph -- per tensor the fused path's relative L2 distance to float64
is at most max(4 x the composed path's, 2e-6), the bar of tests/test_gpu_edge_conv.py -- reproducibility, graph capture
and the fallback bookkeeping.  All on the ragged set pointops_reference.SIZES (705 rows; clouds of 5 and 1 below k)."""
import functools
import gc

import numpy as np
import pytest
import torch

import pointops_reference as PR
import point_transformer_reference as R

pytestmark = pytest.mark.gpu

SIZES = PR.SIZES
N = int(sum(SIZES))
LAYER_CASES = [(32, 8), (64, 16), (512, 16)]
FLOOR = 2e-6


def T(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@functools.lru_cache(maxsize=None)
def _graph(k):
    """The kNN graph of the seeded ragged clouds: p, o, idx (705,k) on the GPU."""
    from adaptpoint_amd import pointops as PO
    dev = torch.device("cuda")
    p, o = T(dev, PR.seeded_clouds(SIZES, 31)), T(dev, PR.offsets(SIZES))
    idx, _ = PO.knnquery(k, p, p, o, o)
    return p, o, idx


def _call(name, *args):
    from adaptpoint_amd.fused import _call as call
    call(name, torch.device("cuda", torch.cuda.current_device()), *args)


def _fold(part, width):
    sums = torch.empty(width, dtype=torch.float64, device=part.device)
    _call("apn_pt_fold", part.data_ptr(), part.shape[0], width, sums.data_ptr())
    return sums


class _Raw:
    """Small-integer inputs of the raw entries at (C, k), and the float64 statement of every intermediate."""

    def __init__(self, dev, C, k, w4_scale=0.0, sc2=1.0):
        from adaptpoint_amd import _lib
        self.C, self.k, self.Cp = C, k, C // 8
        Cp = self.Cp
        _, _, self.idx = _graph(k)
        ints = lambda shape, salt, hi: T(dev, PR.small_ints(shape, 100 * C + k + salt, hi))
        self.qkv, self.h = ints((N, 3 * C), 1, 2), ints((N, k, 3), 2, 2)
        self.W2, self.b2 = ints((C, 3), 3, 2), ints((C,), 4, 2)
        self.W3, self.b3 = ints((Cp, C), 5, 1), ints((Cp,), 6, 2)
        self.W4, self.b4 = ints((Cp, Cp), 7, 1) * w4_scale, ints((Cp,), 8, 1) * w4_scale
        self.wts = torch.cat([self.W2.reshape(-1), self.b2, self.W3.t().reshape(-1), self.b3, self.W4.reshape(-1),
                              self.b4]).contiguous()
        self.bn = torch.cat([torch.ones(C), torch.zeros(C), torch.full((Cp,), sc2), torch.zeros(Cp)]).to(dev)
        self.rows = _lib.load().apn_pt_rows(N, k, C)
        self.mid_rows = _lib.load().apn_pt_mid_rows(N, k, C)
        d = lambda t: t.double()
        j = self.idx.long()
        q, kk, v = d(self.qkv[:, :C]), d(self.qkv[:, C:2 * C]), d(self.qkv[:, 2 * C:])
        self.pr = d(self.h) @ d(self.W2).t() + d(self.b2)                           # (n,k,C)
        self.r = kk[j] - q[:, None, :] + self.pr
        self.t64 = torch.relu(self.r) @ d(self.W3).t() + d(self.b3)                  # (n,k,C')
        self.vpr = v[j] + self.pr

    def common(self):
        return (N, self.k, self.C, self.qkv.data_ptr(), 3 * self.C, self.h.data_ptr(), self.idx.data_ptr(),
                self.wts.data_ptr())

    def forward(self, dev):
        C, Cp, k = self.C, self.Cp, self.k
        part = torch.empty(self.mid_rows, 2 * Cp, dtype=torch.float64, device=dev)
        t = torch.empty(N, k, Cp, device=dev)
        _call("apn_pt_mid", *self.common(), self.bn.data_ptr(), t.data_ptr(), part.data_ptr())
        a, out = torch.empty(N, k, Cp, device=dev), torch.empty(N, C, device=dev)
        _call("apn_pt_attend", *self.common(), self.bn.data_ptr(), t.data_ptr(), a.data_ptr(), out.data_ptr())
        return t, part, a, out


@pytest.mark.parametrize("C", [32, 64, 512])
@pytest.mark.parametrize("k", [8, 16])
def test_raw_forward_entries_on_exact_cases(dev, C, k):
    raw = _Raw(dev, C, k)
    Cp = raw.Cp
    assert (raw.idx[70:75, 5:] == 70).all()                      # the cloud of 5 pads its neighbourhoods with its start
    part = torch.empty(raw.rows, 2 * C, dtype=torch.float64, device=dev)
    _call("apn_pt_rel_stats", *raw.common(), part.data_ptr())
    sums = _fold(part, 2 * C)
    assert torch.equal(sums[:C], raw.r.sum((0, 1))) and torch.equal(sums[C:], (raw.r * raw.r).sum((0, 1)))
    t, part, a, out = raw.forward(dev)
    assert torch.equal(t.double(), raw.t64)
    sums = _fold(part, 2 * Cp)
    assert torch.equal(sums[:Cp], raw.t64.sum((0, 1))) and torch.equal(sums[Cp:], (raw.t64 * raw.t64).sum((0, 1)))
    assert torch.equal(a, torch.full_like(a, 1.0 / k))           # W4 = 0: the softmax is exactly 1 / k
    assert torch.equal(out.double(), raw.vpr.sum(1) / k)
    # eval mode's call (no statistics wanted) writes the same t
    t2 = torch.empty_like(t)
    _call("apn_pt_mid", *raw.common(), raw.bn.data_ptr(), t2.data_ptr(), None)
    assert torch.equal(t2, t)


@pytest.mark.parametrize("C", [32, 64, 512])
def test_raw_scatter_on_exact_cases_catches_a_wrong_weight_channel(dev, C):
    """One-hot go (channel c lives on row c mod 70, a row whose k neighbours are distinct) and an attention weight read
    back from the forward entries that differs from c' to c': dv_j[c] is then a single a[i,s,c mod C'] and dk a sum of
    small integers -- both equal the float64 list sums exactly."""
    from adaptpoint_amd import pointops as PO
    k = 16
    raw = _Raw(dev, C, k, w4_scale=0.25, sc2=2.0 ** -10)
    Cp = raw.Cp
    _, _, a, _ = raw.forward(dev)
    assert torch.allclose(a.sum(1), torch.ones(N, Cp, device=dev), atol=1e-5)
    assert (a[:70, :, 0] != a[:70, :, 1]).any()                  # the weight differs from c' to c'
    go = torch.zeros(N, C, device=dev)
    go[torch.arange(C, device=dev) % 70, torch.arange(C, device=dev)] = 1.0
    dr = T(dev, PR.small_ints((N, k, C), 9, 3))
    csr = PO.csr_of(raw.idx, N)
    dqkv = torch.full((N, 3 * C), float("nan"), device=dev)
    _call("apn_pt_scatter_bwd", N, k, C, dr.data_ptr(), go.data_ptr(), a.data_ptr(), csr.pcnt_poff.data_ptr(),
          csr.plist.data_ptr(), dqkv.data_ptr(), 3 * C)
    j = raw.idx.long().reshape(-1)
    dk64 = torch.zeros(N, C, dtype=torch.float64, device=dev).index_add_(0, j, dr.double().reshape(-1, C))
    terms = go.double()[:, None, :] * a.double().repeat(1, 1, 8)                     # channel c reads weight c mod C'
    dv64 = torch.zeros(N, C, dtype=torch.float64, device=dev).index_add_(0, j, terms.reshape(-1, C))
    wrong = go.double()[:, None, :] * a.double().repeat_interleave(8, dim=2)         # ... not c div 8
    assert not torch.equal(terms, wrong)
    assert torch.isnan(dqkv[:, :C]).all()                        # dq is rel_bwd's
    assert torch.equal(dqkv[:, C:2 * C].double(), dk64)
    assert torch.equal(dqkv[:, 2 * C:].double(), dv64)


@pytest.mark.parametrize("n,width", [(1, 96), (705, 96), (3100, 1536)])
def test_raw_column_sums_on_exact_cases(dev, n, width):
    """apn_pt_colsum + apn_pt_fold (the projection's bias gradient) on small integers in rows of a wider pitch."""
    from adaptpoint_amd import _lib
    ld = width + 5
    src = T(dev, PR.small_ints((n, ld), 77, 4))
    rows = _lib.load().apn_pt_colsum_rows(n)
    part = torch.empty(rows, width, dtype=torch.float64, device=dev)
    _call("apn_pt_colsum", n, width, src.data_ptr(), ld, part.data_ptr())
    assert torch.equal(_fold(part, width), src[:, :width].double().sum(0))


# ------------------------------------------------------------------------------------------------- the layer
def _layer(C, k, fused):
    from adaptpoint_amd.point_transformer import PointTransformerLayer
    return R.seed_module(PointTransformerLayer(C, C, 8, k, fused=fused), 7).cuda()


def _run(layer, p, x, o, graph, w, training):
    layer.train(training)
    x = x.clone().requires_grad_(True)
    out = layer([p, x, o, graph])
    (out * w).sum().backward()
    res = {"out": out.detach(), "dx": x.grad}
    res.update({"grad/" + n: q.grad for n, q in layer.named_parameters()})
    res.update({"buf/" + n: b.detach().clone() for n, b in layer.named_buffers() if not n.endswith("num_batches_tracked")})
    res["nbt"] = [int(b) for n, b in layer.named_buffers() if n.endswith("num_batches_tracked")]
    return res


@functools.lru_cache(maxsize=None)
def _case(C, k, training):
    """Fused, composed and float64 on one shared graph; computed once per case."""
    from adaptpoint_amd import set_abstraction as SA
    from adaptpoint_amd.point_transformer import StageGraph
    dev = torch.device("cuda")
    p, o, idx = _graph(k)
    _, x, _, w = (t.to(dev) for t in R.layer_inputs(SIZES, C, 3))
    graph = StageGraph(p, o, k, idx)
    before = dict(SA.FUSED_FALLBACKS)
    fused = _run(_layer(C, k, True), p, x, o, graph, w, training)
    assert SA.FUSED_FALLBACKS == before                          # the covered shapes add no entry
    comp = _run(_layer(C, k, False), p, x, o, graph, w, training)
    r64 = R.run_layer64(_layer(C, k, False), p, x, o, idx, w, training)
    ref = {"out": r64["out"], "dx": r64["dx"]}
    ref.update({"grad/" + n: g for n, g in r64["grads"].items()})
    ref.update({"buf/" + n: b for n, b in r64["buffers"].items() if not n.endswith("num_batches_tracked")})
    return fused, comp, ref


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("C,k", LAYER_CASES)
def test_layer_against_float64_within_four_times_the_composed_path(dev, C, k, training):
    fused, comp, ref = _case(C, k, training)
    assert sorted(k_ for k_ in fused if k_ != "nbt") == sorted(ref)
    assert fused["nbt"] == comp["nbt"] == [1 if training else 0] * 3
    rows = {n: (R.rel(fused[n], ref[n]), R.rel(comp[n], ref[n])) for n in ref}
    print({n: "%.1e / %.1e" % v for n, v in rows.items()})
    over = {n: v for n, v in rows.items() if not v[0] <= max(4.0 * v[1], FLOOR)}
    assert not over, over


@pytest.mark.parametrize("C,k", LAYER_CASES)
def test_layer_gradients_project_onto_the_float64_gradients(dev, C, k):
    """tests/test_gpu_dgcnn.py's check: a backward kernel that drops or mis-scales a term fails here."""
    fused, _, ref = _case(C, k, True)
    big = [n for n in ref if (n.startswith("grad/") or n == "dx") and ref[n].numel() >= 8192]
    assert big
    for n in big:
        g, g64 = fused[n].double().reshape(-1), ref[n].reshape(-1)
        assert abs(float(torch.dot(g - g64, g64))) / float(torch.dot(g64, g64)) <= 1e-3, n


def test_two_runs_give_equal_bits(dev):
    from adaptpoint_amd.point_transformer import StageGraph
    C, k = 64, 16
    p, o, idx = _graph(k)
    _, x, _, w = (t.to(dev) for t in R.layer_inputs(SIZES, C, 3))
    a = _run(_layer(C, k, True), p, x, o, StageGraph(p, o, k, idx), w, True)
    b = _run(_layer(C, k, True), p, x, o, StageGraph(p, o, k, idx.clone()), w, True)
    for n in a:
        if n != "nbt":
            assert torch.equal(a[n], b[n]), n


def test_forward_and_backward_replay_from_a_hipgraph_without_a_memset_node(dev):
    from adaptpoint_amd import graphs
    from adaptpoint_amd.point_transformer import StageGraph
    C, k = 64, 16
    p, o, idx = _graph(k)
    _, x, _, w = (t.to(dev) for t in R.layer_inputs(SIZES, C, 3))
    graph = StageGraph(p, o, k, idx)
    graph.csr(), graph.d                                         # the lists and the offsets: built before capture
    layer = _layer(C, k, True).train()
    leaves = [x.clone().requires_grad_(True), *layer.parameters()]

    def step():
        out = layer([p, leaves[0], o, graph])
        return [out.detach(), *torch.autograd.grad(out, leaves, w)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                # warm-up: allocator pools, lazy initialisation
        step()
    torch.cuda.current_stream().wait_stream(side)
    eager = [t.detach().clone() for t in step()]
    torch.cuda.synchronize()
    gc.collect()
    g, captured, census = graphs.capture(step, leaves=leaves, what="the fused layer's graph")
    print("fused layer graph:", census)
    assert not census.get("memset", 0) and census.get("kernel", 0) >= 12
    for _ in range(2):
        for t in captured:
            t.detach().zero_()
        g.replay()
        torch.cuda.synchronize()
        for e, c in zip(eager, captured):
            assert torch.equal(e, c.detach())


@pytest.mark.parametrize("C,k", [(64, 33), (48, 8)])
def test_uncovered_shapes_run_composed_with_one_fallback_entry(dev, C, k):
    from adaptpoint_amd import set_abstraction as SA
    from adaptpoint_amd.point_transformer import StageGraph
    p, o, idx = _graph(k)
    _, x, _, w = (t.to(dev) for t in R.layer_inputs(SIZES, C, 3))
    graph = StageGraph(p, o, k, idx)
    before = dict(SA.FUSED_FALLBACKS)
    fused = _run(_layer(C, k, True), p, x, o, graph, w, True)
    added = {r: c - before.get(r, 0) for r, c in SA.FUSED_FALLBACKS.items() if c != before.get(r, 0)}
    assert len(added) == 1 and list(added.values()) == [1] and f"k={k}" in next(iter(added)), added
    comp = _run(_layer(C, k, False), p, x, o, graph, w, True)
    assert torch.equal(fused["out"], comp["out"]) and torch.equal(fused["grad/linear_w.2.weight"], comp["grad/linear_w.2.weight"])


def test_a_forward_hook_sends_a_covered_layer_to_the_composed_path_under_its_own_reason(dev):
    from adaptpoint_amd import set_abstraction as SA
    from adaptpoint_amd.point_transformer import StageGraph
    C, k = 32, 8
    p, o, idx = _graph(k)
    _, x, _, w = (t.to(dev) for t in R.layer_inputs(SIZES, C, 3))
    layer = _layer(C, k, True)
    seen = []
    layer.linear_w[2].register_forward_hook(lambda m, i, out: seen.append(tuple(out.shape)))
    before = dict(SA.FUSED_FALLBACKS)
    res = _run(layer, p, x, o, StageGraph(p, o, k, idx), w, True)
    added = [r for r, c in SA.FUSED_FALLBACKS.items() if c != before.get(r, 0)]
    assert len(added) == 1 and "forward hook" in added[0] and "no fused kernel" not in added[0]
    assert seen == [(N, k, C // 8)] and torch.isfinite(res["out"]).all()
