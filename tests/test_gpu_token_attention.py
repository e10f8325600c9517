"""The head-dim-64 kernels of csrc/token_attention.hip -- the forward with its running-max recurrence and masked tail, the
delta kernel, the two backward kernels -- through their raw entries (apn_token_attention_fwd / _bwd) and through
`token_attention.token_attention`, on the problems of tests/token_attention_cases.py against the references of
tests/token_attention_reference.py.

Four kinds of check:
  exact       sign-code keys, 512 * sign-code queries, integer values, plain and BIASED (every real score negative, so an
              unmasked zero pad would win its row): out must EQUAL the group mean, lse the score + r, dV the scatter-add,
              dQ 0, dK its combinatorial value -- no tolerance, at every ragged T;
  float64     the regimes of attention_cases.REGIMES against float64: an element-wise bar derived from the arithmetic
              (bar 1) and ||kernel - f64|| <= 4 ||model - f64|| + 2e-6 ||f64|| per quantity (bar 2);
  containment every input lies in a NaN-filled parent, every output and the scratch in a sentinel-filled one (every raw
              call in this file): no NaN comes out, no sentinel outside changes, none inside is left -- the rows of the
              last partial tile of dqkv included;
  invariants  results that must agree bit for bit: two runs, a cloud alone / in a batch, a head alone / among six,
              grad / no-grad forward, the autograd Function against the raw entries, a captured graph replayed twice
              (whose census holds no memset node).

MEASURED (MI355X, whole-file run; test_zz prints them): see the table below the imports.
"""
import gc

import pytest
import torch

import token_attention_cases as TC
import token_attention_reference as TR

pytestmark = pytest.mark.gpu

# Per regime and quantity, worst over the cases of the regime, as bar1/L2/k/m:
#   bar1 = max |kernel - f64| / bar 1 (element-wise), L2 = ||kernel - f64|| / ||f64||, k/m = ||kernel - f64|| / ||model - f64||
# Measured on an MI355X (whole-file run):
#   n0.25    out 0.033/4.76e-06/1.00  lse 0.021/4.75e-06/1.02  dq 0.004/6.44e-06/1.13  dk 0.003/6.48e-06/1.12  dv 0.040/4.93e-06/1.00
#   n1       out 0.012/6.07e-06/1.00  lse 0.015/3.30e-07/1.01  dq 0.004/8.23e-06/1.00  dk 0.003/8.40e-06/1.00  dv 0.014/6.69e-06/1.00
#   n2       out 0.015/8.58e-06/1.00  lse 0.034/3.87e-06/1.01  dq 0.004/2.26e-05/1.01  dk 0.006/2.21e-05/1.01  dv 0.015/9.18e-06/1.00
#   n4       out 0.029/1.05e-05/1.00  lse 0.066/1.53e-06/1.00  dq 0.007/1.73e-05/1.00  dk 0.006/1.71e-05/1.00  dv 0.024/1.11e-05/1.01
#   n8       out 0.025/1.49e-05/1.00  lse 0.061/2.02e-06/1.00  dq 0.007/n/a*/1.01  dk 0.011/n/a*/1.01  dv 0.031/1.53e-05/1.00
#   offset   out 0.004/1.38e-06/1.02  lse 0.027/4.11e-07/1.01  dq 0.001/1.31e-04/1.01  dk 0.001/3.11e-05/1.03  dv 0.009/1.39e-05/1.01
#   binades  out 0.115/1.75e-05/1.01  lse 0.252/5.63e-06/1.02  dq 0.070/2.50e-05/1.00  dk 0.043/2.68e-05/1.01  dv 0.103/1.77e-05/1.00
#   late-max out 0.023/8.65e-06/1.00  lse 0.042/5.01e-07/1.00  dq 0.003/3.21e-05/1.01  dk 0.002/1.19e-05/1.03  dv 0.013/9.29e-06/1.01
#   q0       out 0.001/3.97e-08/1.00  lse 0.326/9.12e-08/1.00  dq 0.012/5.98e-06/1.00  dk 0.000/0.00e+00/0.00  dv 0.055/4.22e-06/1.01
# Worst bar-1 ratio 0.326 (lse of B1-T300-H6-q0), worst kernel / model 1.13 (dq of n0.25).
# (*) n8 includes B1-T1-H1, where dq and dk are exactly 0 in float64 (one key: dS = 0) and a relative L2 says nothing;
#     the kernel's |dq|, |dk| there are rounding residue inside bar 1.  q0: dk is exactly 0 (q = 0) in kernel, model and float64.
# The kernels do what the model says (k/m 1.00 .. 1.13): the error is the two-plane arithmetic's own.
# Wall time of this file on an MI355X: 5.5 s (87 tests).

QUANT = ("out", "lse", "dq", "dk", "dv")
WORST = {}


def _call(*a):
    from adaptpoint_amd.fused import _call as call
    return call(*a)


def _raw(dev, qkv, H, g=None):
    """apn_token_attention_fwd (+ _bwd with g) on poisoned buffers, sized exactly as adaptpoint_amd/token_attention.py sizes
    them; the containment assertions; -> dict of float32 views out, lse[, delta, dqkv]."""
    B, T, C3 = qkv.shape
    C = C3 // 3
    x = TC.in_nan_parent(qkv)
    shapes = {"out": (B, T, C), "lse": (B, H, T)}
    if g is not None:
        shapes.update(delta=(B, H, T), dqkv=(B, T, C3))
    bufs = {}
    for name, shape in shapes.items():
        n = 1
        for s in shape:
            n *= s
        bufs[name] = TC.in_sentinel_parent(4 * n, dev)
    ptr = lambda name: bufs[name][0].data_ptr()
    assert all(ptr(name) % 16 == 0 and ptr(name) != bufs[name][1].data_ptr() for name in bufs)
    _call("apn_token_attention_fwd", dev, B, T, H, x.data_ptr(), ptr("out"), ptr("lse"))
    if g is not None:
        gn = TC.in_nan_parent(g)
        _call("apn_token_attention_bwd", dev, B, T, H, x.data_ptr(), ptr("out"), ptr("lse"), gn.data_ptr(), ptr("delta"),
              ptr("dqkv"))
    res = {}
    for name, (view, parent) in bufs.items():
        assert TC.borders_intact(parent), f"{name}: a sentinel outside the buffer changed"
        assert bool((view != TC.SENTINEL).all()), f"{name}: a part of the buffer was never written"
        res[name] = view.view(torch.float32).view(shapes[name])
        assert not bool(torch.isnan(res[name]).any()), f"{name}: a NaN from outside the inputs came in"
    return res


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


# ---- exact ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", TC.EXACT, ids=[c.name for c in TC.EXACT])
def test_exact_cases_hold_with_no_tolerance(dev, case):
    st = TC.exact_structure(case)
    for variant in ("wide", "narrow"):
        v, dO = TC.exact_values(case, variant)
        out, dq, dk, dv, lse, _ = TC.exact_expect(case, st, v, dO)
        got = _raw(dev, TC.pack(st["q"], st["k"], v).to(dev), case.H, dO.to(dev))
        gq, gk, gv = (t.cpu().double() for t in TC.unpack(got["dqkv"]))
        assert torch.equal(got["out"].cpu().double(), out), (case.name, variant, "out")
        assert torch.equal(got["lse"].cpu(), lse), (case.name, variant, "lse")
        assert torch.equal(gv, dv), (case.name, variant, "dv")
        if variant == "narrow":
            assert bool((gq == 0).all()), (case.name, "dq")
            assert torch.equal(gk, dk), (case.name, "dk")


# ---- float64 --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", TC.FLOAT, ids=[c.name for c in TC.FLOAT])
def test_float_cases_against_float64(dev, case):
    qkv, g = TC.float_inputs(case, dev)
    H = case.H
    got = _raw(dev, qkv, H, g)
    ref = TR.float64(qkv, H, g)
    mod = TR.model(qkv, H, g)
    for res in (got, ref, mod):
        res["dq"], res["dk"], res["dv"] = TC.unpack(res["dqkv"])
    ref["bar_dq"], ref["bar_dk"], ref["bar_dv"] = TC.unpack(ref["bar_dqkv"])
    for name in QUANT:
        err = (got[name].double() - ref[name]).abs()
        ratio = float((err / ref["bar_" + name].clamp_min(1e-300)).max())
        norm, merr = float(ref[name].norm()), float((mod[name].double() - ref[name]).norm())
        l2 = float(err.norm())
        key = (case.regime, name)
        old = WORST.get(key, [0.0, 0.0, 0.0, ""])
        WORST[key] = [max(old[0], ratio), max(old[1], l2 / norm if norm else 0.0), max(old[2], l2 / merr if merr else 0.0),
                      case.name if ratio >= old[0] else old[3]]
        print(f"{case.name} {name}: bar1 {ratio:.3f}  L2 {l2 / norm if norm else 0.0:.2e}  k/m {l2 / merr if merr else 0.0:.2f}")
        assert ratio <= 1.0, (case.name, name, "bar 1", ratio)
        assert l2 <= 4 * merr + 2e-6 * norm, (case.name, name, "bar 2", l2, merr, norm)


# ---- invariants -------------------------------------------------------------------------------------------------------------

def _autograd(qkv, H, w):
    from adaptpoint_amd import token_attention as TA
    leaf = qkv.detach().clone().requires_grad_(True)
    out = TA.token_attention(leaf, H)
    out.backward(w)
    return [out.detach(), leaf.grad]


@pytest.mark.parametrize("shape", [(5, 65, 6), (2, 129, 6), (2, 300, 6), (2, 33, 6)], ids=lambda s: "x".join(map(str, s)))
def test_results_do_not_depend_on_the_run_the_batch_the_heads_or_on_grad(dev, shape):
    from adaptpoint_amd import token_attention as TA
    B, T, H = shape
    before = sum(TA.COMPOSED_CALLS.values())
    qkv, w = TC.float_inputs(TC.Float("inv", B, T, H, "n2"), dev)
    a, b = _raw(dev, qkv, H, w), _raw(dev, qkv, H, w)
    names = ("out", "lse", "delta", "dqkv")
    assert _same([a[n] for n in names], [b[n] for n in names]), "two runs"
    full = _autograd(qkv, H, w)
    assert _same(full, [a["out"], a["dqkv"]]), "the autograd Function against the raw entries"
    with torch.no_grad():
        assert torch.equal(TA.token_attention(qkv, H), full[0]), "no-grad forward"
    one = _autograd(qkv[B - 1:], H, w[B - 1:])
    assert _same(one, [t[B - 1:] for t in full]), "a cloud alone / in the batch"
    h, D = H - 2, TC.HEAD_DIM
    pick = torch.cat([torch.arange(D) + part * H * D + h * D for part in range(3)]).to(dev)
    alone = _autograd(qkv[..., pick].contiguous(), 1, w[..., h * D:(h + 1) * D].contiguous())
    assert _same(alone, [full[0][..., h * D:(h + 1) * D], full[1][..., pick]]), "a head alone / among six"
    assert sum(TA.COMPOSED_CALLS.values()) == before


@pytest.mark.parametrize("shape", [(2, 65, 6), (3, 257, 2)], ids=lambda s: "x".join(map(str, s)))
def test_captured_forward_and_backward_replays_the_same_bits_without_a_memset_node(dev, shape):
    from adaptpoint_amd import token_attention as TA, graphs
    B, T, H = shape
    qkv, w = TC.float_inputs(TC.Float("graph", B, T, H, "n2"), dev)
    eager = _autograd(qkv, H, w)
    leaf = qkv.detach().clone().requires_grad_(True)

    def step():
        out = TA.token_attention(leaf, H)
        (grad,) = torch.autograd.grad(out, [leaf], w)
        return [out.detach(), grad]
    torch.cuda.synchronize()
    gc.collect()
    graph, captured, census = graphs.capture(step, leaves=[leaf], what="token attention forward + backward")
    print("token attention graph:", census)
    assert not census.get("memset", 0)
    for _ in range(2):
        for t in captured:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert _same(eager, captured)


def test_other_head_dims_fall_back_and_are_counted(dev):
    from adaptpoint_amd import token_attention as TA
    before = dict(TA.COMPOSED_CALLS)
    qkv = torch.randn(2, 17, 3 * 2 * 32, device=dev)
    assert not TA.supported(qkv, 2) and TA.supported(torch.randn(2, 17, 3 * 2 * 64, device=dev), 2)
    out = TA.token_attention(qkv, 2)
    new = {r: c - before.get(r, 0) for r, c in TA.COMPOSED_CALLS.items() if c != before.get(r, 0)}
    assert list(new.values()) == [1] and "head dim 32" in list(new)[0], new
    assert torch.equal(out, TA.composed(qkv, 2))


def test_zz_worst_figures_of_this_run(dev):
    """Prints, per regime and quantity, the worst bar-1 ratio (with its case), relative L2 and kernel / model ratio over
    whatever ran before it in this process (the table in the header comes from a whole-file run)."""
    for (regime, name), (ratio, l2, km, at) in sorted(WORST.items()):
        print(f"MEASURED {regime:>14} {name:>3}: bar1 {ratio:.3f} ({at})  L2 {l2:.2e}  k/m {km:.2f}")
