"""The attention kernels of csrc/attention.hip -- the image kernel, the MFMA forward with its running-max recurrence, the
two MFMA backward kernels, the one-wave float32 kernel for M <= 32 -- through their raw entries (apn_attention_prep /
_fwd / _bwd, apn_attention_small_fwd / _bwd) and through `attention.attention`, on the problems of tests/attention_cases.py
against the references of tests/attention_reference.py.

Four kinds of check:
  exact       sign-code keys, 256 * sign-code queries, integer values: out must EQUAL the gathered value / the group mean,
              dV the scatter-add, dQ 0, dK its combinatorial value, lse the score + r -- no tolerance;
  float64     Gaussian, offset, random-binade, late-maximum and q = 0 inputs against float64: an element-wise bar derived
              from the arithmetic (bar 1) and a relative-L2 bar against the model of the kernels' arithmetic (bar 2);
  containment every input lies in a NaN-filled parent, every output, the images and the scratch in a sentinel-filled one
              (every raw call in this file): no NaN comes out, no sentinel outside changes, none inside is left;
              the images are looked at: hi + lo against the scaled input, trans against rows;
  invariants  results that must agree bit for bit (runs, batching, heads, grad / no-grad, subsets of gradients, strides,
              power-of-two scaling, a captured graph replayed).

The measured worst ratios per regime and quantity stand below the imports; test_zz prints them for a whole-file run.
"""
import gc
import math

import pytest
import torch

import attention_cases as AC
import attention_reference as AR

pytestmark = pytest.mark.gpu

# Per regime and quantity, measured on an MI355X (whole-file run), worst over the cases of the regime, as bar1/L2/k/m:
#   bar1 = max |kernel - f64| / bar 1 (element-wise), L2 = ||kernel - f64|| / ||f64||, k/m = ||kernel - f64|| / ||model - f64||
#   n0.25    out 0.026/5.03e-06/1.00  lse 0.041/8.46e-08/1.02  dq 0.009/7.17e-06/1.01  dk 0.007/6.72e-06/1.00  dv 0.020/5.92e-06/1.01
#   n1       out 0.015/7.26e-06/1.00  lse 0.047/3.10e-07/1.00  dq 0.006/9.18e-06/1.01  dk 0.007/8.75e-06/1.01  dv 0.019/7.43e-06/1.00
#   n2       out 0.030/1.25e-05/1.00  lse 0.140/1.07e-06/1.00  dq 0.008/1.49e-05/1.01  dk 0.009/1.41e-05/1.01  dv 0.023/1.33e-05/1.00
#   n4       out 0.049/1.44e-05/1.00  lse 0.175/1.64e-06/1.00  dq 0.019/2.04e-05/1.00  dk 0.015/1.90e-05/1.01  dv 0.036/1.48e-05/1.00
#   n8       out 0.076/2.16e-05/1.00  lse 0.208/2.25e-06/1.01  dq 0.038/3.76e-05/1.00  dk 0.027/3.56e-05/1.00  dv 0.087/2.17e-05/1.00
#   offset   out 0.007/3.63e-06/1.02  lse 0.078/1.10e-06/1.00  dq 0.001/2.43e-04/1.02  dk 0.001/7.68e-05/1.04  dv 0.022/5.61e-05/1.01
#   binades  out 0.145/2.52e-05/1.02  lse 0.374/4.09e-06/1.00  dq 0.098/3.30e-05/1.00  dk 0.045/4.58e-05/1.00  dv 0.108/2.42e-05/1.00
#   late-max out 0.017/1.75e-05/1.00  lse 0.095/7.11e-07/1.00  dq 0.003/5.26e-05/1.00  dk 0.005/1.93e-05/1.00  dv 0.017/1.80e-05/1.01
#   q0       out 0.000/2.85e-08/1.00  lse 0.116/3.25e-08/1.00  dq 0.013/5.76e-06/1.01  dk exact 0  dv 0.024/5.33e-06/1.09
# MFMA path: worst bar-1 ratio 0.374 (lse of B2-M1024-H4-binades), worst kernel / model 1.09 (dv of B5-M288-H3-q0).
# Few points (float32 kernel; bar 1 with 32 * 2^-24 per product, bar 2 against the float32 composition):
#   worst bar-1 ratio 0.036 (out of B32-M26-H4-q0), worst relative L2 6.74e-06 (dq of B32-M23-H16-offset),
#   worst kernel / composition 1.56 (dq of B32-M23-H16-offset).
# The kernels do what the model says (k/m 1.00 .. 1.1): the error is the two-plane arithmetic's own, and it grows with
# the score magnitude.  On the CPU the MODEL was observed at <= 0.15 of bar 1 (lse: 0.37, random binades) and the float32
# composition at <= 0.003 (tests/test_attention_cases_cpu.py prints them and asserts <= 1 and <= 0.05).
# Wall time of this file on an MI355X: 12 s (137 tests; the whole GPU suite: 181 s in the same visit).
# Mutation check (each mutation built into a scratch library; tests failing in this file / in tests/test_gpu_attention.py):
#   at_perm_key with s and h exchanged (image kernel)    67 / 7
#   tmax exchange between half-waves dropped             58 / 7
#   lsum without alpha                                   52 / 6
#   delta from g_out * g_out                             70 / 6
#   0.25 dropped from the Kt4 image                      52 / 6
#   lo plane of P zeroed in attn_bwd_kv                  44 / 6
#   small kernel: mine = lane <= m                       63 / 5
#   delta from the hi plane of dO only                   52 / 6
#   hi planes truncated, not rounded (image kernel)      19 / 0
# The last one is caught by this file alone (14 float cases through bar 2 on lse, which moves to 5-10x the model's
# error, and the four image tests); the older file never looks at lse.  The others are caught by both.

QUANT = ("out", "lse", "dq", "dk", "dv")
WORST = {}                      # (regime, quantity) -> [bar-1 ratio, relative L2, kernel / model, case of the bar-1 ratio]


def _call(*a):
    from adaptpoint_amd.fused import _call as call
    return call(*a)


def _f32(view, shape):
    return view.view(torch.float32).view(shape)


def _all_written(view, halves=False):
    """No sentinel is left inside: word by word for float32 buffers, bf16 by bf16 for the bf16 images (each half of the
    sentinel in its own position: 1.03e7 and 8.5e18 as bf16, values no plane of these inputs takes) -- the smallest
    units the kernels store."""
    if not halves:
        return bool((view != AC.SENTINEL).all())
    h = view.view(torch.int16).view(-1, 2)
    lo, hi = AC.SENTINEL & 0xFFFF, AC.SENTINEL >> 16
    return bool(((h[:, 0] != lo) & (h[:, 1] != hi)).all())


def _raw(dev, q, k, v, H, g=None, grad=None):
    """apn_attention_prep + _fwd (+ _bwd with g) on poisoned buffers, sized exactly as adaptpoint_amd/attention.py sizes
    them; the containment assertions; -> dict of views (out, lse, images as bf16[, dq, dk, dv, scratch])."""
    grad = (g is not None) if grad is None else grad
    B, M, C = q.shape
    n = B * H * M * 32
    ins = [AC.in_nan_parent(t) for t in (q, k, v)]
    bufs = {"images": AC.in_sentinel_parent(2 * n * (6 if grad else 3), dev), "out": AC.in_sentinel_parent(4 * B * M * C, dev),
            "lse": AC.in_sentinel_parent(4 * B * H * M, dev)}
    ptr = lambda name: bufs[name][0].data_ptr()
    assert all(ptr(name) % 16 == 0 and ptr(name) != bufs[name][1].data_ptr() for name in bufs)
    _call("apn_attention_prep", dev, B, M, H, ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(), ptr("images"), 1 if grad else 0)
    _call("apn_attention_fwd", dev, B, M, H, ptr("images"), ptr("out"), ptr("lse"))
    if g is not None:
        assert grad
        gn = AC.in_nan_parent(g)
        bufs["scratch"] = AC.in_sentinel_parent(2 * n * 2 + B * H * M * 4, dev)
        for name in ("dq", "dk", "dv"):
            bufs[name] = AC.in_sentinel_parent(4 * B * M * C, dev)
        _call("apn_attention_bwd", dev, B, M, H, ptr("images"), ptr("out"), ptr("lse"), gn.data_ptr(), ptr("scratch"),
              ptr("dq"), ptr("dk"), ptr("dv"))
    res = {}
    for name, (view, parent) in bufs.items():
        assert AC.borders_intact(parent), f"{name}: a sentinel outside the buffer changed"
        if name == "scratch":          # two bf16 images of dO, then delta in float32
            written = _all_written(view[:n], halves=True) and _all_written(view[n:])
        else:
            written = _all_written(view, halves=name == "images")
        assert written, f"{name}: a part of the buffer was never written"
        if name == "images":
            res[name] = view.view(torch.bfloat16)
        elif name == "scratch":
            res[name] = view
        else:
            res[name] = _f32(view, (B, H, M) if name == "lse" else (B, M, C))
        t = res[name] if name != "scratch" else view[:n].view(torch.bfloat16)
        assert not bool(torch.isnan(t.float()).any()), f"{name}: a NaN from outside the inputs came in"
        if name == "scratch":
            assert not bool(torch.isnan(view[n:].view(torch.float32)).any()), "scratch: a NaN in delta"
    return res


def _raw_small(dev, q, k, v, H, g=None):
    B, M, C = q.shape
    ins = [AC.in_nan_parent(t) for t in (q, k, v)]
    names = ("out",) if g is None else ("dq", "dk", "dv")
    bufs = {name: AC.in_sentinel_parent(4 * B * M * C, dev) for name in names}
    ptrs = [bufs[name][0].data_ptr() for name in names]
    if g is None:
        _call("apn_attention_small_fwd", dev, B, M, H, *(t.data_ptr() for t in ins), *ptrs)
    else:
        gn = AC.in_nan_parent(g)
        _call("apn_attention_small_bwd", dev, B, M, H, *(t.data_ptr() for t in ins), gn.data_ptr(), *ptrs)
    res = {}
    for name, (view, parent) in bufs.items():
        assert AC.borders_intact(parent), f"{name}: a sentinel outside the buffer changed"
        assert bool((view != AC.SENTINEL).all()), f"{name}: a part of the buffer was never written"
        res[name] = _f32(view, (B, M, C))
        assert not bool(torch.isnan(res[name]).any()), name
    return res


# ---- exact ------------------------------------------------------------------------------------------------------------------

def _score_log2():
    """The matching key's score as the kernels form it: q = 256 times 0.25f * log2(e) in float32, split into two bf16
    planes, against +-1 keys (one plane): 16 lo + 16 hi, every step exact in float32."""
    c = 256.0 * (torch.tensor(0.25, dtype=torch.float32) * torch.tensor(AR.LOG2E, dtype=torch.float32))
    hi, lo = AR.split(c)
    return float(16.0 * lo + 16.0 * hi)


def _exact(dev, case, run):
    st = AC.exact_structure(case)
    q, k = st["q"].to(dev), st["k"].to(dev)
    for variant in ("wide", "narrow"):
        v, dO = AC.exact_values(case, variant)
        out, dq, dk, dv, _ = AC.exact_expect(case, st, v, dO)
        got = run(q, k, v.to(dev), dO.to(dev))
        eq = lambda name, want: torch.equal(got[name].double().cpu(), want)
        assert eq("out", out), (case.name, variant, "out")
        assert eq("dv", dv), (case.name, variant, "dv")
        if variant == "narrow":
            assert bool((got["dq"] == 0).all()), (case.name, "dq")
            assert eq("dk", dk), (case.name, "dk")
        if "lse" in got:
            # s - lse is exactly 0 or -r: lse = score + log2(group size), both exact
            want = torch.tensor(_score_log2(), dtype=torch.float32) + torch.log2(
                torch.gather(st["size"], 2, st["tkey"]).float())
            assert torch.equal(got["lse"].cpu(), want), (case.name, "lse")


@pytest.mark.parametrize("case", AC.EXACT_MFMA, ids=[c.name for c in AC.EXACT_MFMA])
def test_exact_cases_on_the_mfma_path(dev, case):
    """out == the targeted value / group mean, dV == the scatter-add over the targeting queries / 2^r, dQ == 0,
    dK == its combinatorial value, lse == score + r, with no tolerance (tests/attention_cases.py has the argument: a gap
    of 184 log2 units, exp2(0) = 1, alpha = exp2(0) or exp2(-184) = 0, integer partial sums; k has no low plane, so
    the score of a pair is the same sum of the same products in the forward and in both backward kernels and the
    backward's s - lse is exactly 0 or -r)."""
    _exact(dev, case, lambda q, k, v, g: _raw(dev, q, k, v, case.H, g))


@pytest.mark.parametrize("m", range(1, 32))
def test_exact_cases_on_the_kernel_for_few_points(dev, m):
    """Every M from 1 to 31: the float32 kernel's scores are integer fmas, exp(0) = 1, exp(-128) = 0: the same equalities."""
    for case in [c for c in AC.EXACT_SMALL if c.M == m]:
        def run(q, k, v, g, H=case.H):
            res = _raw_small(dev, q, k, v, H)
            res.update(_raw_small(dev, q, k, v, H, g))
            return res
        _exact(dev, case, run)


# ---- float64 ----------------------------------------------------------------------------------------------------------------

def _bars(case, got, ref, mod, with_model=True):
    for name in QUANT:
        if name not in got:
            continue
        want = ref[name]
        err = (got[name].double() - want).abs()
        ratio = float((err / ref["bar_" + name].clamp_min(1e-300)).max())
        l2 = float(err.norm() / want.norm().clamp_min(1e-300))
        km = float("nan")
        if with_model:
            merr = float((mod[name].double() - want).norm())
            km = float(err.norm()) / max(merr, 1e-300)
        w = WORST.setdefault((case.regime, name), [0.0, 0.0, 0.0, ""])
        if ratio > w[0]:
            w[0], w[3] = ratio, case.name
        w[1] = max(w[1], l2)
        if with_model and km == km and merr > 0:
            w[2] = max(w[2], km)
        print(f"{case.name} {name}: bar-1 ratio {ratio:.3f}, relative L2 {l2:.3e}, kernel/model {km:.3f}")
        # bar 1: element-wise, derived (tests/attention_reference.py: float64)
        assert bool((err <= ref["bar_" + name]).all()), (case.name, name, ratio)
        # bar 2: what tests/test_gpu_invres.py grants a fused path over its composed one (another summation order,
        # hardware exp2 / log2): 4 x the model's own error + 2e-6
        if with_model:
            assert float(err.norm()) <= 4.0 * merr + 2e-6 * float(want.norm()), (case.name, name, km, l2)


@pytest.mark.parametrize("case", AC.FLOAT_MFMA, ids=[c.name for c in AC.FLOAT_MFMA])
def test_float_cases_on_the_mfma_path(dev, case):
    q, k, v, g = AC.float_inputs(case, dev)
    got = _raw(dev, q, k, v, case.H, g)
    ref = AR.float64(q, k, v, case.H, g)
    mod = AR.model(q, k, v, case.H, g)
    _bars(case, got, ref, mod)
    if case.regime == "q0" and case.M & (case.M - 1) == 0:
        # uniform soft-max over 2^n keys of integer values: the mean, exactly
        mean = AC.merged(AC.per_head(v, case.H).double().mean(2, keepdim=True).expand(-1, -1, case.M, -1))
        assert torch.equal(got["out"].double(), mean)
        assert bool((got["lse"] == math.log2(case.M)).all())


@pytest.mark.parametrize("case", AC.FLOAT_SMALL, ids=[c.name for c in AC.FLOAT_SMALL])
def test_float_cases_on_the_kernel_for_few_points(dev, case):
    """Bar 1 with the constant of one product at 32 * 2^-24 instead of the split's 3 * 2^-16: the float32 kernel splits
    nothing, and its longest chain of float32 fmas (a sum over at most 32 keys or queries) has a worst-case error of
    32 * 2^-24 of the sum of the magnitudes.  Bar 2 against the float32 composition on the same device -- for a float32
    kernel the composition IS the plain statement of its arithmetic (float32 throughout, another order of the sums,
    another exp): ||kernel - f64|| <= 4 ||composition - f64|| + 2e-6 ||f64||, as for the MFMA path and its model."""
    from adaptpoint_amd.attention import _reference
    q, k, v, g = AC.float_inputs(case, dev)
    got = _raw_small(dev, q, k, v, case.H)
    got.update(_raw_small(dev, q, k, v, case.H, g))
    ref = AR.float64(q, k, v, case.H, g, C2=32 * AR.EPS)
    leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
    comp = _reference(*leaves, case.H)
    comp.backward(g)
    mod = dict(out=comp.detach(), dq=leaves[0].grad, dk=leaves[1].grad, dv=leaves[2].grad)
    _bars(case._replace(regime="few-" + case.regime), got, ref, mod)


# ---- the images ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(2, 32, 4), (1, 64, 3), (3, 288, 2), (2, 544, 1)], ids=lambda s: "x".join(map(str, s)))
def test_operand_images(dev, shape):
    """hi + lo reproduces x * scale within 2^-17 |x * scale| (two round-to-nearest planes of 8 bits: 2^-9 * 2^-9 = 2^-18,
    + the rounding of x * scale itself); each trans image is its rows counterpart transposed with every 32-tile in
    accumulator-row order, after undoing the scale (a power of two, or against the same float32 product); the
    forward-only prep writes the first three images and they equal the first three of the full prep."""
    B, M, H = shape
    case = AC.Float("images", B, M, H, "binades")
    q, k, v, g = AC.float_inputs(case, dev)
    res = _raw(dev, q, k, v, H, g)
    n = B * H * M * 32
    img = res["images"]
    assert torch.equal(_raw(dev, q, k, v, H)["images"], img[:3 * n])
    qh, kh, vh, gh = (AC.per_head(t, H) for t in (q, k, v, g))
    scale = float(torch.tensor(0.25, dtype=torch.float32) * torch.tensor(AR.LOG2E, dtype=torch.float32))
    scratch = res["scratch"]
    gs, gt = scratch[:n // 2].view(torch.bfloat16), scratch[n // 2:n].view(torch.bfloat16)
    rows = {"Qs": (img[:n], qh * scale), "Ks": (img[n:2 * n], kh), "Vs": (img[3 * n:4 * n], vh), "dOs": (gs, gh)}
    trans = {"Vt": (img[2 * n:3 * n], vh), "Qt4": (img[4 * n:5 * n], qh * 0.25), "Kt4": (img[5 * n:], kh * 0.25), "dOt": (gt, gh)}
    planes = {}
    for name, (im, x) in list(rows.items()) + list(trans.items()):
        hi, lo = (AR.rows_image if name in rows else AR.trans_image)(im, B, H, M)
        planes[name] = (hi, lo)
        assert bool(((hi.double() + lo.double() - x.double()).abs() <= 2.0 ** -17 * x.double().abs()).all()), name
        want = AR.split(x)                                           # round to nearest even, the remainder in float32
        assert torch.equal(hi, want[0]) and torch.equal(lo, want[1]), name
    for t, r, s in (("Vt", "Vs", 1.0), ("Kt4", "Ks", 0.25), ("dOt", "dOs", 1.0)):
        for part in (0, 1):
            assert torch.equal(planes[t][part], planes[r][part] * s), (t, r, part)
    # delta = rowsum(dO * O), after the two images of dO in the scratch
    delta = scratch[n:].view(torch.float32).view(B, H, M)
    want = (gh.double() * AC.per_head(res["out"], H).double()).sum(-1)
    mag = (gh.double() * AC.per_head(res["out"], H).double()).abs().sum(-1)
    assert bool(((delta.double() - want).abs() <= 18 * 2.0 ** -24 * mag).all())


# ---- invariants -------------------------------------------------------------------------------------------------------------

def _autograd(q, k, v, H, w, needs=(True, True, True)):
    from adaptpoint_amd import attention as A
    leaves = [t.detach().clone().requires_grad_(n) if n else t for t, n in zip((q, k, v), needs)]
    out = A.attention(*leaves, H)
    if any(needs):
        out.backward(w)
    return [out.detach()] + [t.grad if n else None for t, n in zip(leaves, needs)]


def _same(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


INVARIANT_SHAPES = [(3, 288, 3), (2, 1024, 4), (5, 32, 2), (3, 7, 2), (32, 4, 4)]


@pytest.mark.parametrize("shape", INVARIANT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bit_level_invariants(dev, shape):
    """Two runs; cloud b alone; head h alone; the forward without grad; any subset of gradients; strided and expanded
    inputs and an expanded g; power-of-two scaling of v and dO -- all bit for bit, and nothing composed."""
    from adaptpoint_amd import attention as A
    B, M, H = shape
    q, k, v, w = AC.float_inputs(AC.Float("inv", B, M, H, "n2"), dev)
    before = sum(A.COMPOSED_CALLS.values())
    full = _autograd(q, k, v, H, w)
    assert _same(full, _autograd(q, k, v, H, w)), "two runs"
    for b in {0, B - 1}:
        one = _autograd(q[b:b + 1], k[b:b + 1], v[b:b + 1], H, w[b:b + 1])
        assert _same([t[b:b + 1] for t in full], one), ("cloud", b)
    for h in {0, H - 1}:
        sl = slice(16 * h, 16 * h + 16)
        one = _autograd(q[..., sl], k[..., sl], v[..., sl], 1, w[..., sl])
        assert _same([t[..., sl] for t in full], one), ("head", h)
    with torch.no_grad():
        assert torch.equal(A.attention(q, k, v, H), full[0]), "the forward without grad (three images)"
    for needs in [(True, False, False), (False, True, False), (False, False, True), (True, True, False), (False, True, True),
                  (True, False, True)]:
        part = _autograd(q, k, v, H, w, needs)
        assert _same([full[0]] + [f if n else None for f, n in zip(full[1:], needs)], part), needs
    # strided (a slice of a wider tensor, a transposed copy), and a cloud expanded over the batch
    wide = torch.randn(B, M, 3 * H * 16 + 5, device=dev)
    wide[..., 2:2 + H * 16] = q
    assert _same(full, _autograd(wide[..., 2:2 + H * 16], k.transpose(0, 1).contiguous().transpose(0, 1), v, H, w)), "strided"
    ke = k[:1].expand(B, -1, -1)
    assert _same(_autograd(q, ke.contiguous(), v, H, w), _autograd(q, ke, v, H, w)), "expanded k"
    leaves = [t.detach().clone().requires_grad_(True) for t in (q, k, v)]
    A.attention(*leaves, H).sum().backward()                     # g arrives as an expanded scalar 1
    ones = _autograd(q, k, v, H, torch.ones_like(w))
    assert _same(ones[1:], [t.grad for t in leaves]), "expanded g"
    for s in (-7, 7):
        scaled = _autograd(q, k, v * 2.0 ** s, H, w)
        assert torch.equal(scaled[0], full[0] * 2.0 ** s), ("v scaled", s)
        scaled = _autograd(q, k, v, H, w * 2.0 ** s)
        assert _same([full[0]] + [t * 2.0 ** s for t in full[1:]], scaled), ("dO scaled", s)
    assert sum(A.COMPOSED_CALLS.values()) == before


@pytest.mark.parametrize("shape", [(2, 288, 3), (3, 7, 2)], ids=lambda s: "x".join(map(str, s)))
def test_captured_forward_and_backward_replay_equals_eager(dev, shape):
    from adaptpoint_amd import attention as A, graphs
    B, M, H = shape
    q, k, v, w = AC.float_inputs(AC.Float("graph", B, M, H, "n2"), dev)
    eager = _autograd(q, k, v, H, w)
    leaves = [t.detach().clone().requires_grad_(True) for t in (q, k, v)]

    def step():
        out = A.attention(*leaves, H)
        grads = torch.autograd.grad(out, leaves, w)
        return [out.detach()] + list(grads)
    torch.cuda.synchronize()
    gc.collect()
    graph, captured, census = graphs.capture(step, leaves=leaves, what="attention forward + backward")
    print("attention graph:", census)
    for _ in range(2):
        for t in captured:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert _same(eager, captured)


# ---- the limits of the grid ---------------------------------------------------------------------------------------------------

def test_batches_above_the_grid_limit_are_composed_and_counted(dev):
    """B = 65536 is no grid dimension: `supported` says so and the composition runs, counted under a reason that names
    the batch; B = 65535 still runs the kernels (here the one for few points, M = 3)."""
    from adaptpoint_amd import attention as A
    gen = torch.Generator().manual_seed(5)
    q, k, v = (torch.randn(65536, 32, 16, generator=gen).to(dev) for _ in range(3))
    assert not A.supported(q, 1) and A.supported(q[:65535], 1)
    many_heads = torch.empty(1, 32, 65536 * 16, device=dev)
    assert not A.supported(many_heads, 65536) and A.supported(many_heads[..., :65535 * 16], 65535)
    assert "heads 65536" in A._why_composed(many_heads, 65536) and "head dim" in A._why_composed(many_heads, 3)
    assert "heads 0" in A._why_composed(many_heads, 0)
    del many_heads
    before = dict(A.COMPOSED_CALLS)
    out = A.attention(q, k, v, 1)
    new = {r: c - before.get(r, 0) for r, c in A.COMPOSED_CALLS.items() if c != before.get(r, 0)}
    assert len(new) == 1 and list(new.values()) == [1] and "batch 65536" in list(new)[0], new
    want = A._reference(q.double(), k.double(), v.double(), 1)
    assert float((out.double() - want).abs().max()) <= 1e-5
    total = sum(A.COMPOSED_CALLS.values())
    q, k, v = (torch.randn(65535, 3, 16, generator=gen).to(dev) for _ in range(3))
    out = A.attention(q, k, v, 1)
    assert sum(A.COMPOSED_CALLS.values()) == total
    want = A._reference(q.double(), k.double(), v.double(), 1)
    assert float((out.double() - want).abs().max()) <= 2e-6 * max(1.0, float(want.abs().max()))


def test_zz_worst_figures_of_this_run(dev):
    """Prints, per regime and quantity, the worst bar-1 ratio (with its case), relative L2 and kernel / model ratio over
    whatever ran before it in this process (the table in the header comes from a whole-file run)."""
    for (regime, name), (ratio, l2, km, at) in sorted(WORST.items()):
        print(f"MEASURED {regime:>14} {name:>3}: bar1 {ratio:.3f} ({at})  L2 {l2:.2e}  k/m {km:.2f}")
        assert ratio <= 1.0, (regime, name, at)
