"""The four kernels of csrc/augment.hip -- apn_anchor_transforms, apn_anchor_transforms_grad, apn_deform_forward,
apn_deform_backward -- through their raw entries, on the problems of tests/augment_cases.py and the fixture
tests/golden/augment_golden.npz, against the float64 restatement of tests/augment_reference.py.

Three kinds of check:
  exact       T1-T5, E1-E3: switched-off factors, prob = 0, prob = +-100, anchor counts around the 64-thread block with a
              guard pattern behind the last anchor, absent optional arguments, integer clouds with planted farthest
              points and ties -- values that must EQUAL what is claimed, no tolerance;
  float64     every element of lin, off, g_prob, z, mu, r, out, g_lin, g_off, g_mask within ITS OWN bar, which the
              restatement derives from the kernels' operation order (its docstring; 4 ulp assumed per tanhf / expf / sinf /
              cosf call -- no accuracy table for them was found in the ROCm installation); the farthest point's index equal;
  invariants  a batch equals its clouds one by one, two runs agree, bit for bit; every output norm is below 1.
Every raw call here writes into buffers with a sentinel-filled tail that is checked afterwards; the transform entries
get buffers padded to whole 64-anchor blocks, so even a kernel without its tail guard stays inside them.

Measured on an MI355X (whole-file run), the largest |kernel - restatement| / bar per tensor, worst over every case:
  lin     0.183  (wide)
  off     0.166  (project)
  g_prob  0.527  (wide)
  z       0.542  (N4096-M1-B3-s0.5-none)
  mu      0.057  (N2-M2-B3-s0.2-none)
  r       0.019  (N257-M8-B3-s0.5-soft)
  out     0.042  (N4096-M1-B3-s0.5-none)
  g_lin   0.009  (N2-M2-B3-s0.2-none)
  g_off   0.006  (fixture-tie)
  g_mask  0.032  (N257-M8-B3-s0.5-soft)
No ratio exceeds 1 (test_zz asserts it).  The bars are worst-case running bounds; the two largest ratios are z at M = 1, where the
bound treats w and 1 / w as independent, and g_prob at w_R_range = 180.
Wall time of this file on an MI355X: 2.3 s (42 tests; the whole GPU suite: 1127 tests in 186 s).
Mutation check (each mutation built into a scratch library, none committed; tests failing in this file / among the four cases
of the two older kernel tests of tests/test_gpu_adaptpoint.py):
  centre entry written as cz*cx (anchor_rotation.h)     9 / 1
  gR[4]*sz*sy dropped from g_sx                         8 / 1
  sign of gR[5]*sx flipped in g_cz                      8 / 1
  tie-break to the highest index                        7 / 0
  forward's point loops cut to 15 iterations            5 / 0
  g_r * e share removed from spread                    23 / 3
  mean divided by the padded count                     17 / 1
  g_mask from the masked gradient                      18 / 3
  tail guard i >= n removed (transforms kernel)        14 / 0
Every mutation fails here; the tie-break, the 15-iteration loop and the missing tail guard pass the older tests untouched.
"""
import os

import numpy as np
import pytest
import torch

import augment_cases as C
import augment_reference as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "augment_golden.npz")
SENT = 12345.671875                      # a float32 value no output takes
TAIL = 64
WORST = {}                               # tensor -> [largest error / bar, case]


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


def _call(*a):
    from adaptpoint_amd.fused import _call as call
    return call(*a)


def _in(dev, a, rows=None):
    """float64 array of float32 values -> a flat device buffer, zero-padded to `rows` leading rows."""
    wide, a = np.asarray(a, np.float64), np.ascontiguousarray(a, np.float32)
    assert np.array_equal(a.astype(np.float64), wide), "an input that is no float32 value"
    if rows is not None and rows > a.shape[0]:
        a = np.concatenate([a, np.zeros((rows - a.shape[0],) + a.shape[1:], np.float32)])
    return torch.from_numpy(a).reshape(-1).to(dev)


def _out(dev, words):
    return torch.full((words + TAIL,), SENT, device=dev)


def _take(buf, shape, what):
    """the result part of a sentinel-tailed buffer as numpy; nothing behind it was written, all of it was"""
    words = int(np.prod(shape))
    host = buf.cpu().numpy()
    assert np.all(host[words:] == np.float32(SENT)), f"{what}: written behind its end"
    return host[:words].reshape(shape).copy()


def _ptr(t):
    return None if t is None else t.data_ptr()


def transforms_raw(dev, prob, keep, axes, ranges, g_lin=None, g_off=None, grad=True, zeros=()):
    """prob (n,9), keep (n,3), axes (n,3) -> lin (n,3,3), off (n,3)[, g_prob (n,9)] float32.  g_lin / g_off None: a null
    pointer, unless named in `zeros` (then an all-zero buffer)."""
    n = prob.shape[0]
    cap = (n + 63) // 64 * 64
    p, k, a = _in(dev, prob, cap), _in(dev, keep, cap), _in(dev, axes, cap)
    lin, off = _out(dev, cap * 9), _out(dev, cap * 3)
    _call("apn_anchor_transforms", dev, n, p.data_ptr(), k.data_ptr(), a.data_ptr(), *map(float, ranges), lin.data_ptr(), off.data_ptr())
    host_lin, host_off = lin.cpu().numpy(), off.cpu().numpy()
    assert np.all(host_lin[n * 9:] == np.float32(SENT)) and np.all(host_off[n * 3:] == np.float32(SENT)), "written behind the last anchor"
    res = [host_lin[:n * 9].reshape(n, 3, 3).copy(), host_off[:n * 3].reshape(n, 3).copy()]
    if grad:
        gl = _in(dev, g_lin if g_lin is not None else np.zeros((n, 3, 3)), cap) if (g_lin is not None or "g_lin" in zeros) else None
        go = _in(dev, g_off if g_off is not None else np.zeros((n, 3)), cap) if (g_off is not None or "g_off" in zeros) else None
        gp = _out(dev, cap * 9)
        _call("apn_anchor_transforms_grad", dev, n, p.data_ptr(), k.data_ptr(), a.data_ptr(), *map(float, ranges), _ptr(gl), _ptr(go),
              gp.data_ptr())
        host = gp.cpu().numpy()
        assert np.all(host[n * 9:] == np.float32(SENT)), "g_prob written behind the last anchor"
        res.append(host[:n * 9].reshape(n, 9).copy())
    return res


def deform_raw(dev, x, anchors, lin, off, axes, mask, sigma, gout=None, want_g_mask=True):
    """-> dict z, mu, r, kfar, out[, g_lin, g_off, g_mask] (numpy float32 / int)"""
    B, N, _ = x.shape
    M = anchors.shape[1]
    xd, ad, ld, od, axd = (_in(dev, t) for t in (x, anchors, lin, off, axes))
    md = None if mask is None else _in(dev, mask)
    z, stat, out = _out(dev, B * N * 3), _out(dev, B * 8), _out(dev, B * N * 3)
    _call("apn_deform_forward", dev, B, N, M, xd.data_ptr(), ad.data_ptr(), ld.data_ptr(), od.data_ptr(), axd.data_ptr(), _ptr(md),
          float(sigma), z.data_ptr(), stat.data_ptr(), out.data_ptr())
    st = _take(stat, (B, 8), "stat")
    res = dict(z=_take(z, (B, N, 3), "z"), out=_take(out, (B, N, 3), "out"), mu=st[:, :3].copy(), r=st[:, 3].copy(),
               kfar=st[:, 4].copy().view(np.int32).astype(np.int64))
    assert np.all(st[:, 5:] == np.float32(SENT))
    assert np.all((res["kfar"] >= 0) & (res["kfar"] < N)), "the stored index is a point of the cloud"
    if gout is not None:
        gd = _in(dev, gout)
        g_lin, g_off = _out(dev, B * M * 9), _out(dev, B * M * 3)
        g_mask = _out(dev, B * N) if want_g_mask else None
        _call("apn_deform_backward", dev, B, N, M, xd.data_ptr(), ad.data_ptr(), axd.data_ptr(), _ptr(md), float(sigma), z.data_ptr(),
              stat.data_ptr(), gd.data_ptr(), g_lin.data_ptr(), g_off.data_ptr(), _ptr(g_mask))
        res.update(g_lin=_take(g_lin, (B, M, 3, 3), "g_lin"), g_off=_take(g_off, (B, M, 3), "g_off"))
        if want_g_mask:
            res["g_mask"] = _take(g_mask, (B, N), "g_mask")
    assert all(np.isfinite(v).all() for v in res.values())
    assert float(np.linalg.norm(res["out"].astype(np.float64), axis=-1).max()) < 1.0, "an output point on or outside the unit sphere"
    return res


def within(name, got, ref, label):
    """every element of `got` within its own bar of the restatement"""
    err = np.abs(got.astype(np.float64) - ref.v)
    ratio = float(np.max(np.where(err > 0, err / np.maximum(ref.e, 1e-300), 0.0))) if err.size else 0.0
    if ratio > WORST.get(name, [0.0])[0]:
        WORST[name] = [ratio, label]
    print(f"{label}: {name} worst error / bar {ratio:.3f} (largest error {float(err.max()):.3e}, bar there "
          f"{float(ref.e.reshape(-1)[err.argmax()]):.3e})")
    assert np.all(err <= ref.e), (label, name, ratio)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


# ---- anchor transforms, exact ----------------------------------------------------------------------------------------------

def test_t1_prob_zero_gives_diag_s_and_no_offset(dev):
    keep, axes = C.switch_table()
    lin, off, _ = transforms_raw(dev, np.zeros((64, 9)), keep, axes, C.RANGES["project"], np.ones((64, 3, 3)), np.ones((64, 3)))
    s = 1.0 + keep[:, 1:2] * axes                                      # sigmoid(0) (3 - 1) + 1 = 2 where on, else 1
    assert np.array_equal(lin.astype(np.float64), s[:, None, :] * np.eye(3)) and np.all(off == 0)


def test_t2_switched_off_factors_are_exact(dev):
    keep, axes = C.switch_table()
    rng = np.random.default_rng(21)
    prob = C.f32(2.0 * rng.normal(size=(64, 9)))
    for ranges in C.RANGES.values():
        lin, off, g = transforms_raw(dev, prob, keep, axes, ranges, C.f32(rng.normal(size=(64, 3, 3))), C.f32(rng.normal(size=(64, 3))))
        no_rot, scale_off, shift_off = keep[:, 0] == 0, (keep[:, 1:2] * axes) == 0, (keep[:, 2:3] * axes) == 0
        assert np.all(lin[no_rot] == lin[no_rot] * np.eye(3, dtype=np.float32)), "keep[0] = 0: R = I exactly"
        assert np.all(g[:, 0:3][no_rot] == 0)
        diag = lin[:, [0, 1, 2], [0, 1, 2]]
        assert np.all(diag[no_rot][scale_off[no_rot]] == 1.0), "a scale switched off is exactly 1"
        assert np.all(diag[no_rot][~scale_off[no_rot]] > 1.0)
        assert np.all(g[:, 3:6][scale_off] == 0) and np.all(g[:, 3:6][~scale_off] != 0)
        assert np.all(off[shift_off] == 0) and np.all(g[:, 6:9][shift_off] == 0) and np.all(off[~shift_off] != 0)


def test_t3_saturated_inputs_stay_finite_and_exact(dev):
    keep, axes = C.switch_table()
    rng = np.random.default_rng(22)
    prob = np.where(rng.integers(0, 2, (64, 9)) == 1, 100.0, -100.0)
    r_range, s_range, t_range = C.RANGES["project"]
    gl, go = C.f32(rng.normal(size=(64, 3, 3))), C.f32(rng.normal(size=(64, 3)))
    lin, off, g = transforms_raw(dev, prob, keep, axes, (r_range, s_range, t_range), gl, go)
    lin1, _, _ = transforms_raw(dev, prob, keep, axes, (r_range, 1.0, t_range), gl, go)      # s_range = 1: lin is R itself
    assert np.isfinite(lin).all() and np.isfinite(off).all() and np.isfinite(g).all()
    assert np.array_equal(off.astype(np.float64), np.sign(prob[:, 6:9]) * t_range * keep[:, 2:3] * axes)
    s = np.where((prob[:, 3:6] > 0) & (keep[:, 1:2] * axes == 1), s_range, 1.0).astype(np.float32)
    assert same_bits(lin, lin1 * s[:, None, :]), "s is exactly s_range or 1"
    assert np.all(g == 0)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 193])
def test_t4_anchor_counts_around_the_block(dev, n):
    """The `i >= n` tail: the last anchor equals the same anchor computed alone, and nothing behind it is written
    (transforms_raw checks the sentinels behind every result)."""
    rng = np.random.default_rng(n)
    prob = C.f32(2.0 * rng.normal(size=(n, 9)))
    keep = rng.integers(0, 2, (n, 3)).astype(np.float64)
    axes = C.axis_bits(rng.integers(1, 8, n))
    gl, go = C.f32(rng.normal(size=(n, 3, 3))), C.f32(rng.normal(size=(n, 3)))
    for ranges in C.RANGES.values():
        whole = transforms_raw(dev, prob, keep, axes, ranges, gl, go)
        for i in sorted({0, n - 1}):
            alone = transforms_raw(dev, prob[i:i + 1], keep[i:i + 1], axes[i:i + 1], ranges, gl[i:i + 1], go[i:i + 1])
            assert all(same_bits(w[i:i + 1], a) for w, a in zip(whole, alone)), (n, i)


def test_t5_absent_gradients_equal_zeros(dev, gold):
    prob, keep, axes = (gold["t_wide_" + k].reshape(512, -1) for k in ("prob", "keep", "axes"))
    gl, go = gold["t_wide_g_lin"].reshape(512, 3, 3), gold["t_wide_g_off"].reshape(512, 3)
    run = lambda **kw: transforms_raw(dev, prob, keep, axes, C.RANGES["wide"], **kw)[2]
    assert same_bits(run(g_lin=None, g_off=go), run(g_lin=None, g_off=go, zeros=("g_lin",)))
    assert same_bits(run(g_lin=gl, g_off=None), run(g_lin=gl, g_off=None, zeros=("g_off",)))
    assert same_bits(run(), run(zeros=("g_lin", "g_off"))) and np.all(run() == 0)


# ---- anchor transforms against the restatement -----------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["project", "wide"])
def test_transforms_within_their_bars(dev, gold, name):
    """The fixture's 512 anchors (all 56 combinations the reference draws) and the 8 keep combinations with axes = 0."""
    k, ranges = f"t_{name}_", C.RANGES[name]
    keep0, axes0 = C.switch_table()
    extra = axes0.sum(1) == 0
    cat = lambda a, b: np.concatenate([a, b])
    prob = cat(gold[k + "prob"].reshape(512, 9), gold[k + "prob"].reshape(512, 9)[:8])
    keep, axes = cat(gold[k + "keep"].reshape(512, 3), keep0[extra]), cat(gold[k + "axes"].reshape(512, 3), axes0[extra])
    gl = cat(gold[k + "g_lin"].reshape(512, 3, 3), gold[k + "g_lin"].reshape(512, 3, 3)[:8])
    go = cat(gold[k + "g_off"].reshape(512, 3), gold[k + "g_off"].reshape(512, 3)[:8])
    lin, off, g = transforms_raw(dev, prob, keep, axes, ranges, gl, go)
    rl, ro = R.anchor_transforms(prob, keep, axes, ranges)
    rg = R.anchor_transforms_grad(prob, keep, axes, ranges, gl, go)
    within("lin", lin, rl, name), within("off", off, ro, name), within("g_prob", g, rg, name)


# ---- deformation, exact ------------------------------------------------------------------------------------------------------

def _exact_out(z, mu, r, mask=None):
    """the float32 statement of out, its single rounding: (z - mu) is exact, s = (1 / r) * 0.999999f is a power of two
    times the constant, so the product rounds once (a 0 / 1 mask changes nothing)"""
    s = (np.float32(1.0) / np.float32(r)) * np.float32(0.999999)
    out = (z.astype(np.float32) - mu.astype(np.float32)[:, None]) * s
    return out if mask is None else out * mask.astype(np.float32)[..., None]


@pytest.mark.parametrize("M", [1, 2, 4, 8])
def test_e1_exact_cloud(dev, M):
    c = C.exact_deform(512, M, C.two_ties(), seed=M)
    hard = (np.random.default_rng(M).uniform(size=(1, 512)) < 0.8).astype(np.float64)
    for mask in (None, hard):
        got = deform_raw(dev, c["x"], c["anchors"], c["lin"], c["off"], c["axes"], mask, 0.5)
        assert same_bits(got["z"], c["z"]) and same_bits(got["mu"], c["mu"]), "z and mu are exact"
        assert float(got["r"][0]) == 8.0 and int(got["kfar"][0]) == 5
        assert same_bits(got["out"], _exact_out(c["z"], c["mu"], 8.0, mask))
        if mask is not None:
            assert np.all(got["out"][mask == 0] == 0)


@pytest.mark.parametrize("ties", ["two", "three"])
def test_e2_ties_take_the_lowest_index(dev, ties):
    """Two / three points at exactly the largest radius, in different waves (5, 70, 300): the stored index is the lowest;
    after a permutation of the cloud it moves with the points; the backward credits that point alone (the restatement's
    lowest-index rule, within bars -- the even split would be far outside them: tests/test_augment_cases_cpu.py)."""
    planted = C.two_ties() if ties == "two" else C.three_ties()
    tied = [i for i, p in planted.items() if max(abs(v) for v in p) == 4.0]
    c = C.exact_deform(512, 4, planted, seed=31)
    rng = np.random.default_rng(32)
    gout = C.f32(rng.normal(size=(1, 512, 3)))
    for trial in range(3):
        perm = np.arange(512) if trial == 0 else rng.permutation(512)
        x, g = c["x"][:, perm], gout[:, perm]
        where_now = [int(np.nonzero(perm == i)[0][0]) for i in tied]
        got = deform_raw(dev, x, c["anchors"], c["lin"], c["off"], c["axes"], None, 0.5, g)
        assert int(got["kfar"][0]) == min(where_now), (ties, trial)
        assert float(got["r"][0]) == 8.0 and same_bits(got["z"], c["z"][:, perm])
        z, mu, r, kfar, out = R.deform(x, c["anchors"], c["lin"], c["off"], c["axes"], None, 0.5)
        assert int(kfar[0]) == min(where_now)
        g_lin, g_off, g_mask = R.deform_grad(x, c["anchors"], c["axes"], None, 0.5, z, mu, r, kfar, g)
        label = f"E2-{ties}-{trial}"
        within("g_lin", got["g_lin"], g_lin, label), within("g_off", got["g_off"], g_off, label)
        within("g_mask", got["g_mask"], g_mask, label)


def test_e2_fixture_tie_cloud(dev, gold):
    """The tie cloud of the fixture through both kernels each way: prob's gradient within its bars of the restatement
    (which reproduces the reference's own gradient to 1e-12 on the CPU)."""
    _chain(dev, gold, "tie_", expect_kfar=5)


def test_e3_the_mask(dev):
    c = C.deform_case(C.DEFORM_TABLE[8])                                  # N = 777, hard mask
    assert c["mask_draw"] is not None
    ones = np.ones_like(c["mask"])
    args = (c["x"], c["anchors"], c["lin"], c["off"], c["axes"])
    hard = deform_raw(dev, *args, c["mask"], c["sigma"], c["gout"])
    assert np.all(hard["out"][c["mask"] == 0] == 0) and np.all(np.abs(hard["out"][c["mask"] == 1]).sum(-1) > 0)
    absent, given = deform_raw(dev, *args, None, c["sigma"], c["gout"]), deform_raw(dev, *args, ones, c["sigma"], c["gout"])
    for k in absent:
        assert same_bits(absent[k], given[k]) if absent[k].dtype == np.float32 else np.array_equal(absent[k], given[k]), k
    without = deform_raw(dev, *args, c["mask"], c["sigma"], c["gout"], want_g_mask=False)
    assert same_bits(without["g_lin"], hard["g_lin"]) and same_bits(without["g_off"], hard["g_off"]) and "g_mask" not in without


# ---- deformation against the restatement ---------------------------------------------------------------------------------

def _deform_within(dev, label, x, anchors, lin, off, axes, mask, sigma, gout, free_kfar=False):
    """forward and backward of one case within bars; lin / off arrays (exact inputs) -> the kernel's results"""
    got = deform_raw(dev, x, anchors, lin, off, axes, mask, sigma, gout)
    z, mu, r, kfar, out = R.deform(x, anchors, lin, off, axes, mask, sigma)
    within("z", got["z"], z, label), within("mu", got["mu"], mu, label), within("r", got["r"], r, label)
    within("out", got["out"], out, label)
    if free_kfar:                   # N = 2: both points are farthest (tests/augment_cases.py); the stored one must be one of them
        rad = R.centred_radii(z.v, mu.v)
        rows = np.arange(len(kfar))
        assert np.all(rad[rows, got["kfar"]] >= rad.max(1) - 2 * r.e)
        kfar = got["kfar"]
    else:
        assert np.array_equal(got["kfar"], kfar), label
    g_lin, g_off, g_mask = R.deform_grad(x, anchors, axes, mask, sigma, z, mu, r, kfar, gout)
    within("g_lin", got["g_lin"], g_lin, label), within("g_off", got["g_off"], g_off, label)
    within("g_mask", got["g_mask"], g_mask, label)
    return got


@pytest.mark.parametrize("row", C.DEFORM_TABLE, ids=C.DEFORM_IDS)
def test_deformation_within_its_bars(dev, row):
    c = C.deform_case(row)
    _deform_within(dev, C.DEFORM_IDS[C.DEFORM_TABLE.index(row)], c["x"], c["anchors"], c["lin"], c["off"], c["axes"], c["mask"],
                   c["sigma"], c["gout"], free_kfar=row[0] == 2)


def _chain(dev, gold, k, expect_kfar=None):
    """A fixture case through all four kernels: transforms -> deformation -> its backward -> the transforms' gradient;
    the restatement runs the same chain and carries each stage's bar into the next."""
    names = ("x", "anchors", "prob", "keep", "axes", "kernel_axes", "gout")
    d = {n: gold[k + n] for n in names}
    B, N, _ = d["x"].shape
    M = d["anchors"].shape[1]
    mask = gold[k + "mask"] if k + "mask" in gold.files else None
    ranges = tuple(float(v) for v in gold[k + "ranges"]) if k + "ranges" in gold.files else C.RANGES["project"]
    sigma = float(gold[k + "sigma"].reshape(-1)[0]) if k + "sigma" in gold.files else 0.5
    flat = lambda a: a.reshape(B * M, -1)
    lin, off, _ = transforms_raw(dev, flat(d["prob"]), flat(d["keep"]), flat(d["axes"]), ranges)
    got = deform_raw(dev, d["x"], d["anchors"], lin.reshape(B, M, 3, 3), off.reshape(B, M, 3), d["kernel_axes"], mask, sigma, d["gout"])
    g_prob = transforms_raw(dev, flat(d["prob"]), flat(d["keep"]), flat(d["axes"]), ranges, got["g_lin"].reshape(B * M, 3, 3),
                            got["g_off"].reshape(B * M, 3))[2].reshape(B, M, 9)
    rl, ro = R.anchor_transforms(d["prob"], d["keep"], d["axes"], ranges)
    z, mu, r, kfar, out = R.deform(d["x"], d["anchors"], rl, ro, d["kernel_axes"], mask, sigma)
    g_lin, g_off, g_mask = R.deform_grad(d["x"], d["anchors"], d["kernel_axes"], mask, sigma, z, mu, r, kfar, d["gout"])
    rg = R.anchor_transforms_grad(d["prob"], d["keep"], d["axes"], ranges, g_lin, g_off)
    label = "fixture-" + k.rstrip("_")
    assert np.array_equal(got["kfar"], kfar) and (expect_kfar is None or int(kfar[0]) == expect_kfar)
    within("z", got["z"], z, label), within("out", got["out"], out, label)
    within("g_lin", got["g_lin"], g_lin, label), within("g_off", got["g_off"], g_off, label)
    within("g_mask", got["g_mask"], g_mask, label), within("g_prob", g_prob, rg, label)
    # and the reference's recorded float64 results lie within the same bars but for pi (2.8e-8 of an angle) -- the
    # restatement with the double pi reproduces them to 1e-12 (tests/test_augment_cases_cpu.py); print the distance only
    print(f"{label}: |kernel - reference's out| max {float(np.abs(got['out'] - gold[k + 'out']).max()):.3e}")


@pytest.mark.parametrize("i", range(6))
def test_fixture_geometry_through_all_four_kernels(dev, gold, i):
    _chain(dev, gold, f"g{i}_")


# ---- invariants ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("row", [C.DEFORM_TABLE[i] for i in (2, 7, 9)], ids=[C.DEFORM_IDS[i] for i in (2, 7, 9)])
def test_a_batch_equals_its_clouds_and_two_runs_agree(dev, row):
    c = C.deform_case(row)
    run = lambda sl: deform_raw(dev, c["x"][sl], c["anchors"][sl], c["lin"][sl], c["off"][sl], c["axes"][sl],
                                None if c["mask"] is None else c["mask"][sl], c["sigma"], c["gout"][sl])
    whole, again = run(slice(None)), run(slice(None))
    for k in whole:
        assert np.array_equal(whole[k].view(np.uint32) if whole[k].dtype == np.float32 else whole[k],
                              again[k].view(np.uint32) if again[k].dtype == np.float32 else again[k]), k
    for b in range(row[2]):
        one = run(slice(b, b + 1))
        for k in whole:
            assert np.array_equal(np.ascontiguousarray(whole[k][b:b + 1]).view(np.uint32 if whole[k].dtype == np.float32 else np.int64),
                                  one[k].view(np.uint32 if one[k].dtype == np.float32 else np.int64)), (k, b)


def test_zz_report_the_worst_ratios():
    """A reporter, not a check of its own: prints, for a whole-file run in file order, the largest error / bar per tensor
    (the header's figures).  `within()` has already asserted every element; run alone, under -k or distributed, this
    finds WORST empty or partial and says nothing.  When the whole file did run, all ten tensors must have been seen."""
    if len(WORST) >= 10:
        assert set(WORST) == {"lin", "off", "g_prob", "z", "mu", "r", "out", "g_lin", "g_off", "g_mask"}
    for name, (ratio, label) in sorted(WORST.items()):
        print(f"worst error / bar  {name:7s} {ratio:.3f}  ({label})")
    assert all(v[0] <= 1.0 for v in WORST.values())
