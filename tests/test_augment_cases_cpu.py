"""CPU suite for the checks of csrc/augment.hip: the float64 restatement (tests/augment_reference.py) and the package's
composed forms against the fixture made from the reference's own methods (tests/golden/augment_golden.npz), the exact
cases' claimed values, and the conditions every random case of tests/test_gpu_augment_cases.py must meet."""
import math
import os

import numpy as np
import pytest
import torch

import augment_cases as C
import augment_reference as R

TOL = 1e-12
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "augment_golden.npz")
N_GEOMETRY = 6


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


def close(got, want, what):
    err = float(np.abs(np.asarray(got) - want).max())
    assert err <= TOL * max(1.0, float(np.abs(want).max())), (what, err)


def geometry_inputs(gold, k):
    """-> the arrays of case k ('g0_' .. or 'tie_') by short name; ranges and sigma as Python numbers."""
    names = ("x", "anchors", "prob", "keep", "axes", "kernel_axes", "gout")
    d = {n: gold[k + n] for n in names}
    d["mask"] = gold[k + "mask"] if k + "mask" in gold.files else np.ones(d["x"].shape[:2])
    d["ranges"] = tuple(float(v) for v in gold[k + "ranges"]) if k + "ranges" in gold.files else C.RANGES["project"]
    d["sigma"] = float(gold[k + "sigma"].reshape(-1)[0]) if k + "sigma" in gold.files else 0.5
    return d


def restate(d, pi):
    lin, off = R.anchor_transforms(d["prob"], d["keep"], d["axes"], d["ranges"], pi=pi)
    z, mu, r, kfar, out = R.deform(d["x"], d["anchors"], lin, off, d["kernel_axes"], d["mask"], d["sigma"])
    g_lin, g_off, g_mask = R.deform_grad(d["x"], d["anchors"], d["kernel_axes"], d["mask"], d["sigma"], z, mu, r, kfar, d["gout"])
    g_prob = R.anchor_transforms_grad(d["prob"], d["keep"], d["axes"], d["ranges"], g_lin, g_off, pi=pi)
    return dict(z=z, mu=mu, r=r, kfar=kfar, out=out, g_prob=g_prob, g_mask=g_mask)


@pytest.mark.parametrize("name", ["project", "wide"])
def test_restatement_reproduces_the_transform_fixture(gold, name):
    k, ranges = f"t_{name}_", C.RANGES[name]
    prob, keep, axes = gold[k + "prob"], gold[k + "keep"], gold[k + "axes"]
    lin, off = R.anchor_transforms(prob, keep, axes, ranges, pi=math.pi)
    g = R.anchor_transforms_grad(prob, keep, axes, ranges, gold[k + "g_lin"], gold[k + "g_off"], pi=math.pi)
    close(lin.v, gold[k + "lin"], "lin"), close(off.v, gold[k + "off"], "off"), close(g.v, gold[k + "g_prob"], "g_prob")
    combos = {(tuple(a), tuple(b)) for a, b in zip(keep.reshape(-1, 3), axes.reshape(-1, 3))}
    assert len(combos) == 56 and prob.shape[0] * prob.shape[1] == 512
    assert np.array_equal(C.f32(prob), prob)                                    # float32 values: a kernel reads them exactly


@pytest.mark.parametrize("k", [f"g{i}_" for i in range(N_GEOMETRY)] + ["tie_"])
def test_restatement_reproduces_the_geometry_fixture(gold, k):
    d = geometry_inputs(gold, k)
    got = restate(d, math.pi)
    for n in ("z", "out", "g_prob") + (("g_mask",) if k != "tie_" else ()):
        close(got[n].v, gold[k + n], k + n)
    for n in ("x", "anchors", "prob", "gout", "mask"):
        assert np.array_equal(C.f32(d[n]), d[n]), n


def _noise(d):
    from adaptpoint_amd.augmentor import Noise
    return Noise(keep=torch.from_numpy(d["keep"]), axes=torch.from_numpy(d["axes"]).int(),
                 kernel_axes=torch.from_numpy(d["kernel_axes"]).int().unsqueeze(1))


@pytest.mark.parametrize("name", ["project", "wide"])
def test_composed_transforms_reproduce_the_fixture(gold, name):
    from adaptpoint_amd.augmentor import anchor_transforms_composed
    k, ranges = f"t_{name}_", C.RANGES[name]
    d = dict(keep=gold[k + "keep"], axes=gold[k + "axes"], kernel_axes=np.ones((64, 3)))
    p = torch.from_numpy(gold[k + "prob"]).requires_grad_(True)
    lin, off = anchor_transforms_composed(p, _noise(d), *ranges)
    ((lin * torch.from_numpy(gold[k + "g_lin"])).sum() + (off * torch.from_numpy(gold[k + "g_off"])).sum()).backward()
    close(lin.detach().numpy(), gold[k + "lin"], "lin"), close(off.detach().numpy(), gold[k + "off"], "off")
    close(p.grad.numpy(), gold[k + "g_prob"], "g_prob")


@pytest.mark.parametrize("k", [f"g{i}_" for i in range(N_GEOMETRY)] + ["tie_"])
def test_composed_geometry_reproduces_the_fixture(gold, k):
    """anchor_transforms_composed + deform_normalise_mask(fused=False) in float64, gradients included.  The tie cloud
    decides the rule at the farthest point: `unit_sphere` must send the radius gradient to the first of the equal points
    (`.max(dim=-1)[0]`, the reference's), not split it (`amax`)."""
    from adaptpoint_amd.augmentor import anchor_transforms_composed, deform_normalise_mask
    d = geometry_inputs(gold, k)
    p = torch.from_numpy(d["prob"]).requires_grad_(True)
    mk = torch.from_numpy(d["mask"]).requires_grad_(True)
    noise = _noise(d)
    lin, off = anchor_transforms_composed(p, noise, *d["ranges"])
    out = deform_normalise_mask(torch.from_numpy(d["x"]), torch.from_numpy(d["anchors"]), lin, off, noise.kernel_axes, mk,
                                d["sigma"], fused=False)
    (out * torch.from_numpy(d["gout"])).sum().backward()
    close(out.detach().numpy(), gold[k + "out"], k + "out")
    close(p.grad.numpy(), gold[k + "g_prob"], k + "g_prob")
    if k != "tie_":
        close(mk.grad.numpy(), gold[k + "g_mask"], k + "g_mask")


def test_the_tie_cloud_decides_the_rule(gold):
    """Two points at exactly the largest radius, in float64 and float32; the even split moves prob's gradient by more
    than 100 bars, so a kernel or mirror following the other rule cannot pass."""
    d = geometry_inputs(gold, "tie_")
    low = restate(d, R.PI32)
    rad = R.centred_radii(low["z"].v, low["mu"].v)
    assert rad[0, 5] == rad[0, 40] == rad.max() == 8.0 and int(low["kfar"][0]) == 5
    lin, off = R.anchor_transforms(d["prob"], d["keep"], d["axes"], d["ranges"])
    g_lin, g_off, _ = R.deform_grad(d["x"], d["anchors"], d["kernel_axes"], d["mask"], d["sigma"], low["z"], low["mu"],
                                    low["r"], low["kfar"], d["gout"], tie_rule="split")
    split = R.anchor_transforms_grad(d["prob"], d["keep"], d["axes"], d["ranges"], g_lin, g_off)
    assert float((np.abs(split.v - low["g_prob"].v) / np.maximum(low["g_prob"].e, 1e-300)).max()) > 100.0


# ---- the conditions on the random cases ----------------------------------------------------------------------------------

def check_conditions(x, anchors, lin, off, axes, mask, draw, sigma, exempt_gap=False):
    z, mu, r, kfar, out = R.deform(x, anchors, lin, off, axes, mask, sigma)
    rad = np.sort(R.centred_radii(z.v, mu.v), axis=1)
    if not exempt_gap:
        assert np.all(rad[:, -1] - rad[:, -2] >= C.GAP * rad[:, -1]), "condition 1"
        assert np.all(2 * r.e < rad[:, -1] - rad[:, -2]), "twice the bar on any radius is below the gap: float32 picks the same point"
    if draw is not None:
        assert float(np.abs(draw - 0.8).min()) >= C.MASK_CLEAR and np.array_equal(mask, (draw < 0.8).astype(np.float64)), "condition 2"
    assert R.weight_sum_min(x, anchors, axes, sigma) >= C.WSUM_MIN, "condition 3"
    assert float(np.linalg.norm(out.v, axis=-1).max()) < 1.0


@pytest.mark.parametrize("row", C.DEFORM_TABLE, ids=C.DEFORM_IDS)
def test_conditions_on_the_random_deformation_cases(row):
    c = C.deform_case(row)
    check_conditions(c["x"], c["anchors"], c["lin"], c["off"], c["axes"], c["mask"], c["mask_draw"], c["sigma"],
                     exempt_gap=row[0] == 2)
    for n in ("x", "anchors", "lin", "off", "gout"):
        assert np.array_equal(C.f32(c[n]), c[n]), n


def test_the_table_crosses_every_size_the_kernels_branch_on():
    rows = C.DEFORM_TABLE
    assert {r[0] for r in rows} == {2, 63, 64, 65, 255, 256, 257, 777, 4095, 4096}
    assert {r[1] for r in rows} == {1, 2, 3, 4, 8} and {r[2] for r in rows} == {1, 3} and {r[3] for r in rows} == {0.5, 0.2}
    assert {c for r in rows for c in r[4]} == set(range(1, 8)) and {r[5] for r in rows} == {"hard", "soft", "none"}
    assert all(len(r[4]) == r[2] for r in rows)


@pytest.mark.parametrize("i", range(N_GEOMETRY))
def test_conditions_on_the_fixture_cases(gold, i):
    d = geometry_inputs(gold, f"g{i}_")
    lin, off = R.anchor_transforms(d["prob"], d["keep"], d["axes"], d["ranges"])
    draw = gold[f"g{i}_mask_draw"] if f"g{i}_mask_draw" in gold.files else None
    check_conditions(d["x"], d["anchors"], lin, off, d["kernel_axes"], d["mask"], draw, d["sigma"])


def test_the_wide_fixture_tells_the_centre_entry_apart(gold):
    """Condition 4: at w_R_range = 180 an anchor with its rotation on has cz cy and cz cx more than 0.1 apart, so the
    reference's centre entry sz sy sx + cz cy is told from the textbook's sz sy sx + cz cx."""
    prob, keep = gold["t_wide_prob"], gold["t_wide_keep"]
    ang = R.PI32 * (np.tanh(prob[..., :3]) * 180.0) / 180.0 * keep[..., :1]
    cx, cy, cz = (np.cos(ang[..., i]) for i in range(3))
    assert float(np.abs(cz * cy - cz * cx).max()) > 0.1


# ---- the exact cases, evaluated by the restatement ------------------------------------------------------------------------

def test_exact_transform_cases_have_the_values_claimed():
    keep, axes = C.switch_table()
    lin, off = R.anchor_transforms(np.zeros((64, 9)), keep, axes, C.RANGES["project"])           # T1
    s = 1.0 + keep[:, 1:2] * axes                                                               # 2 where on, else 1
    assert np.array_equal(lin.v, s[:, None, :] * np.eye(3)) and np.all(off.v == 0) and np.all(off.e == 0)
    rng = np.random.default_rng(3)
    prob = C.f32(2.0 * rng.normal(size=(64, 9)))                                                # T2
    lin, off = R.anchor_transforms(prob, keep, axes, C.RANGES["project"])
    g = R.anchor_transforms_grad(prob, keep, axes, C.RANGES["project"], rng.normal(size=(64, 3, 3)), rng.normal(size=(64, 3)))
    no_rot = keep[:, 0] == 0
    scale_off = (keep[:, 1:2] * axes) == 0
    shift_off = (keep[:, 2:3] * axes) == 0
    sc = np.linalg.norm(lin.v, axis=1)                                                          # column norms: s (R's columns
    assert np.all(lin.v[no_rot] == lin.v[no_rot] * np.eye(3))                                   # ... are not unit: centre entry)
    assert np.all(sc[no_rot][scale_off[no_rot]] == 1.0)
    for arr in (g.v, g.e):
        assert np.all(arr[:, 0:3][no_rot] == 0) and np.all(arr[:, 3:6][scale_off] == 0) and np.all(arr[:, 6:9][shift_off] == 0)
    assert np.all(off.v[shift_off] == 0) and np.all(off.e[shift_off] == 0)
    sign = np.where(rng.integers(0, 2, (64, 9)) == 1, 100.0, -100.0)                           # T3
    r_range, s_range, t_range = C.RANGES["project"]                    # expf(100) overflows float32: sigmoid_ models it
    lin, off = R.anchor_transforms(sign, keep, axes, (r_range, s_range, t_range))
    lin1, _ = R.anchor_transforms(sign, keep, axes, (r_range, 1.0, t_range))                    # s_range = 1: lin is R itself
    g = R.anchor_transforms_grad(sign, keep, axes, (r_range, s_range, t_range), rng.normal(size=(64, 3, 3)), rng.normal(size=(64, 3)))
    assert all(np.isfinite(t.v).all() and np.isfinite(t.e).all() for t in (lin, off, g))
    assert np.array_equal(off.v, np.sign(sign[:, 6:9]) * t_range * keep[:, 2:3] * axes)
    s = np.where((sign[:, 3:6] > 0) & (keep[:, 1:2] * axes == 1), s_range, 1.0)
    assert np.array_equal(lin.v, lin1.v * s[:, None, :]), "s is exactly s_range or 1"
    assert np.all(g.v == 0)


@pytest.mark.parametrize("M", [1, 2, 4, 8])
def test_exact_deformation_case_has_the_values_claimed(M):
    """E1: the restatement gives z, mu, r = 8 and the planted index exactly, and the float32 statement of `out` with its
    single rounding (what the GPU test demands bit for bit) lies within the restatement's bar of its float64 value."""
    c = C.exact_deform(512, M, C.two_ties(), seed=M)
    z, mu, r, kfar, out = R.deform(c["x"], c["anchors"], c["lin"], c["off"], c["axes"], None, 0.5)
    assert np.array_equal(z.v, c["z"]) and np.array_equal(mu.v, c["mu"])
    assert float(r.v[0]) == 8.0 and int(kfar[0]) == 5 and c["rad"][0, 70] == 8.0
    assert np.sort(c["rad"][0])[-3] <= 4.0
    s32 = (np.float32(1.0) / np.float32(8.0)) * np.float32(0.999999)
    out32 = (c["z"].astype(np.float32) - c["mu"].astype(np.float32)[:, None]) * s32
    assert np.all(np.abs(out32.astype(np.float64) - out.v) <= out.e) and np.all(out.e <= 1e-5)


def test_exact_tie_cases():
    """E2: two and three points at the largest radius; the lowest index is taken, and moves with the point."""
    for planted, first in ((C.two_ties(), 5), (C.three_ties(), 5), (C.two_ties(70, 5), 5), (C.three_ties(300, 70, 5), 5)):
        c = C.exact_deform(512, 4, planted, seed=9)
        assert int(c["kfar"][0]) == first and (c["rad"][0] == 8.0).sum() == len([p for p in planted.values() if max(map(abs, p)) == 4.0])
