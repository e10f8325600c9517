"""GPU suite: apn_emd_ratios / apn_emd_match / apn_emd_cost / apn_emd_cost_grad (csrc/emd.hip) through
`adaptpoint_amd.emd` against the numpy statement of their contract (tests/emd_reference.py).

Exact cases, no tolerance (tests/test_emd_cpu.py shows that the float32 statement has them too):
  * an integer lattice and a permutation of it: at level -4^7 every weight between different points underflows to 0 and
    a point's own is exp(0) = 1, so `match` EQUALS the permutation matrix, the cost and both gradients are exactly 0 and
    the later levels add exactly 0;
  * a lattice against the same lattice with every point twice, both ways round: match[l,k] == (d[l,k] == 0), row and
    column sums are exactly the integer-division multipliers;
  * one point on one point: match == 1;
  * cost and gradients from an explicit `match` of small integers over integer coordinates: every partial sum is an
    integer below 2^24 in any order (asserted), so they EQUAL the float64 statement;
  * two runs give the same bits; the tables and the materialised `match` give the same bits; a captured hipGraph of the
    module's forward + backward replays the eager bits and holds no memset node.
The shapes stand on both sides of the iteration's switch-over (emd.EMD_ONE_LAUNCH_MAX = 128: one launch per call up to
it, 20 launches beyond) and of the split kernels' own (four waves per workgroup below 256 points, eight from there on),
off the wave (64) and the row tile (64), past one column chunk (1024), and go up to 300 clouds.

Measured bars on seeded uniform clouds in [-1,1]^3 (the inputs of tests/golden/emd_golden.npz).  The iteration is mildly
ill-conditioned, so the yardstick is computed here, on the same inputs, from the two numpy statements alone:
E32 = max |x32 - x64| for x = match, cost, grad1, grad2.  The kernel must stay within 8 E32 of the float64 statement:
its summation order and the hardware's exp2 differ from both statements by perturbations of the class that separates
the statements from each other, while a bug (a wrong level, a swapped role, a missed tail) shows at 1e-2 and above.
The module's loss and gradients are held to the same bars around the golden, scaled as the module scales them
(cost / n, mean over B: an error of the mean is at most the largest error of a cloud)."""
import gc
import os

import numpy as np
import pytest
import torch

import emd_reference as ER

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = 128                                                   # emd.EMD_ONE_LAUNCH_MAX, asserted below
PERMUTED = [(2, 5, 5), (3, 64, 64), (300, 16, 16), (2, ONE, ONE), (2, ONE + 1, ONE + 1), (1, 513, 513),
            (1, 1100, 1100)]
DOUBLED = [(2, 6, 3), (2, 65, 130), (2, 130, 65), (2, ONE, 64), (2, 2 * ONE + 2, ONE + 1), (1, 257, 514)]
EXPLICIT = [(1, 1, 1), (2, 5, 3), (3, 64, 64), (2, 65, 130), (2, 300, 100), (1, 513, 257), (300, 16, 16), (2, ONE, ONE),
            (2, ONE + 1, ONE), (1, 1100, 1030)]
UNIFORM = [(2, 7, 3), (3, 64, 64), (2, ONE, 100), (2, ONE + 1, 100), (2, 300, 100), (1, 513, 257), (300, 16, 16),
           (1, 1100, 1030)]


@pytest.fixture(scope="module")
def golden_emd():
    return np.load(os.path.join(ROOT, "tests", "golden", "emd_golden.npz"))


def _dev(dev, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def _host(*tensors):
    return [t.cpu().numpy() for t in tensors]


def _everything(dev, xyz1, xyz2, grad_cost=None):
    """tables, match, and cost / gradients from both sources, as numpy arrays."""
    from adaptpoint_amd import emd as E
    assert E.EMD_ONE_LAUNCH_MAX == ONE
    a, b = _dev(dev, xyz1, xyz2)
    assert E.emd_covers(a, b)
    B, n, m = xyz1.shape[0], xyz1.shape[1], xyz2.shape[1]
    g = torch.ones(B, device=dev) if grad_cost is None else _dev(dev, grad_cost)[0]
    ratio_l, ratio_r = E.emd_ratios(a, b)
    assert tuple(ratio_l.shape) == (B, 10, n) and tuple(ratio_r.shape) == (B, 10, m)
    match = E.match_from_ratios(a, b, ratio_l, ratio_r)
    assert tuple(match.shape) == (B, m, n) and match.dtype == torch.float32
    out = {"ratio_l": ratio_l, "ratio_r": ratio_r, "match": match,
           "cost_tab": E.cost(a, b, ratios=(ratio_l, ratio_r)), "cost_mem": E.matchcost_forward(a, b, match)}
    out["g1_tab"], out["g2_tab"] = E.cost_grad(g, a, b, ratios=(ratio_l, ratio_r))
    out["g1_mem"], out["g2_mem"] = E.matchcost_backward(g, a, b, match)
    assert tuple(out["cost_tab"].shape) == (B,) and out["g1_tab"].shape == a.shape and out["g2_tab"].shape == b.shape
    return {k: v.cpu().numpy() for k, v in out.items()}


def _sources_agree(out):
    for key in ("cost", "g1", "g2"):
        assert np.array_equal(out[key + "_tab"].view(np.uint32), out[key + "_mem"].view(np.uint32)), key


@pytest.mark.parametrize("B,n,m", PERMUTED)
def test_permuted_lattice_gives_the_permutation_matrix(dev, B, n, m):
    xyz1 = ER.lattice_cloud(B, n, seed=n * 7 + B)
    xyz2, perm = ER.permuted(xyz1, seed=n * 11 + B)
    out = _everything(dev, xyz1, xyz2)
    assert np.array_equal(out["match"], (perm[:, :, None] == np.arange(n)[None, None, :]).astype(np.float32))
    for key in ("cost_tab", "cost_mem", "g1_tab", "g2_tab", "g1_mem", "g2_mem"):
        assert not out[key].any(), key
    # level 0 moves everything, the later levels find nothing left: the tables are one-hot in the level index
    for table in (out["ratio_l"], out["ratio_r"]):
        assert (table[:, 0] == 1).all() and not table[:, 1:].any()


@pytest.mark.parametrize("B,n,m", DOUBLED)
def test_doubled_lattice_matches_exactly_the_coincident_points(dev, B, n, m):
    small = min(n, m)
    assert max(n, m) == 2 * small
    base = ER.lattice_cloud(B, small, seed=small * 13 + B)
    twice = np.concatenate([base, base], 1)[:, np.random.default_rng(small).permutation(2 * small)]
    xyz1, xyz2 = (twice, base) if n > m else (base, twice)
    out = _everything(dev, xyz1, xyz2)
    assert np.array_equal(out["match"], (ER.dist(xyz1, xyz2, np.float64) == 0).astype(np.float32))
    multi_l, multi_r = ER.multipliers(n, m)
    assert sorted((multi_l, multi_r)) == [1, 2]
    assert (out["match"].sum(1) == multi_l).all() and (out["match"].sum(2) == multi_r).all()
    for key in ("cost_tab", "cost_mem", "g1_tab", "g2_tab", "g1_mem", "g2_mem"):
        assert not out[key].any(), key


def test_one_point_on_one_point(dev):
    xyz = np.full((3, 1, 3), 0.75, np.float32)
    out = _everything(dev, xyz, xyz)
    assert np.array_equal(out["match"], np.ones((3, 1, 1), np.float32)) and not out["cost_tab"].any()


@pytest.mark.parametrize("B,n,m", EXPLICIT)
def test_cost_and_gradients_of_an_explicit_integer_match_equal_the_statement(dev, B, n, m):
    from adaptpoint_amd import emd as E
    rng = np.random.default_rng(n * 131 + m)
    xyz1 = rng.integers(-4, 5, (B, n, 3)).astype(np.float32)
    xyz2 = rng.integers(-4, 5, (B, m, 3)).astype(np.float32)
    keep = rng.random((B, m, n)) < min(1.0, 600.0 / (n * m))        # few enough weights for every sum to stay exact
    match = (rng.integers(1, 4, (B, m, n)) * keep).astype(np.float32)
    grad_cost = rng.choice(np.array([-2, -1, 1, 2, 3], np.float32), B)
    d = ER.dist(xyz1, xyz2, np.float64)
    assert (d * match).sum((1, 2)).max() < 2 ** 24 and match.any()
    step = np.abs(xyz1[:, None, :, :].astype(np.float64) - xyz2[:, :, None, :]) * (2 * match)[..., None]
    assert 3 * max(step.sum(1).max(), step.sum(2).max()) < 2 ** 24
    a, b, mt, g = _dev(dev, xyz1, xyz2, match, grad_cost)
    cost, = _host(E.matchcost_forward(a, b, mt))
    assert np.array_equal(cost.astype(np.float64), ER.cost64(xyz1, xyz2, match))
    grad1, grad2 = _host(*E.matchcost_backward(g, a, b, mt))
    want1, want2 = ER.grad64(grad_cost, xyz1, xyz2, match)
    assert np.array_equal(grad1.astype(np.float64), want1) and np.array_equal(grad2.astype(np.float64), want2)
    assert np.abs(want1).max() > 0 and np.abs(want2).max() > 0


@pytest.mark.parametrize("B,n,m", UNIFORM)
def test_two_runs_and_the_two_sources_give_the_same_bits(dev, B, n, m):
    xyz1, xyz2 = ER.uniform_clouds(B, n, m, seed=n + m)
    grad_cost = np.random.default_rng(n).standard_normal(B).astype(np.float32)
    first = _everything(dev, xyz1, xyz2, grad_cost)
    second = _everything(dev, xyz1, xyz2, grad_cost)
    for key in first:
        assert np.array_equal(first[key].view(np.uint32), second[key].view(np.uint32)), key
    _sources_agree(first)
    assert np.isfinite(first["match"]).all() and (first["match"] >= 0).all() and first["cost_tab"].min() > 0
    assert np.abs(first["g1_tab"]).max() > 0 and np.abs(first["g2_tab"]).max() > 0


@pytest.mark.parametrize("B,n,m", [(2, 7, 3), (3, 100, 70), (2, 300, 130)])
def test_outputs_are_fully_written(dev, B, n, m):
    """Every output and scratch buffer arrives filled with NaN: nothing has to be zeroed, nothing is left unwritten."""
    from adaptpoint_amd.fused import _call
    xyz1, xyz2 = _dev(dev, *ER.uniform_clouds(B, n, m, seed=77))
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=dev)
    ratio_l, ratio_r, state, match = nan(B, 10, n), nan(B, 10, m), nan(B, n + m), nan(B, m, n)
    _call("apn_emd_ratios", dev, B, n, m, xyz1.data_ptr(), xyz2.data_ptr(), ratio_l.data_ptr(), ratio_r.data_ptr(),
          state.data_ptr())
    _call("apn_emd_match", dev, B, n, m, xyz1.data_ptr(), xyz2.data_ptr(), ratio_l.data_ptr(), ratio_r.data_ptr(),
          match.data_ptr())
    assert not torch.isnan(ratio_l).any() and not torch.isnan(ratio_r).any() and not torch.isnan(match).any()
    want = ER.match64(*_host(xyz1, xyz2))
    assert np.abs(match.cpu().numpy() - want).max() < 1e-4
    ones = torch.ones(B, device=dev)
    for source in ((match.data_ptr(), None, None), (None, ratio_l.data_ptr(), ratio_r.data_ptr())):
        part, cost, grad1, grad2 = nan(B, (n + 63) // 64), nan(B), nan(B, n, 3), nan(B, m, 3)
        _call("apn_emd_cost", dev, B, n, m, xyz1.data_ptr(), xyz2.data_ptr(), *source, part.data_ptr(), cost.data_ptr())
        _call("apn_emd_cost_grad", dev, B, n, m, ones.data_ptr(), xyz1.data_ptr(), xyz2.data_ptr(), *source,
              grad1.data_ptr(), grad2.data_ptr())
        for t in (part, cost, grad1, grad2):
            assert not torch.isnan(t).any()


def _bars(xyz1, xyz2, grad_cost):
    """x64 and E32 = max |x32 - x64| for x = match, cost, g1, g2: from the two statements alone."""
    m64, m32 = ER.match64(xyz1, xyz2), ER.match32(xyz1, xyz2)
    x64 = {"match": m64, "cost": ER.cost64(xyz1, xyz2, m64)}
    x32 = {"match": m32, "cost": ER.cost32(xyz1, xyz2, m32)}
    x64["g1"], x64["g2"] = ER.grad64(grad_cost, xyz1, xyz2, m64)
    x32["g1"], x32["g2"] = ER.grad32(grad_cost, xyz1, xyz2, m32)
    e32 = {k: np.abs(x32[k].astype(np.float64) - x64[k]).max() for k in x64}
    assert all(0 < e < 1e-2 for e in e32.values())
    return x64, e32


@pytest.mark.parametrize("name", list(ER.GOLDEN_CASES))
def test_kernels_stay_within_eight_times_the_statements_own_distance(dev, name):
    B, n, m, _ = ER.GOLDEN_CASES[name]
    xyz1, xyz2 = ER.golden_inputs(name)
    grad_cost = np.ones(B, np.float32)
    x64, e32 = _bars(xyz1, xyz2, grad_cost)
    out = _everything(dev, xyz1, xyz2, grad_cost)
    assert np.isfinite(out["match"]).all() and (out["match"] >= 0).all()
    _sources_agree(out)
    got = {"match": out["match"], "cost": out["cost_tab"], "g1": out["g1_tab"], "g2": out["g2_tab"]}
    ratios = {k: np.abs(got[k].astype(np.float64) - x64[k]).max() / e32[k] for k in got}
    print(f"EMD-RATIO {name} {(B, n, m)}: " + ", ".join(f"{k} {ratios[k]:.2f} x E32 = {e32[k]:.2e}" for k in ratios))
    for k in ratios:
        assert ratios[k] <= 8, (k, ratios[k])


@pytest.mark.parametrize("name", list(ER.GOLDEN_CASES))
def test_module_against_the_golden(dev, golden_emd, name):
    from adaptpoint_amd import emd as E
    B, n, m, _ = ER.GOLDEN_CASES[name]
    xyz1, xyz2 = ER.golden_inputs(name)
    scale = np.full(B, 1.0 / (n * B))                           # d loss / d cost (float64: the golden's own factor)
    x64, e32 = _bars(xyz1, xyz2, scale)
    assert abs((x64["cost"] / n).mean() - golden_emd[f"{name}_loss"]) <= 1e-12         # the bars' centre is the golden
    assert np.abs(x64["g1"] - golden_emd[f"{name}_g1"]).max() <= 1e-12
    a, b = (t.requires_grad_(True) for t in _dev(dev, xyz1, xyz2))
    loss = E.earth_mover_distance()(a, b)
    loss.backward()
    off = {"loss": abs(loss.item() - golden_emd[f"{name}_loss"]) / (e32["cost"] / n),
           "g1": np.abs(a.grad.cpu().numpy() - golden_emd[f"{name}_g1"]).max() / e32["g1"],
           "g2": np.abs(b.grad.cpu().numpy() - golden_emd[f"{name}_g2"]).max() / e32["g2"]}
    print(f"EMD-MODULE {name} {(B, n, m)}: " + ", ".join(f"{k} {v:.2f} x E32" for k, v in off.items()))
    for k, v in off.items():
        assert v <= 8, (k, v)


@pytest.mark.parametrize("B,n,m", [(4, 100, 100), (2, 200, 150)])
def test_replay_from_a_hipgraph_equals_eager_without_a_memset_node(dev, B, n, m):
    from adaptpoint_amd import emd as E, graphs
    xyz1, xyz2 = ER.uniform_clouds(B, n, m, seed=5)
    a, b = (t.requires_grad_(True) for t in _dev(dev, xyz1, xyz2))
    loss = E.earth_mover_distance()

    def step():
        value = loss(a, b)
        return [value, *torch.autograd.grad(value, [a, b])]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                       # warm-up: allocator pools, lazy initialisation
        step()
    torch.cuda.current_stream().wait_stream(side)
    eager = [t.detach().clone() for t in step()]
    torch.cuda.synchronize()
    gc.collect()
    graph, captured, census = graphs.capture(step, leaves=[a, b], what="the EMD loss's graph")
    print(f"earth_mover_distance forward + backward at {(B, n, m)}:", census)
    assert not census.get("memset", 0) and census.get("kernel", 0) >= 4
    for _ in range(2):
        for t in captured:
            t.detach().zero_()
        graph.replay()
        torch.cuda.synchronize()
        for x, y in zip(eager, captured):
            assert torch.equal(x, y.detach())
