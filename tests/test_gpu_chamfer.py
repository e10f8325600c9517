"""GPU suite: apn_chamfer_forward / apn_chamfer_backward (csrc/chamfer.hip) through `adaptpoint_amd.chamfer_dist` against
the numpy statement of their contract (tests/chamfer_reference.py).

Exact forward: integer coordinates in [-4, 4] -- every squared distance is an integer <= 192, exact in fp32, and ties are
plentiful -- so distances and indices (the smallest index among equally near points) must EQUAL `nearest64`.  The shapes
take both paths (max(n, m) <= 64: one wave per cloud and direction; beyond: 256-source tiles, targets in chunks of 1024),
sizes that are no multiple of the wave, the tile or the chunk, more than one tile and chunk, and a batch beyond 65535.

Error bars on seeded normal inputs: tau = 6 x 2^-24, the derivation of tests/test_gpu_knn.py at C = 3.  With d64 the
float64 distance to the RETURNED index: |dist - d64| <= tau d64, and d64 <= Dmin (1 + 3 tau).

Gradient: with the indices of `nearest64` and seeded normal clouds and grad_dist, `backward` must EQUAL `backward32`, the
ordered float32 statement, bit for bit.

Modules: on the inputs of tests/golden/chamfer_golden.npz (what the reference's own classes gave over the float64
statement) the indices are the golden's, the losses lie within (n + 8) 2^-24 relative -- 6 for the distance, 2 for the
root and the scaling, the rest for a sum of non-negative terms in any order; n: the smaller cloud -- and the gradients
within (T + 10) 2^-24 sum |term|: backward32's bar plus 8 for the coefficient's rounding through 1 / (2 sqrt d), the
mean and the halving."""
import gc
import os

import numpy as np
import pytest
import torch

import chamfer_reference as CR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -24
EXACT = [(1, 1, 1), (2, 5, 3), (3, 32, 32), (2, 64, 64), (2, 65, 63), (1, 130, 33), (2, 33, 700), (2, 513, 511),
         (1, 1025, 2048), (300, 32, 32), (70000, 4, 4)]
GRADIENT = [(2, 32, 32), (3, 64, 17), (2, 130, 33), (2, 700, 513), (70000, 4, 4)]


@pytest.fixture(scope="module")
def golden_chamfer():
    return np.load(os.path.join(ROOT, "tests", "golden", "chamfer_golden.npz"))


def _forward(dev, xyz1, xyz2):
    from adaptpoint_amd import chamfer_dist as CD
    a, b = torch.from_numpy(xyz1).to(dev), torch.from_numpy(xyz2).to(dev)
    assert CD.chamfer_covers(a, b)
    out = CD.forward(a, b)
    B, n, m = xyz1.shape[0], xyz1.shape[1], xyz2.shape[1]
    assert [tuple(t.shape) for t in out] == [(B, n), (B, m), (B, n), (B, m)]
    assert [t.dtype for t in out] == [torch.float32, torch.float32, torch.int32, torch.int32]
    return tuple(t.cpu().numpy() for t in out)


def _backward(dev, xyz1, xyz2, idx1, idx2, g1, g2):
    from adaptpoint_amd import chamfer_dist as CD
    args = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (xyz1, xyz2, idx1, idx2, g1, g2)]
    gx1, gx2 = CD.backward(*args)
    assert gx1.shape == xyz1.shape and gx2.shape == xyz2.shape and gx1.dtype == gx2.dtype == torch.float32
    return gx1.cpu().numpy(), gx2.cpu().numpy()


@pytest.mark.parametrize("B,n,m", EXACT)
def test_exact_cases_equal_the_reference(dev, B, n, m):
    xyz1 = CR.integer_cloud((B, n, 3), seed=n * 131 + m)
    xyz2 = CR.integer_cloud((B, m, 3), seed=m * 137 + n + 1)
    dist1, dist2, idx1, idx2 = _forward(dev, xyz1, xyz2)
    for dist, idx, (ref_d, ref_i) in ((dist1, idx1, CR.nearest64(xyz1, xyz2)), (dist2, idx2, CR.nearest64(xyz2, xyz1))):
        assert np.array_equal(idx, ref_i)
        assert np.array_equal(dist.astype(np.float64), ref_d)


@pytest.mark.parametrize("n,m", [(40, 64), (300, 1030)])
def test_identical_points_give_index_zero_and_distance_zero(dev, n, m):
    xyz1, xyz2 = np.full((2, n, 3), 2.5, np.float32), np.full((2, m, 3), 2.5, np.float32)
    for out in _forward(dev, xyz1, xyz2):
        assert not out.any()


@pytest.mark.parametrize("n", [50, 300])
def test_distinct_points_find_themselves(dev, n):
    xyz = np.random.default_rng(81).standard_normal((2, n, 3)).astype(np.float32)
    assert len(np.unique(xyz.reshape(-1, 3), axis=0)) == 2 * n
    dist1, dist2, idx1, idx2 = _forward(dev, xyz, xyz)
    own = np.broadcast_to(np.arange(n, dtype=np.int32), (2, n))
    assert np.array_equal(idx1, own) and np.array_equal(idx2, own) and not dist1.any() and not dist2.any()


@pytest.mark.parametrize("B,n,m", [(2, 300, 300), (2, 1000, 70)])
def test_error_bars_on_normal_inputs(dev, B, n, m):
    rng = np.random.default_rng(500 + n)
    xyz1, xyz2 = rng.standard_normal((B, n, 3)).astype(np.float32), rng.standard_normal((B, m, 3)).astype(np.float32)
    dist1, dist2, idx1, idx2 = _forward(dev, xyz1, xyz2)
    for dist, idx, a, b in ((dist1, idx1, xyz1, xyz2), (dist2, idx2, xyz2, xyz1)):
        assert (idx >= 0).all() and (idx < b.shape[1]).all()
        all64 = CR.dist2_64(b, a)                                  # (B, |a|, |b|)
        d64 = np.take_along_axis(all64, idx.astype(np.int64)[..., None], -1)[..., 0]
        dmin = all64.min(-1)
        err = np.abs(dist.astype(np.float64) - d64) / d64
        print(f"({B},{n},{m}): worst |dist - d64| / d64 = {err.max() / EPS:.2f} x 2^-24 (bar 6); worst d64 / Dmin - 1 = "
              f"{(d64 / dmin - 1).max() / EPS:.2f} x 2^-24 (bar 18)")
        assert (np.abs(dist.astype(np.float64) - d64) <= CR.TAU * d64).all()
        assert (d64 <= dmin * (1 + 3 * CR.TAU)).all()


def _gradient_case(B, n, m):
    rng = np.random.default_rng(600 + n + m)
    xyz1, xyz2 = rng.standard_normal((B, n, 3)).astype(np.float32), rng.standard_normal((B, m, 3)).astype(np.float32)
    return xyz1, xyz2, rng.standard_normal((B, n)).astype(np.float32), rng.standard_normal((B, m)).astype(np.float32)


def _all_to_one():
    """(1,300,6): one target at the origin and five beyond 100 -- a list of 300 and five empty lists."""
    rng = np.random.default_rng(611)
    xyz1 = rng.standard_normal((1, 300, 3)).astype(np.float32)
    xyz2 = (rng.standard_normal((1, 6, 3)) + 200).astype(np.float32)
    xyz2[0, 0] = 0
    return xyz1, xyz2, rng.standard_normal((1, 300)).astype(np.float32), rng.standard_normal((1, 6)).astype(np.float32)


@pytest.mark.parametrize("case", GRADIENT + ["all to one"], ids=str)
def test_gradient_equals_the_ordered_float32_statement_bit_for_bit(dev, case):
    xyz1, xyz2, g1, g2 = _all_to_one() if case == "all to one" else _gradient_case(*case)
    _, _, idx1, idx2 = CR.forward64(xyz1, xyz2)
    if case == "all to one":
        assert np.bincount(idx1[0], minlength=6).tolist() == [300, 0, 0, 0, 0, 0]
    got = _backward(dev, xyz1, xyz2, idx1, idx2, g1, g2)
    want = CR.backward32(xyz1, xyz2, idx1, idx2, g1, g2)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("B,n,m", [(3, 40, 33), (2, 300, 257)])
def test_outputs_are_fully_written(dev, B, n, m):
    from adaptpoint_amd.fused import _call
    xyz1, xyz2, g1, g2 = (torch.from_numpy(a).to(dev) for a in _gradient_case(B, n, m))
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=dev)
    dist1, dist2 = nan(B, n), nan(B, m)
    idx1, idx2 = (torch.full((B, k), -7, dtype=torch.int32, device=dev) for k in (n, m))
    _call("apn_chamfer_forward", dev, B, n, m, xyz1.data_ptr(), xyz2.data_ptr(), dist1.data_ptr(), dist2.data_ptr(),
          idx1.data_ptr(), idx2.data_ptr())
    assert not torch.isnan(dist1).any() and not torch.isnan(dist2).any()
    assert (idx1 >= 0).all() and (idx1 < m).all() and (idx2 >= 0).all() and (idx2 < n).all()
    gx1, gx2 = nan(B, n, 3), nan(B, m, 3)
    _call("apn_chamfer_backward", dev, B, n, m, xyz1.data_ptr(), xyz2.data_ptr(), idx1.data_ptr(), idx2.data_ptr(),
          g1.data_ptr(), g2.data_ptr(), gx1.data_ptr(), gx2.data_ptr())
    assert not torch.isnan(gx1).any() and not torch.isnan(gx2).any()


@pytest.mark.parametrize("loss", CR.LOSSES)
@pytest.mark.parametrize("name", list(CR.GOLDEN_CASES))
def test_modules_against_the_golden(dev, golden_chamfer, monkeypatch, name, loss):
    from adaptpoint_amd import chamfer_dist as CD
    xyz1, xyz2, (ignore, keep1, keep2) = CR.golden_inputs(name)
    seen = []
    real = CD.forward
    monkeypatch.setattr(CD, "forward", lambda *a: seen.append(real(*a)) or seen[-1])
    a = torch.from_numpy(xyz1).to(dev).requires_grad_(True)
    b = torch.from_numpy(xyz2).to(dev).requires_grad_(True)
    cls = {"l1": CD.ChamferDistanceL1, "l2": CD.ChamferDistanceL2, "l2_split": CD.ChamferDistanceL2_split}[loss]
    value = cls(ignore_zeros=ignore)(a, b)
    value = torch.stack(list(value)) if isinstance(value, tuple) else value
    value.sum().backward()
    assert len(seen) == 1
    idx1, idx2 = golden_chamfer[f"{name}_idx1"], golden_chamfer[f"{name}_idx2"]
    assert np.array_equal(seen[0][2].cpu().numpy(), idx1) and np.array_equal(seen[0][3].cpu().numpy(), idx2)
    want = golden_chamfer[f"{name}_{loss}"]
    rel = np.abs(value.detach().cpu().numpy().astype(np.float64) - want) / np.abs(want)
    bar = min(len(keep1), len(keep2)) + 8
    print(f"{name} {loss}: loss off by {rel.max() / EPS:.2f} x 2^-24 relative (bar {bar})")
    assert (rel <= bar * EPS).all()
    # the gradient's bar: the terms of the float64 statement with the loss's float64 coefficients
    k1, k2 = xyz1[:, keep1].astype(np.float64), xyz2[:, keep2].astype(np.float64)
    d1, d2, i1, i2 = CR.forward64(k1, k2)
    assert np.array_equal(i1, idx1) and np.array_equal(i2, idx2)
    sides = CR.backward64(k1, k2, i1, i2, *CR.loss_coefficients(loss, d1, d2))
    for got, key, keep, (g64, T, S) in ((a.grad, "g1", keep1, sides[0]), (b.grad, "g2", keep2, sides[1])):
        got = got.cpu().numpy().astype(np.float64)
        want = golden_chamfer[f"{name}_{loss}_{key}"]
        assert np.abs(g64 - want[:, keep]).max() <= 1e-12 * np.abs(want).max()           # the bar's terms are the golden's
        bound = (T + 10) * EPS * S
        err = np.abs(got[:, keep] - want[:, keep])
        print(f"{name} {loss} {key}: worst gradient error = {(err / bound).max():.2f} of (T + 10) 2^-24 sum |term|")
        assert (err <= bound).all()
        dropped = np.setdiff1d(np.arange(want.shape[1]), keep)
        assert not got[:, dropped].any() and not want[:, dropped].any()


def test_two_runs_are_bit_identical(dev):
    for xyz1, xyz2, g1, g2 in (_gradient_case(2, 700, 513), _gradient_case(5, 32, 32), _all_to_one()):
        first = _forward(dev, xyz1, xyz2)
        second = _forward(dev, xyz1, xyz2)
        assert all(np.array_equal(x, y) for x, y in zip(first, second))
        ga = _backward(dev, xyz1, xyz2, first[2], first[3], g1, g2)
        gb = _backward(dev, xyz1, xyz2, first[2], first[3], g1, g2)
        assert np.array_equal(ga[0], gb[0]) and np.array_equal(ga[1], gb[1])


@pytest.mark.parametrize("B,n,m", [(4, 256, 256), (64, 32, 32)])
def test_replay_from_a_hipgraph_equals_eager_without_a_memset_node(dev, B, n, m):
    from adaptpoint_amd import chamfer_dist as CD, graphs
    xyz1, xyz2, _, _ = _gradient_case(B, n, m)
    a = torch.from_numpy(xyz1).to(dev).requires_grad_(True)
    b = torch.from_numpy(xyz2).to(dev).requires_grad_(True)
    loss = CD.ChamferDistanceL1()

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
    graph, captured, census = graphs.capture(step, leaves=[a, b], what="the Chamfer loss's graph")
    print(f"Chamfer L1 forward + backward at {(B, n, m)}:", census)
    assert not census.get("memset", 0) and census.get("kernel", 0) >= 2
    for _ in range(2):
        for t in captured:
            t.detach().zero_()
        graph.replay()
        torch.cuda.synchronize()
        for x, y in zip(eager, captured):
            assert torch.equal(x, y.detach())
