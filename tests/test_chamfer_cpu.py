"""CPU suite: `adaptpoint_amd.chamfer_dist` without a GPU.

  * the modules' glue (ChamferFunction's save / restore, the three losses' arithmetic, the `ignore_zeros` row filter) run
    on CPU with `chamfer_dist.forward` / `backward` replaced by the float64 statement (tests/chamfer_reference.py) must
    reproduce what the reference's own classes gave over the same statement (tests/golden/chamfer_golden.npz).  Both
    sides are float64 results of the same formulae; the bar is one float32 rounding, 2^-24 relative (of the largest
    gradient entry for the gradients), far above float64 reassociation and far below any mistake in the arithmetic;
  * `backward32`, the ordered float32 statement the kernel is held to bit for bit, against `backward64`: every element
    within (T + 2) 2^-24 sum |term| -- one rounding in the difference, one in the product, T - 1 in the ordered sum;
  * the argument checks, and `chamfer_covers` agreeing with them."""
import os

import numpy as np
import pytest
import torch

import chamfer_reference as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -24


@pytest.fixture(scope="module")
def golden_chamfer():
    return np.load(os.path.join(ROOT, "tests", "golden", "chamfer_golden.npz"))


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


@pytest.fixture
def statement(monkeypatch):
    """`chamfer_dist.forward` / `backward` backed by the float64 statement, on CPU tensors; records the calls."""
    from adaptpoint_amd import chamfer_dist as CD
    calls = []

    def forward(xyz1, xyz2):
        assert xyz1.is_contiguous() and xyz2.is_contiguous()
        calls.append("forward")
        return tuple(_t(a) for a in CR.forward64(xyz1.numpy(), xyz2.numpy()))

    def backward(xyz1, xyz2, idx1, idx2, grad_dist1, grad_dist2):
        assert grad_dist1.is_contiguous() and grad_dist2.is_contiguous()
        calls.append("backward")
        (g1, _, _), (g2, _, _) = CR.backward64(xyz1.numpy(), xyz2.numpy(), idx1.numpy(), idx2.numpy(),
                                               grad_dist1.numpy(), grad_dist2.numpy())
        return _t(g1), _t(g2)
    monkeypatch.setattr(CD, "forward", forward)
    monkeypatch.setattr(CD, "backward", backward)
    return calls


def _loss(CD, loss, ignore):
    cls = {"l1": CD.ChamferDistanceL1, "l2": CD.ChamferDistanceL2, "l2_split": CD.ChamferDistanceL2_split}[loss]
    return cls(ignore_zeros=ignore)


@pytest.mark.parametrize("loss", CR.LOSSES)
@pytest.mark.parametrize("name", list(CR.GOLDEN_CASES))
def test_module_glue_reproduces_the_reference_classes(golden_chamfer, statement, name, loss):
    from adaptpoint_amd import chamfer_dist as CD
    xyz1, xyz2, (ignore, _, _) = CR.golden_inputs(name)
    a, b = _t(xyz1).double().requires_grad_(True), _t(xyz2).double().requires_grad_(True)
    value = _loss(CD, loss, ignore)(a, b)
    assert isinstance(value, tuple) == (loss == "l2_split")
    value = torch.stack(list(value)) if isinstance(value, tuple) else value
    value.sum().backward()
    assert statement == ["forward", "backward"]
    want = golden_chamfer[f"{name}_{loss}"]
    assert np.abs(value.detach().numpy() - want).max() <= EPS * np.abs(want).max()
    for got, key in ((a.grad, "g1"), (b.grad, "g2")):
        want = golden_chamfer[f"{name}_{loss}_{key}"]
        assert np.isfinite(want).all() and np.abs(want).max() > 0
        assert np.abs(got.numpy() - want).max() <= EPS * np.abs(want).max()
    if ignore:                                                # the filtered rows take no gradient
        B, n, m, _, _, zero1, zero2 = CR.GOLDEN_CASES[name]
        assert not a.grad.numpy()[:, list(zero1)].any() and not b.grad.numpy()[:, list(zero2)].any()


def test_function_makes_its_inputs_contiguous_and_is_once_differentiable(statement):
    from adaptpoint_amd import chamfer_dist as CD
    xyz1, xyz2, _ = CR.golden_inputs("patches")
    a = _t(xyz1).double().transpose(1, 2).contiguous().transpose(1, 2).requires_grad_(True)     # (B,n,3), strided
    assert not a.is_contiguous()
    b = _t(xyz2).double().requires_grad_(True)
    d1, d2 = CD.ChamferFunction.apply(a, b)                   # the statement asserts contiguity
    w = torch.ones_like(d1, requires_grad=True)               # a differentiable grad_dist1: a second derivative is asked for
    ga, = torch.autograd.grad((d1 * w).sum() + d2.sum(), a, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        ga.sum().backward()


def _all_to_one(seed):
    """Every point of xyz1 chooses target 0 of xyz2 (at the origin; the others lie beyond 100): one list of n, m - 1 empty."""
    rng = np.random.default_rng(seed)
    xyz1 = rng.standard_normal((1, 300, 3)).astype(np.float32)
    xyz2 = (rng.standard_normal((1, 6, 3)) + 200).astype(np.float32)
    xyz2[0, 0] = 0
    return xyz1, xyz2


def statement_cases():
    """(xyz1, xyz2, grad_dist1, grad_dist2): 18 seeded cases, the all-to-one case among them."""
    cases = []
    for k, (B, n, m) in enumerate([(2, 32, 32), (3, 64, 17), (2, 130, 33), (1, 40, 200), (1, 1, 50), (2, 50, 1), (4, 8, 8),
                                   (1, 257, 129)] * 2):
        rng = np.random.default_rng(7000 + k)
        cases.append((rng.standard_normal((B, n, 3)).astype(np.float32), rng.standard_normal((B, m, 3)).astype(np.float32)))
    cases += [_all_to_one(7100), _all_to_one(7101)]
    out = []
    for k, (xyz1, xyz2) in enumerate(cases):
        rng = np.random.default_rng(7200 + k)
        out.append((xyz1, xyz2, rng.standard_normal(xyz1.shape[:2]).astype(np.float32),
                    rng.standard_normal(xyz2.shape[:2]).astype(np.float32)))
    return out


def test_ordered_float32_statement_is_within_its_derived_bound_of_float64():
    worst = 0.0
    cases = statement_cases()
    assert len(cases) == 18
    for xyz1, xyz2, g1, g2 in cases:
        _, _, idx1, idx2 = CR.forward64(xyz1, xyz2)
        got = CR.backward32(xyz1, xyz2, idx1, idx2, g1, g2)
        ref = CR.backward64(xyz1, xyz2, idx1, idx2, g1, g2)
        for g32, (g64, T, S) in zip(got, ref):
            assert g32.dtype == np.float32 and (T >= 1).all()
            bound = (T + 2) * EPS * S
            assert (np.abs(g32.astype(np.float64) - g64) <= bound).all()
            worst = max(worst, (np.abs(g32.astype(np.float64) - g64) / bound).max())
    xyz1, xyz2, g1, g2 = cases[-1]
    _, _, idx1, idx2 = CR.forward64(xyz1, xyz2)
    assert not idx1.any() and CR.backward64(xyz1, xyz2, idx1, idx2, g1, g2)[1][1][0, 0, 0] == 301    # the list of 300 + 1
    print(f"backward32 against backward64: worst error = {worst:.2f} of the bound (T + 2) 2^-24 sum |term|")


def test_batched_form_of_the_statement_equals_the_scalar_form():
    """tests/chamfer_reference.py evaluates many small clouds with array operations: the same bits as the scalars."""
    rng = np.random.default_rng(7300)
    xyz1, xyz2 = rng.standard_normal((70, 5, 3)).astype(np.float32), rng.standard_normal((70, 4, 3)).astype(np.float32)
    g1, g2 = rng.standard_normal((70, 5)).astype(np.float32), rng.standard_normal((70, 4)).astype(np.float32)
    _, _, idx1, idx2 = CR.forward64(xyz1, xyz2)
    many = CR.backward32(xyz1, xyz2, idx1, idx2, g1, g2)
    for lo in (0, 35):
        s = slice(lo, lo + 35)
        few = CR.backward32(xyz1[s], xyz2[s], idx1[s], idx2[s], g1[s], g2[s])
        assert np.array_equal(many[0][s], few[0]) and np.array_equal(many[1][s], few[1])


def test_nearest64_takes_the_first_minimum():
    a = np.zeros((1, 2, 3), np.float32)
    b = np.array([[[1, 0, 0], [0, 1, 0], [0, 0, -1], [2, 0, 0]]], np.float32)
    d, i = CR.nearest64(a, b)
    assert np.array_equal(i, [[0, 0]]) and np.array_equal(d, [[1, 1]])
    d, i = CR.nearest64(b, a)
    assert np.array_equal(i, [[0, 0, 0, 0]]) and np.array_equal(d, [[1, 1, 1, 4]])


def test_argument_checks_raise_the_house_errors_and_covers_agrees():
    from adaptpoint_amd import chamfer_dist as CD
    f32 = lambda *shape: torch.zeros(*shape, dtype=torch.float32)
    a, b = f32(2, 8, 3), f32(2, 5, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        CD.forward(a, b)
    with pytest.raises(RuntimeError, match="no CPU path"):
        CD.backward(a, b, torch.zeros(2, 8, dtype=torch.int32), torch.zeros(2, 5, dtype=torch.int32), f32(2, 8), f32(2, 5))
    with pytest.raises(RuntimeError, match="float32"):
        CD.forward(a.double(), b.double())
    with pytest.raises(RuntimeError, match="float32"):
        CD.forward(a, b.double())
    with pytest.raises(RuntimeError, match="int32"):
        CD.backward(a, b, torch.zeros(2, 8, dtype=torch.int64), torch.zeros(2, 5, dtype=torch.int32), f32(2, 8), f32(2, 5))
    with pytest.raises(RuntimeError, match="batch sizes differ"):
        CD.forward(a, f32(3, 5, 3))
    with pytest.raises(RuntimeError, match=r"\(B,n,3\)"):
        CD.forward(a, f32(2, 5, 4))
    big = torch.empty(1, CD.CHAMFER_MAX_POINTS + 1, 3, dtype=torch.float32)
    with pytest.raises(RuntimeError, match="CHAMFER_MAX_POINTS"):
        CD.forward(big, f32(1, 5, 3))
    with pytest.raises(RuntimeError, match="CHAMFER_MAX_POINTS"):
        CD.forward(f32(1, 5, 3), big)
    with pytest.raises(RuntimeError, match="CHAMFER_MAX_POINTS"):
        CD.forward(f32(1, 0, 3), f32(1, 5, 3))
    with pytest.raises(RuntimeError, match="2\\^24"):
        CD.forward(torch.empty(2 ** 22, 4, 3, device="meta"), torch.empty(2 ** 22, 4, 3, device="meta"))
    for x, y in ((a, b), (a.double(), b.double()), (a, f32(3, 5, 3)), (big, f32(1, 5, 3)), (f32(1, 5, 3), big), (a, f32(2, 5, 4))):
        assert CD.chamfer_covers(x, y) is False
    # on a device the same limits decide alone: meta tensors have shapes and dtypes but claim no device memory
    assert CD._shape_problem(torch.empty(1, CD.CHAMFER_MAX_POINTS, 3, device="meta"), torch.empty(1, 1, 3, device="meta")) is None
    assert CD._shape_problem(torch.empty(255, 65536, 3, device="meta"), torch.empty(255, 1, 3, device="meta")) is None
    assert CD._shape_problem(torch.empty(256, 65536, 3, device="meta"), torch.empty(256, 1, 3, device="meta")) is not None


def test_library_declares_both_entries_and_agrees_on_the_limits():
    from adaptpoint_amd import _lib, chamfer_dist as CD
    assert {"apn_chamfer_forward", "apn_chamfer_backward", "apn_chamfer_max_points"} <= set(_lib.SIGNATURES)
    lib = _lib.load()
    assert lib.apn_chamfer_max_points() == CD.CHAMFER_MAX_POINTS >= 16384
    EINVAL, P = -1, 4096                                      # P: a non-null address that is never read

    def fwd(b=2, n=8, m=5, xyz1=P, xyz2=P, dist1=P, dist2=P, idx1=P, idx2=P):
        return lib.apn_chamfer_forward(b, n, m, xyz1, xyz2, dist1, dist2, idx1, idx2, None)

    def bwd(b=2, n=8, m=5, xyz1=P, xyz2=P, idx1=P, idx2=P, grad_dist1=P, grad_dist2=P, grad_xyz1=P, grad_xyz2=P):
        return lib.apn_chamfer_backward(b, n, m, xyz1, xyz2, idx1, idx2, grad_dist1, grad_dist2, grad_xyz1, grad_xyz2, None)
    for entry, names in ((fwd, ("xyz1", "xyz2", "dist1", "dist2", "idx1", "idx2")),
                         (bwd, ("xyz1", "xyz2", "idx1", "idx2", "grad_dist1", "grad_dist2", "grad_xyz1", "grad_xyz2"))):
        assert entry(b=-1) == EINVAL and entry(n=0) == EINVAL and entry(m=0) == EINVAL and entry(n=-3) == EINVAL
        assert entry(n=CD.CHAMFER_MAX_POINTS + 1) == EINVAL and entry(m=CD.CHAMFER_MAX_POINTS + 1) == EINVAL
        assert entry(b=2 ** 22, n=4, m=4) == EINVAL and entry(b=256, n=65536, m=1) == EINVAL       # b max(n, m) = 2^24
        assert entry(b=0, **{k: None for k in names}) == 0                                          # no clouds: a no-op
        for k in names:
            assert entry(**{k: None}) == EINVAL, (entry.__name__, k)
