"""CPU suite: `adaptpoint_amd.emd` without a GPU.

  * the float64 statement (tests/emd_reference.py) reproduces the hand-worked case of the reference's test_emd_loss.py
    (two points each, which match crosswise), and the reference's quirks: multipliers by integer division, (B,m,n);
  * the exact cases of tests/test_gpu_emd.py hold for the float32 statement: a permuted integer lattice gives the
    permutation matrix, a duplicated lattice `d == 0`;
  * the glue (EarthMoverDistanceFunction's save / restore, the module's arithmetic, the three extension functions) run on
    CPU with `emd_ratios` / `match_from_ratios` / `cost` / `cost_grad` replaced by the float64 statement must reproduce
    what the reference's own classes gave over the same statement (tests/golden/emd_golden.npz).  Both sides are float64
    results of the same formulae; the bar is one float32 rounding, 2^-24 relative to the largest entry;
  * the argument checks, `emd_covers` agreeing with them, the library's refusals, and `emd_cuda`'s re-exports."""
import os

import numpy as np
import pytest
import torch

import emd_reference as ER

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -24


@pytest.fixture(scope="module")
def golden_emd():
    return np.load(os.path.join(ROOT, "tests", "golden", "emd_golden.npz"))


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


@pytest.fixture
def statement(monkeypatch):
    """The four kernel-backed functions of `adaptpoint_amd.emd` backed by the float64 statement, on CPU tensors."""
    from adaptpoint_amd import emd as E
    calls = []

    def emd_ratios(xyz1, xyz2):
        assert xyz1.is_contiguous() and xyz2.is_contiguous()
        calls.append("ratios")
        return tuple(_t(a) for a in ER.ratios64(xyz1.numpy(), xyz2.numpy()))

    def match_from_ratios(xyz1, xyz2, ratio_l, ratio_r):
        calls.append("match")
        return _t(ER.match64(xyz1.numpy(), xyz2.numpy(), (ratio_l.numpy(), ratio_r.numpy())))

    def source(xyz1, xyz2, match, ratios):
        assert (match is None) != (ratios is None)
        if match is not None:
            return match.numpy()
        return ER.match64(xyz1.numpy(), xyz2.numpy(), tuple(r.numpy() for r in ratios))

    def cost(xyz1, xyz2, match=None, ratios=None):
        calls.append("cost from " + ("match" if ratios is None else "tables"))
        return _t(ER.cost64(xyz1.numpy(), xyz2.numpy(), source(xyz1, xyz2, match, ratios)))

    def cost_grad(grad_cost, xyz1, xyz2, match=None, ratios=None):
        assert grad_cost.is_contiguous()
        calls.append("grad from " + ("match" if ratios is None else "tables"))
        return tuple(_t(g) for g in ER.grad64(grad_cost.numpy(), xyz1.numpy(), xyz2.numpy(), source(xyz1, xyz2, match, ratios)))
    for fn in (emd_ratios, match_from_ratios, cost, cost_grad):
        monkeypatch.setattr(E, fn.__name__, fn)
    return calls


def test_statement_reproduces_the_reference_hand_worked_case():
    """test_emd_loss.py: p1 = {a0, a1}, p2 = {b0, b1} with a0 nearest b1 and a1 nearest b0; the expected cost of a cloud
    is |a0 - b1|^2 + |a1 - b0|^2 and the module divides by n = 2.  The annealing leaves a small residue of mass on the
    far pairs: the reference's own script prints the two numbers side by side without a bar; 1e-3 relative holds."""
    p1 = np.repeat(np.array([[[1.7, -0.1, 0.1], [0.1, 1.2, 0.3]]], np.float32), 3, 0)
    p2 = np.repeat(np.array([[[0.3, 1.8, 0.2], [1.2, -0.2, 0.3]]], np.float32), 3, 0)
    match = ER.match64(p1, p2)
    assert match.shape == (3, 2, 2)
    cross = np.array([[0.0, 1.0], [1.0, 0.0]])                 # match[l,k]: l = 0 takes k = 1
    assert np.abs(match - cross).max() < 1e-3
    want = ((p1[:, 0].astype(np.float64) - p2[:, 1]) ** 2).sum(-1) + ((p1[:, 1].astype(np.float64) - p2[:, 0]) ** 2).sum(-1)
    cost = ER.cost64(p1, p2, match)
    assert np.abs(cost - want).max() <= 1e-3 * want.max()
    # d (sum_b w_b cost_b / 2) with the script's weights: 2 w_b (a_k - b_partner) / 2
    w = np.array([0.5, 2.0, 1 / 3.0])
    g1, g2 = ER.grad64(w / 2, p1, p2, match)
    want1 = w[:, None, None] * (p1.astype(np.float64) - p2[:, ::-1])
    assert np.abs(g1 - want1).max() <= 2e-3 * np.abs(want1).max()
    assert np.abs(g2 + want1[:, ::-1]).max() <= 2e-3 * np.abs(want1).max()


def test_multipliers_are_integer_divisions_and_match_is_b_m_n():
    assert ER.multipliers(7, 3) == (1, 2) and ER.multipliers(3, 7) == (2, 1) and ER.multipliers(5, 5) == (1, 1)
    assert ER.multipliers(300, 100) == (1, 3) and ER.multipliers(65, 130) == (2, 1)
    for n, m in ((7, 3), (3, 7)):
        xyz1, xyz2 = ER.uniform_clouds(2, n, m, 31)
        ratio_l, ratio_r = ER.ratios64(xyz1, xyz2)
        assert ratio_l.shape == (2, 10, n) and ratio_r.shape == (2, 10, m)
        match = ER.match64(xyz1, xyz2, (ratio_l, ratio_r))
        assert match.shape == (2, m, n) and (match >= 0).all()
        multi_l, multi_r = ER.multipliers(n, m)
        # no point gives away more than its multiplier; (7,3): the three points of xyz2 carry 2 each, 6 of 7 units move
        assert (match.sum(1) <= multi_l + 1e-9).all() and (match.sum(2) <= multi_r + 1e-9).all()
        assert np.abs(match.sum((1, 2)) - min(n * multi_l, m * multi_r)).max() < 1e-2


def test_levels_are_the_reference_s():
    assert ER.LEVELS == (-16384.0, -4096.0, -1024.0, -256.0, -64.0, -16.0, -4.0, -1.0, -0.25, 0.0)


@pytest.mark.parametrize("f", ["32", "64"])
def test_exact_cases_hold_for_the_statements(f):
    ratios, match_of = (ER.ratios32, ER.match32) if f == "32" else (ER.ratios64, ER.match64)
    xyz1 = ER.lattice_cloud(2, 40, 5)
    xyz2, perm = ER.permuted(xyz1, 6)
    match = match_of(xyz1, xyz2, ratios(xyz1, xyz2))
    want = (perm[:, :, None] == np.arange(40)[None, None, :])
    if f == "32":
        assert np.array_equal(match, want.astype(np.float32))
    else:
        assert np.abs(match - want).max() < 1e-8                  # 1 / (1 + 1e-9) in float64
    base = ER.lattice_cloud(2, 20, 7)
    twice = np.concatenate([base, base], 1)[:, np.random.default_rng(8).permutation(40)]
    for a, b in ((twice, base), (base, twice)):
        match = match_of(a, b, ratios(a, b))
        zero = ER.dist(a, b, np.float64) == 0
        if f == "32":
            assert np.array_equal(match, zero.astype(np.float32))
        else:
            assert np.abs(match - zero).max() < 1e-8


def test_float32_statement_stays_near_the_float64_statement():
    for name in ER.GOLDEN_CASES:
        xyz1, xyz2 = ER.golden_inputs(name)
        m64, m32 = ER.match64(xyz1, xyz2), ER.match32(xyz1, xyz2)
        assert m32.dtype == np.float32 and (m32 >= 0).all()
        e = np.abs(m32 - m64).max()
        print(f"{name}: E32(match) = {e:.2e}")
        assert e < 1e-4


@pytest.mark.parametrize("name", list(ER.GOLDEN_CASES))
def test_module_glue_reproduces_the_reference_classes(golden_emd, statement, name):
    from adaptpoint_amd import emd as E
    xyz1, xyz2 = ER.golden_inputs(name)
    a, b = _t(xyz1).double().requires_grad_(True), _t(xyz2).double().requires_grad_(True)
    loss = E.earth_mover_distance()(a, b, transpose=True)          # accepted and ignored
    loss.backward()
    assert statement == ["ratios", "cost from tables", "grad from tables"]
    want = golden_emd[f"{name}_loss"]
    assert abs(loss.item() - want) <= EPS * abs(want)
    for got, key in ((a.grad, "g1"), (b.grad, "g2")):
        want = golden_emd[f"{name}_{key}"]
        assert np.isfinite(want).all() and np.abs(want).max() > 0
        assert np.abs(got.numpy() - want).max() <= EPS * np.abs(want).max()


def test_extension_functions_compose_like_the_reference_function(golden_emd, statement):
    """approxmatch_forward + matchcost_forward + matchcost_backward, as the reference's Function chains them."""
    from adaptpoint_amd import emd as E
    import emd_cuda
    assert emd_cuda.approxmatch_forward is E.approxmatch_forward and emd_cuda.matchcost_forward is E.matchcost_forward
    assert emd_cuda.matchcost_backward is E.matchcost_backward
    assert emd_cuda.__all__ == ["approxmatch_forward", "matchcost_forward", "matchcost_backward"]
    name = "tiny"
    B, n, m, _ = ER.GOLDEN_CASES[name]
    xyz1, xyz2 = (_t(x).double() for x in ER.golden_inputs(name))
    match = emd_cuda.approxmatch_forward(xyz1, xyz2)
    assert tuple(match.shape) == (B, m, n)
    cost = emd_cuda.matchcost_forward(xyz1, xyz2, match)
    assert tuple(cost.shape) == (B,)
    grad1, grad2 = emd_cuda.matchcost_backward(torch.full((B,), 1.0 / (n * B), dtype=torch.float64), xyz1, xyz2, match)
    assert statement == ["ratios", "match", "cost from match", "grad from match"]
    assert abs((cost / n).mean().item() - golden_emd[f"{name}_loss"]) <= EPS * golden_emd[f"{name}_loss"]
    for got, key in ((grad1, "g1"), (grad2, "g2")):
        want = golden_emd[f"{name}_{key}"]
        assert np.abs(got.numpy() - want).max() <= EPS * np.abs(want).max()


def test_function_makes_its_inputs_contiguous_and_is_once_differentiable(statement):
    from adaptpoint_amd import emd as E
    xyz1, xyz2 = ER.golden_inputs("tiny")
    a = _t(xyz1).double().transpose(1, 2).contiguous().transpose(1, 2).requires_grad_(True)     # (B,n,3), strided
    assert not a.is_contiguous()
    b = _t(xyz2).double().requires_grad_(True)
    cost = E.EarthMoverDistanceFunction.apply(a, b)             # the statement asserts contiguity
    w = torch.ones_like(cost, requires_grad=True)               # a differentiable grad_cost: a second derivative is asked for
    ga, = torch.autograd.grad((cost * w).sum(), a, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        ga.sum().backward()


def test_argument_checks_raise_the_house_errors_and_covers_agrees():
    from adaptpoint_amd import emd as E
    f32 = lambda *shape: torch.zeros(*shape, dtype=torch.float32)
    a, b = f32(2, 8, 3), f32(2, 5, 3)
    match, tables = f32(2, 5, 8), (f32(2, 10, 8), f32(2, 10, 5))
    for call in (lambda: E.approxmatch_forward(a, b), lambda: E.emd_ratios(a, b),
                 lambda: E.matchcost_forward(a, b, match), lambda: E.matchcost_backward(f32(2), a, b, match),
                 lambda: E.cost(a, b, ratios=tables), lambda: E.cost_grad(f32(2), a, b, ratios=tables),
                 lambda: E.match_from_ratios(a, b, *tables), lambda: E.earth_mover_distance()(a, b)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
    with pytest.raises(RuntimeError, match="xyz1 must be float32"):
        E.approxmatch_forward(a.double(), b.double())
    with pytest.raises(RuntimeError, match="xyz2 must be float32"):
        E.approxmatch_forward(a, b.double())
    with pytest.raises(RuntimeError, match="batch sizes differ"):
        E.approxmatch_forward(a, f32(3, 5, 3))
    with pytest.raises(RuntimeError, match=r"\(B,n,3\)"):
        E.approxmatch_forward(a, f32(2, 5, 4))
    big = torch.empty(1, E.EMD_MAX_POINTS + 1, 3, dtype=torch.float32)
    for x, y in ((big, f32(1, 5, 3)), (f32(1, 5, 3), big), (f32(1, 0, 3), f32(1, 5, 3))):
        with pytest.raises(RuntimeError, match="EMD_MAX_POINTS"):
            E.approxmatch_forward(x, y)
    with pytest.raises(RuntimeError, match="2\\^24"):
        E.emd_ratios(torch.empty(2 ** 22, 4, 3, device="meta"), torch.empty(2 ** 22, 4, 3, device="meta"))
    with pytest.raises(RuntimeError, match="either match or the two ratio tables"):
        E.cost(a, b)
    with pytest.raises(RuntimeError, match="either match or the two ratio tables"):
        E.cost_grad(f32(2), a, b, match=match, ratios=tables)
    # what only a device tensor reaches: meta tensors have shapes, dtypes and strides but claim no memory
    meta = lambda *shape: torch.empty(*shape, dtype=torch.float32, device="meta")
    for x, y in ((a, b), (a.double(), b.double()), (a, f32(3, 5, 3)), (big, f32(1, 5, 3)), (f32(1, 5, 3), big), (a, f32(2, 5, 4))):
        assert E.emd_covers(x, y) is False
    assert E._shape_problem(meta(1, E.EMD_MAX_POINTS, 3), meta(1, 1, 3)) is None
    assert E._shape_problem(meta(2047, 8192, 3), meta(2047, 1, 3)) is None
    assert E._shape_problem(meta(2048, 8192, 3), meta(2048, 1, 3)) is not None


def test_non_contiguous_and_misshapen_arguments_are_named(monkeypatch):
    """The checks that come after "no CPU path" in `_check`'s order, reached with `is_cuda` answered for CPU tensors."""
    from adaptpoint_amd import emd as E

    class OnDevice(torch.Tensor):
        is_cuda = True
    f32 = lambda *shape: torch.zeros(*shape, dtype=torch.float32).as_subclass(OnDevice)
    a, b = f32(2, 8, 3), f32(2, 5, 3)
    strided = f32(2, 3, 8).transpose(1, 2)
    assert not strided.is_contiguous()
    with pytest.raises(RuntimeError, match="xyz1 must be contiguous"):
        E.emd_ratios(strided, b)
    with pytest.raises(RuntimeError, match="match must be float32"):
        E.matchcost_forward(a, b, f32(2, 5, 8).double())
    with pytest.raises(RuntimeError, match="grad_cost must be float32"):
        E.matchcost_backward(f32(2).double(), a, b, f32(2, 5, 8))
    with pytest.raises(RuntimeError, match="match must be contiguous"):
        E.matchcost_forward(a, b, f32(2, 8, 5).transpose(1, 2))
    with pytest.raises(RuntimeError, match=r"match must be \(2, 5, 8\)"):
        E.matchcost_forward(a, b, f32(2, 8, 5))
    with pytest.raises(RuntimeError, match=r"grad_cost must be \(2,\)"):
        E.matchcost_backward(f32(2, 1), a, b, f32(2, 5, 8))
    with pytest.raises(RuntimeError, match=r"ratio_r must be \(2, 10, 5\)"):
        E.cost(a, b, ratios=(f32(2, 10, 8), f32(2, 10, 8)))


def test_library_declares_the_entries_and_agrees_on_the_limits():
    from adaptpoint_amd import _lib, emd as E
    names = {"apn_emd_max_points", "apn_emd_one_launch_max", "apn_emd_cost_parts", "apn_emd_ratios", "apn_emd_match",
             "apn_emd_cost", "apn_emd_cost_grad"}
    assert names <= set(_lib.SIGNATURES)
    lib = _lib.load()
    assert lib.apn_emd_max_points() == E.EMD_MAX_POINTS >= 8192
    assert lib.apn_emd_one_launch_max() == E.EMD_ONE_LAUNCH_MAX
    assert [lib.apn_emd_cost_parts(n) for n in (0, 1, 64, 65, 8192, 8193)] == [0, 1, 1, 2, 128, 0]
    assert E._TILE == 64
    EINVAL, P = -1, 4096                                      # P: a non-null address that is never read

    def ratios(b=2, n=8, m=5, xyz1=P, xyz2=P, ratio_l=P, ratio_r=P, state=P):
        return lib.apn_emd_ratios(b, n, m, xyz1, xyz2, ratio_l, ratio_r, state, None)

    def match(b=2, n=8, m=5, xyz1=P, xyz2=P, ratio_l=P, ratio_r=P, match=P):
        return lib.apn_emd_match(b, n, m, xyz1, xyz2, ratio_l, ratio_r, match, None)

    def cost(b=2, n=8, m=5, xyz1=P, xyz2=P, match=P, ratio_l=P, ratio_r=P, part=P, cost=P):
        return lib.apn_emd_cost(b, n, m, xyz1, xyz2, match, ratio_l, ratio_r, part, cost, None)

    def grad(b=2, n=8, m=5, grad_cost=P, xyz1=P, xyz2=P, match=P, ratio_l=P, ratio_r=P, grad1=P, grad2=P):
        return lib.apn_emd_cost_grad(b, n, m, grad_cost, xyz1, xyz2, match, ratio_l, ratio_r, grad1, grad2, None)
    always = {ratios: ("xyz1", "xyz2", "ratio_l", "ratio_r", "state"), match: ("xyz1", "xyz2", "ratio_l", "ratio_r", "match"),
              cost: ("xyz1", "xyz2", "part", "cost"), grad: ("grad_cost", "xyz1", "xyz2", "grad1", "grad2")}
    for entry, needed in always.items():
        assert entry(b=-1) == EINVAL and entry(n=0) == EINVAL and entry(m=0) == EINVAL and entry(n=-3) == EINVAL
        assert entry(n=E.EMD_MAX_POINTS + 1) == EINVAL and entry(m=E.EMD_MAX_POINTS + 1) == EINVAL
        assert entry(b=2 ** 22, n=4, m=4) == EINVAL and entry(b=2048, n=8192, m=1) == EINVAL        # b max(n, m) = 2^24
        everything = entry.__code__.co_varnames[3:entry.__code__.co_argcount]
        assert entry(b=0, **{k: None for k in everything}) == 0                                     # no clouds: a no-op
        for k in needed:
            assert entry(**{k: None}) == EINVAL, (entry.__name__, k)
    for entry in (cost, grad):                                # without match, both tables are needed
        assert entry(match=None, ratio_l=None) == EINVAL and entry(match=None, ratio_r=None) == EINVAL
