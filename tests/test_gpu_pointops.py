"""GPU suite: the stacked-cloud operators (csrc/pointops.hip, apn_po_csr) through `adaptpoint_amd.pointops` against the
numpy statements of their contract (tests/pointops_reference.py).

No tolerance wherever the contract fixes the order:
  * integer-lattice clouds -- squared distances are small integers, exact in fp32, and ties are plentiful -- so kNN indices
    and distances EQUAL the (d2, index) sort, the ball query and the sampler (with the reference's positional tie rule,
    emulated thread by thread) EQUAL their statements;
  * values and gradients of grouping, interpolation, subtraction and aggregation on seeded normal inputs EQUAL the float32
    statements bit for bit (the interpolation entry is fed host-computed weights, so that torch's device division is not
    part of the comparison); with small-integer inputs every backward EQUALS the float64 statement (the sum of magnitudes
    stays below 2^24, asserted).
Against the golden (the reference's own Functions over the float64 statements, uniform clouds): indices equal, values and
gradients within the bars derived from operation counts in `pointops_reference.golden_bounds`.

Cloud sets: SIZES = (70, 5, 200, 1, 129, 300) with queries = supports; the same supports queried by the first quarter of
every cloud ((17, 1, 50, 0, 32, 75): an empty query cloud in the middle); one cloud of 1100 (T = 1024, more rows than
threads, past one kNN chunk); 300 clouds of 16.  k crosses the one-register / two-register list at 64 | 65."""
import functools
import gc
import os

import numpy as np
import pytest
import torch

import pointops_reference as PR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETS = {"self": (PR.SIZES, False), "quarter": (PR.SIZES, True), "big": ((1100,), False), "many": ((16,) * 300, False)}
KS = [1, 3, 16, 33, 64, 65, 100]
CS = [1, 3, 32, 33]
AGG = [(32, 4), (6, 3), (33, 33), (8, 1)]
F32, F64 = np.float32, np.float64


@functools.lru_cache(maxsize=None)
def cloud_set(name, lattice=True):
    """xyz, new_xyz, offset, new_offset of a cloud set; the quarter queries are the first rows of every cloud."""
    sizes, quarter = SETS[name]
    xyz = PR.lattice_clouds(sizes, 77) if lattice else PR.seeded_clouds(sizes, 78)
    off = PR.offsets(sizes)
    if not quarter:
        return xyz, xyz, off, off
    rows = np.concatenate([np.arange(s, s + (e - s) // 4) for s, e in PR.ranges(off)])
    return xyz, xyz[rows], off, PR.offsets(PR.quarter(sizes))


@functools.lru_cache(maxsize=None)
def knn_statement(name):
    """The (d2, index) sort at k = 100 (float32 = float64 on a lattice); a smaller k is its leading columns."""
    xyz, new_xyz, off, noff = cloud_set(name)
    idx, d2 = PR.knn(100, xyz, new_xyz, off, noff, F32)
    idx.setflags(write=False)
    d2.setflags(write=False)
    return idx, d2


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "pointops_golden.npz"))


@pytest.fixture(scope="module")
def scene(gold):
    return PR.golden_scene(int(gold["seed"]))


def T(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def N(t):
    return t.detach().cpu().numpy()


def raw_knn(dev, k, xyz, new_xyz, off, noff):
    from adaptpoint_amd import pointops as PO
    a, q = T(dev, xyz), T(dev, new_xyz)
    assert PO.pointops_covers(a, T(dev, off), q, T(dev, noff))
    idx = torch.full((len(new_xyz), k), -7, dtype=torch.int32, device=dev)
    d2 = torch.full((len(new_xyz), k), -7.0, dtype=torch.float32, device=dev)
    PO.knnquery_cuda(len(new_xyz), k, a, q, T(dev, off), T(dev, noff), idx, d2)
    return N(idx), N(d2)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", list(SETS))
def test_knn_on_lattices_equals_the_sorted_statement(dev, name, k):
    xyz, new_xyz, off, noff = cloud_set(name)
    want_i, want_d = knn_statement(name)
    idx, d2 = raw_knn(dev, k, xyz, new_xyz, off, noff)
    assert np.array_equal(idx, want_i[:, :k]) and np.array_equal(d2, want_d[:, :k])


def test_knn_pads_short_clouds_with_the_cloud_start_and_1e10(dev):
    """The kept quirk, at cloud sizes 1 and 5 with k = 16; the Function's sqrt turns 1e10 into 1e5."""
    from adaptpoint_amd import pointops as PO
    xyz, new_xyz, off, noff = cloud_set("self")
    idx, d2 = raw_knn(dev, 16, xyz, new_xyz, off, noff)
    for (s, e) in PR.ranges(off):
        if e - s in (1, 5):
            assert (idx[s:e, e - s:] == s).all() and (d2[s:e, e - s:] == np.float32(1e10)).all()
            assert (idx[s:e, :e - s] >= s).all() and (d2[s:e, :e - s] < 1e10).all()
    _, dist = PO.knnquery(16, T(dev, xyz), None, T(dev, off), T(dev, off))
    assert N(dist)[70, 5] == np.float32(1e5)              # the 5-point cloud starts at row 70


@pytest.mark.parametrize("radius,nsample", [(1.5, 8), (2.5, 33), (3.0, 70), (0.0, 4)])
@pytest.mark.parametrize("name", list(SETS))
def test_ball_query_on_lattices_equals_the_statement(dev, name, radius, nsample):
    from adaptpoint_amd import pointops as PO
    xyz, new_xyz, off, noff = cloud_set(name)
    idx = torch.full((len(new_xyz), nsample), -7, dtype=torch.int32, device=dev)
    PO.ballquery_cuda(len(new_xyz), radius, nsample, T(dev, xyz), T(dev, new_xyz), T(dev, off), T(dev, noff), idx)
    want = PR.ball(radius, nsample, xyz, new_xyz, off, noff, F32)
    assert np.array_equal(N(idx), want)
    if radius == 0.0:
        assert not want.any()                             # no hit: zeros


FPS_CASES = {   # name: (cloud sizes, sample sizes): T and rows per thread -> the kernel's variants
    "T64": ((70, 5, 100, 1, 64), (17, 1, 25, 0, 64)),
    "T256": (PR.SIZES, PR.quarter(PR.SIZES)),
    "T256-all": (PR.SIZES, PR.SIZES),
    "T1024-2rows": ((1100, 3), (275, 3)),
    "T1024-4rows": ((3000,), (24,)),
    "T1024-8rows": ((5000, 1030), (24, 24)),
    "T1024-16rows": ((12000,), (24,)),
    "T1024-24rows": ((17000, 2), (24, 1)),
    "T1024-streamed": ((25000, 40), (24, 0)),
}


@pytest.mark.parametrize("name", list(FPS_CASES))
def test_furthest_sampling_on_lattices_equals_the_tree_statement(dev, name):
    """Distances are exact and equal maxima abound: only the reference's positional tie rule gives these picks."""
    from adaptpoint_amd import pointops as PO
    sizes, samples = FPS_CASES[name]
    xyz, off, noff = PR.lattice_clouds(sizes, 91), PR.offsets(sizes), PR.offsets(samples)
    want, want_tmp, written, _ = PR.fps_tree(xyz, off, noff, max(sizes), F32)
    idx = torch.full((int(noff[-1]),), -7, dtype=torch.int32, device=dev)
    tmp = torch.full((len(xyz),), 1e10, dtype=torch.float32, device=dev)
    PO.furthestsampling_cuda(len(sizes), max(sizes), T(dev, xyz), T(dev, off), T(dev, noff), tmp, idx)
    assert written.all() and np.array_equal(N(idx), want)
    assert np.array_equal(N(tmp), want_tmp)
    got = PO.furthestsampling(T(dev, xyz), T(dev, off), T(dev, noff))
    assert got.dtype == torch.int32 and np.array_equal(N(got), want)


def test_golden_indices(dev, gold, scene):
    from adaptpoint_amd import pointops as PO
    xyz, off, noff = T(dev, scene["xyz"]), T(dev, scene["offset"]), T(dev, scene["new_offset"])
    fidx = PO.furthestsampling(xyz, off, noff)
    assert np.array_equal(N(fidx), gold["fps_idx"])
    coarse = xyz[fidx.long()].contiguous()
    idx3, dist3 = PO.knnquery(3, xyz, None, off, off)
    assert np.array_equal(N(idx3), gold["knn3_idx"])
    assert (np.abs(N(dist3).astype(F64) - gold["knn3_dist"]) <= PR.TAU * gold["knn3_dist"]).all()
    assert np.array_equal(N(PO.knnquery(16, xyz, coarse, off, noff)[0]), gold["knn16_idx"])
    assert np.array_equal(N(PO.knnquery(33, xyz, coarse, off, noff)[0]), gold["knn33_idx"])
    assert np.array_equal(N(PO.knnquery(3, coarse, coarse, noff, noff)[0]), gold["cknn3_idx"])
    assert np.array_equal(N(PO.ballquery(PR.GOLDEN_CASES["ball"][3], 16, xyz, coarse, off, noff)), gold["ball_idx"])


def feature_case(name, k, c, w_c=None):
    """Seeded normal inputs on a cloud set's lattice kNN graph: idx (m,k), supports' and queries' features."""
    xyz, new_xyz, off, noff = cloud_set(name)
    idx = knn_statement(name)[0][:, :k].copy()
    n, m = len(xyz), len(new_xyz)
    seed = 17 * k + c
    return dict(n=n, m=m, idx=idx, inp=PR.features((n, c), seed), qry=PR.features((m, c), seed + 1),
                pos=PR.features((m, k, c), seed + 2), wk=PR.features((m, k), seed + 3),
                wc=PR.features((m, k, w_c or 1), seed + 4), g_mkc=PR.features((m, k, c), seed + 5),
                g_mc=PR.features((m, c), seed + 6))


def run_ops(dev, case, k, c, w_c, ints=False):
    """Every differentiable raw entry on a case -> name: array."""
    from adaptpoint_amd import pointops as PO
    n, m = case["n"], case["m"]
    d = {key: T(dev, v) for key, v in case.items() if isinstance(v, np.ndarray)}
    e = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=dev)
    out = {}
    out["group"] = e(m, k, c)
    PO.grouping_forward_cuda(m, k, c, d["inp"], d["idx"], out["group"])
    out["group_g"] = e(n, c)
    PO.grouping_backward_cuda(m, k, c, d["g_mkc"], d["idx"], out["group_g"])
    out["interp"] = e(m, c)
    PO.interpolation_forward_cuda(m, c, k, d["inp"], d["idx"], d["wk"], out["interp"])
    out["interp_g"] = e(n, c)
    PO.interpolation_backward_cuda(m, c, k, d["g_mc"], d["idx"], d["wk"], out["interp_g"])
    out["sub"] = e(m, k, c)
    PO.subtraction_forward_cuda(m, k, c, d["qry"], d["inp"], d["idx"], out["sub"])
    out["sub_g1"], out["sub_g2"] = e(m, c), e(n, c)
    PO.subtraction_backward_cuda(m, k, c, d["idx"], d["g_mkc"], out["sub_g1"], out["sub_g2"])
    if w_c:
        out["agg"] = e(m, c)
        PO.aggregation_forward_cuda(m, k, c, w_c, d["inp"], d["pos"], d["wc"], d["idx"], out["agg"])
        out["agg_gi"], out["agg_gp"], out["agg_gw"] = e(n, c), e(m, k, c), e(m, k, w_c)
        PO.aggregation_backward_cuda(m, k, c, w_c, d["inp"], d["pos"], d["wc"], d["idx"], d["g_mc"], out["agg_gi"],
                                     out["agg_gp"], out["agg_gw"])
    return {key: N(v) for key, v in out.items()}


def statement_ops(case, w_c, f):
    n, idx = case["n"], case["idx"]
    out = {"group": PR.grouping_fwd(case["inp"], idx, f), "group_g": PR.grouping_bwd(case["g_mkc"], idx, n, f),
           "interp": PR.interpolation_fwd(case["inp"], idx, case["wk"], f),
           "interp_g": PR.interpolation_bwd(case["g_mc"], idx, case["wk"], n, f),
           "sub": PR.subtraction_fwd(case["qry"], case["inp"], idx, f)}
    out["sub_g1"], out["sub_g2"] = PR.subtraction_bwd(case["g_mkc"], idx, n, f)
    if w_c:
        out["agg"] = PR.aggregation_fwd(case["inp"], case["pos"], case["wc"], idx, f)
        out["agg_gi"], out["agg_gp"], out["agg_gw"] = PR.aggregation_bwd(case["inp"], case["pos"], case["wc"], idx,
                                                                           case["g_mc"], f)
    return out


def assert_same_bits(got, want):
    assert set(got) == set(want)
    for key in want:
        assert got[key].shape == want[key].shape and got[key].dtype == np.float32, key
        assert np.array_equal(got[key].view(np.int32), np.ascontiguousarray(want[key], dtype=F32).view(np.int32)), key


@pytest.mark.parametrize("name,k", [("quarter", 3), ("quarter", 16), ("many", 16), ("big", 3)])
@pytest.mark.parametrize("c", CS)
def test_values_and_gradients_equal_the_float32_statement_bit_for_bit(dev, name, k, c):
    case = feature_case(name, k, c)
    assert_same_bits(run_ops(dev, case, k, c, None), statement_ops(case, None, F32))


@pytest.mark.parametrize("name,k", [("quarter", 3), ("many", 16)])
@pytest.mark.parametrize("c,w_c", AGG)
def test_aggregation_equals_the_float32_statement_bit_for_bit(dev, name, k, c, w_c):
    case = feature_case(name, k, c, w_c)
    got, want = run_ops(dev, case, k, c, w_c), statement_ops(case, w_c, F32)
    assert_same_bits({key: v for key, v in got.items() if key.startswith("agg")},
                     {key: v for key, v in want.items() if key.startswith("agg")})


def test_interpolation_with_host_weights_equals_the_statement(dev):
    """The composed use: kNN on seeded clouds, weights computed on the host in float32 from the kernel's distances."""
    xyz, new_xyz, off, noff = cloud_set("quarter", lattice=False)
    coarse = new_xyz                                             # interpolate from the quarter rows back to all rows
    idx, d2 = raw_knn(dev, 3, coarse, xyz, noff, off)
    w = PR.interpolation_weights(d2, F32)
    case = dict(n=len(coarse), m=len(xyz), idx=idx, inp=PR.features((len(coarse), 33), 5), wk=w,
                g_mc=PR.features((len(xyz), 33), 6))
    from adaptpoint_amd import pointops as PO
    d = {key: T(dev, v) for key, v in case.items() if isinstance(v, np.ndarray)}
    out = torch.empty(case["m"], 33, device=dev)
    grad = torch.empty(case["n"], 33, device=dev)
    PO.interpolation_forward_cuda(case["m"], 33, 3, d["inp"], d["idx"], d["wk"], out)
    PO.interpolation_backward_cuda(case["m"], 33, 3, d["g_mc"], d["idx"], d["wk"], grad)
    assert_same_bits({"out": N(out), "grad": N(grad)},
                     {"out": PR.interpolation_fwd(case["inp"], idx, w, F32),
                      "grad": PR.interpolation_bwd(case["g_mc"], idx, w, case["n"], F32)})


@pytest.mark.parametrize("name,k", [("self", 16), ("quarter", 65), ("many", 3), ("big", 100)])
def test_csr_is_the_sorted_inverse_of_the_index(dev, name, k):
    from adaptpoint_amd import pointops as PO
    xyz, new_xyz, _, _ = cloud_set(name)
    idx = knn_statement(name)[0][:, :k].copy()
    n, m = len(xyz), len(new_xyz)
    csr = PO.build_csr(T(dev, idx), n)
    pcnt, poff, plist = N(csr.pcnt), N(csr.poff), N(csr.plist)
    want = PR.csr(idx, n)
    assert int(pcnt.sum()) == m * k
    assert np.array_equal(pcnt, want[0]) and np.array_equal(poff, want[1]) and np.array_equal(plist, want[2])
    ends = poff + pcnt
    inner = np.ones(m * k, dtype=bool)
    inner[poff[pcnt > 0]] = False                                # list starts
    assert (np.diff(plist)[inner[1:]] > 0).all() and ends.max() == m * k


@pytest.mark.parametrize("name,k,c,w_c", [("quarter", 16, 6, 3), ("many", 16, 33, 33), ("big", 3, 8, 1)])
def test_small_integer_backwards_equal_the_float64_statement(dev, name, k, c, w_c):
    case = feature_case(name, k, c, w_c)
    for key in ("inp", "qry", "pos", "wk", "wc", "g_mkc", "g_mc"):
        case[key] = PR.small_ints(case[key].shape, 3 + len(key) + k, hi=3)
    pcnt = PR.csr(case["idx"], case["n"])[0]
    # every term is an integer of magnitude <= 3 * (3 + 3) = 18, a list or slot sum has at most max(pcnt, k, c) of them
    assert 18 * max(int(pcnt.max()), k, c) < 2 ** 24
    got, want = run_ops(dev, case, k, c, w_c), statement_ops(case, w_c, F64)
    for key in ("group_g", "interp_g", "sub_g1", "sub_g2", "agg_gi", "agg_gp", "agg_gw"):
        assert np.array_equal(got[key].astype(F64), want[key]), key


def module_results(dev, scene, gold):
    """Everything `golden_bounds` bars, through the module's Functions; losses are summed in float64."""
    from adaptpoint_amd import pointops as PO
    t = lambda key, grad=False: T(dev, scene[key]).requires_grad_(grad)
    xyz, off, noff = t("xyz"), t("offset"), t("new_offset")
    coarse = xyz[PO.furthestsampling(xyz, off, noff).long()].contiguous()
    out = {"knn3_dist": N(PO.knnquery(3, xyz, xyz, off, off)[1])}
    for name, use_xyz in (("qg_xyz", True), ("qg_feat", False)):
        a, b, f = t("xyz", True), coarse.clone().requires_grad_(True), t("feat", True)
        val = PO.queryandgroup(16, a, b, f, None, off, noff, use_xyz=use_xyz)
        w = t(f"w_{name}")
        val.backward(w)
        out[f"{name}_loss"] = float((val.detach().double() * w.double()).sum())
        out[f"{name}_gfeat"] = N(f.grad)
        if use_xyz:
            out[f"{name}_gxyz"], out[f"{name}_gnew"] = N(a.grad), N(b.grad)
    f = t("cfeat", True)
    val = PO.interpolation2(coarse, xyz, f, noff, off, 3)
    val.backward(t("w_interp"))
    out["interp_out"], out["interp_gfeat"] = N(val), N(f.grad)
    assert torch.equal(PO.interpolation(coarse, xyz, f.detach(), noff, off, 3), val.detach())      # the composed name
    cidx, _ = PO.knnquery(3, coarse, coarse, noff, noff)
    a, b = t("in1", True), t("in2", True)
    val = PO.subtraction(a, b, cidx)
    val.backward(t("w_sub"))
    out["sub_loss"] = float((val.detach().double() * t("w_sub").double()).sum())
    out["sub_g1"], out["sub_g2"] = N(a.grad), N(b.grad)
    a, p, w = t("ainp", True), t("apos", True), t("aw", True)
    val = PO.aggregation(a, p, w, cidx)
    val.backward(t("w_agg"))
    out["agg_out"], out["agg_ginp"], out["agg_gpos"], out["agg_gw"] = N(val), N(a.grad), N(p.grad), N(w.grad)
    assert getattr(cidx, "_apn_po_csr", None) is not None           # one list build, shared by both Functions
    return out


def test_module_functions_equal_the_golden_within_the_derived_bars(dev, gold, scene):
    bars, got = PR.golden_bounds(scene, gold), module_results(dev, scene, gold)
    assert set(bars) == set(got)
    for name, bar in bars.items():
        err = np.abs(np.asarray(got[name], dtype=F64) - gold[name])
        print(name, float(err.max()), float((err / np.maximum(bar, 1e-300)).max()))
        assert np.shape(err) == np.shape(gold[name]) and (err <= bar).all(), (name, float(err.max()))


def test_two_runs_give_the_same_bits(dev, gold, scene):
    a, b = module_results(dev, scene, gold), module_results(dev, scene, gold)
    for key in a:
        assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), key
    case = feature_case("many", 16, 33, 33)
    first, second = run_ops(dev, case, 16, 33, 33), run_ops(dev, case, 16, 33, 33)
    assert_same_bits(first, second)


def test_indices_outside_the_rows_are_clamped(dev):
    """A hand-made idx with entries below 0 and at or past n: every entry computes what the statement gives on the
    clamped indices (the statements clamp as the contract says)."""
    case = feature_case("quarter", 3, 6, 3)
    idx = case["idx"].copy()
    idx[::5, 0] = -3
    idx[1::7, 1] = case["n"]
    idx[2::11, 2] = 2 ** 31 - 1
    case["idx"] = idx
    got, want = run_ops(dev, case, 3, 6, 3), statement_ops(case, 3, F32)
    assert_same_bits(got, want)
    clamped = dict(case, idx=PR.clamp(idx, case["n"]).astype(np.int32))
    assert_same_bits(got, statement_ops(clamped, 3, F32))


def test_chain_replayed_from_a_hipgraph_equals_eager_without_a_memset_node(dev):
    """knnquery -> grouping -> subtraction -> aggregation -> (sum, as its gradient handed to autograd) -> backward."""
    from adaptpoint_amd import graphs, pointops as PO
    xyz_np, _, off_np, _ = cloud_set("self", lattice=False)
    n, c, k = len(xyz_np), 32, 16
    xyz, off = T(dev, xyz_np), T(dev, off_np)
    f1, f2, f3 = (T(dev, PR.features((n, c), 40 + i)).requires_grad_(True) for i in range(3))
    w = T(dev, PR.features((n, c), 44))

    def step():
        idx, _ = PO.knnquery(k, xyz, xyz, off, off)
        pos = PO.grouping(f1, idx)
        wgt = PO.subtraction(f2, f3, idx)
        out = PO.aggregation(f1, pos, wgt, idx)
        return [idx, out.detach(), *torch.autograd.grad(out, [f1, f2, f3], w)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                       # warm-up: allocator pools, lazy initialisation
        step()
    torch.cuda.current_stream().wait_stream(side)
    eager = [t.detach().clone() for t in step()]
    torch.cuda.synchronize()
    gc.collect()
    graph, captured, census = graphs.capture(step, leaves=[f1, f2, f3], what="the pointops chain's graph")
    print("pointops chain graph:", census)
    assert not census.get("memset", 0) and census.get("kernel", 0) >= 10
    for _ in range(2):
        for t in captured:
            t.detach().zero_()
        graph.replay()
        torch.cuda.synchronize()
        for x, y in zip(eager, captured):
            assert torch.equal(x, y.detach())
