"""The stacked-cloud operators without a GPU: the numpy statements of tests/pointops_reference.py against the golden made
from the reference's own `functions/pointops.py` (tests/golden/make_golden_pointops.py), the exported names, and the
argument validation of every new C entry.

Bars: the float32 statements follow the contract's operation order, the golden is float64.  Their distance is barred by
operation counts -- (terms per sum + roundings per term) x 2^-24 x the sum of the terms' magnitudes, derived case by
case in `pointops_reference.golden_bounds` (a squared distance is within tau = 6 x 2^-24, a square root halves that and
rounds once, an interpolation weight collects 16 x 2^-24) -- never by what the statements happen to give.  Indices are
compared exactly: the generator asserts that every decision the golden records is more than 2 tau from flipping."""
import inspect
import os

import numpy as np
import pytest

import pointops_reference as PR

HERE = os.path.dirname(os.path.abspath(__file__))
EINVAL = -1
P = 4096                          # a non-null address that is never read


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(HERE, "golden", "pointops_golden.npz"))


@pytest.fixture(scope="module")
def scene(gold):
    return PR.golden_scene(int(gold["seed"]))


@pytest.mark.parametrize("f", [np.float32, np.float64])
def test_statements_reproduce_the_golden_indices(gold, scene, f):
    xyz, off, noff = scene["xyz"], scene["offset"], scene["new_offset"]
    fidx, tmp, written, _ = PR.fps_tree(xyz, off, noff, max(PR.SIZES), f)
    assert written.all() and np.array_equal(fidx, gold["fps_idx"])
    assert list(np.diff(np.concatenate(([0], noff)))) == list(PR.quarter(PR.SIZES)) and 0 in PR.quarter(PR.SIZES)
    coarse = xyz[fidx]
    assert np.array_equal(PR.knn(3, xyz, xyz, off, off, f)[0], gold["knn3_idx"])
    assert np.array_equal(PR.knn(16, xyz, coarse, off, noff, f)[0], gold["knn16_idx"])
    assert np.array_equal(PR.knn(33, xyz, coarse, off, noff, f)[0], gold["knn33_idx"])
    assert np.array_equal(PR.knn(3, coarse, coarse, noff, noff, f)[0], gold["cknn3_idx"])
    assert np.array_equal(PR.ball(PR.GOLDEN_CASES["ball"][3], 16, xyz, coarse, off, noff, f), gold["ball_idx"])
    # the kept quirk, present in the golden: the 1-point and 5-point clouds pad k = 16 with the cloud's first row
    starts = np.concatenate(([0], off[:-1]))
    qcloud = np.array([PR.cloud_of(q, noff) for q in range(len(coarse))])
    for cloud, size in ((1, 5), (3, 1)):
        rows = gold["knn16_idx"][qcloud == cloud]
        assert (rows[:, size:] == starts[cloud]).all()


def test_float32_statements_reproduce_the_golden_values_within_the_derived_bars(gold, scene):
    bars, got = PR.golden_bounds(scene, gold), PR.golden_eval32(scene, gold)
    assert set(bars) == set(got)
    for name, bar in bars.items():
        err = np.abs(np.asarray(got[name], dtype=np.float64) - gold[name])
        assert np.shape(err) == np.shape(gold[name]) and (err <= bar).all(), (name, float(err.max()))
    # the bars are error bars, not tolerances: a perturbation of a few 1e-6 relative is caught
    assert (np.abs(got["agg_out"] * (1 + 4e-6) - gold["agg_out"]) > bars["agg_out"]).any()


def test_statements_agree_with_elementary_forms():
    """csr is the inverse of the index; the list sums equal np.add.at on small integers (exact in any order); the FPS tree
    prefers the smallest bit-reversed thread among equal maxima."""
    rng = np.random.default_rng(5)
    idx = rng.integers(-2, 12, (9, 4)).astype(np.int32)               # some outside [0, 10): clamped
    pcnt, poff, plist = PR.csr(idx, 10)
    flat = PR.clamp(idx, 10).reshape(-1)
    assert pcnt.sum() == 36
    for j in range(10):
        lst = plist[poff[j]:poff[j] + pcnt[j]]
        assert (np.diff(lst) > 0).all() and (flat[lst] == j).all()
    g = PR.small_ints((9, 4, 3), 1)
    want = np.zeros((10, 3))
    np.add.at(want, flat, g.reshape(-1, 3))
    for f in (np.float32, np.float64):
        assert np.array_equal(PR.grouping_bwd(g, idx, 10, f), want)
    # four points at the corners of a square around the first pick: rows 1, 2, 3 tie; T = 4, bit-reversed ids 2, 1, 3
    sq = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float32)
    fidx = PR.fps_tree(sq, np.array([4], np.int32), np.array([2], np.int32), 4, np.float32)[0]
    assert list(fidx) == [0, 2]


def test_shim_and_module_export_the_reference_names():
    import pointops_cuda
    from adaptpoint_amd import pointops
    eleven = ["knnquery_cuda", "ballquery_cuda", "furthestsampling_cuda"] + [
        f"{op}_{d}_cuda" for op in ("grouping", "interpolation", "subtraction", "aggregation") for d in ("forward", "backward")]
    assert sorted(pointops_cuda.__all__) == sorted(eleven)
    for name in eleven:
        assert getattr(pointops_cuda, name) is getattr(pointops, name)
    args = lambda fn: list(inspect.signature(fn).parameters)
    assert args(pointops.knnquery_cuda) == ["m", "nsample", "xyz", "new_xyz", "offset", "new_offset", "idx", "dist2"]
    assert args(pointops.subtraction_backward_cuda) == ["n", "nsample", "c", "idx", "grad_output", "grad_input1", "grad_input2"]
    assert args(pointops.aggregation_backward_cuda)[4:] == ["input", "position", "weight", "idx", "grad_output", "grad_input",
                                                            "grad_position", "grad_weight"]
    for name in ("FurthestSampling", "KNNQuery", "BallQuery", "Grouping", "Subtraction", "Aggregation", "Interpolation"):
        assert issubclass(getattr(pointops, name), __import__("torch").autograd.Function)
    for name in ("furthestsampling", "knnquery", "ballquery", "grouping", "querygroup", "queryandgroup", "subtraction",
                 "aggregation", "interpolation", "interpolation2", "pointops_covers"):
        assert callable(getattr(pointops, name))
    assert args(pointops.queryandgroup) == ["nsample", "xyz", "new_xyz", "feat", "idx", "offset", "new_offset", "use_xyz"]
    assert args(pointops.interpolation) == ["xyz", "new_xyz", "feat", "offset", "new_offset", "k"]
    import torch
    cpu = torch.zeros(4, 3)
    assert not pointops.pointops_covers(cpu, torch.tensor([4], dtype=torch.int32))       # CPU tensors: no
    with pytest.raises(RuntimeError, match="CUDA/HIP"):
        pointops.knnquery_cuda(4, 1, cpu, cpu, torch.tensor([4], dtype=torch.int32), torch.tensor([4], dtype=torch.int32),
                               torch.zeros(4, 1, dtype=torch.int32), torch.zeros(4, 1))


def test_argument_validation_of_the_pointops_entries_needs_no_gpu():
    """Limits alone with non-null dummy pointers, empty work, then each null pointer: every check returns before any
    HIP call."""
    from adaptpoint_amd import _lib
    lib = _lib.load()
    big = 1 << 24

    def nulls(call, count):
        """call(pointers) with every pointer set, then each one null in turn."""
        for hole in range(count):
            assert call([None if i == hole else P for i in range(count)]) == EINVAL, hole

    knn = lambda b=2, n=8, m=8, k=3, p=(P,) * 6: lib.apn_po_knn_query(b, n, m, k, *p, None)
    assert knn(b=0) == EINVAL and knn(n=-1) == EINVAL and knn(m=-1) == EINVAL and knn(n=big) == EINVAL and knn(m=big) == EINVAL
    assert knn(k=0) == EINVAL and knn(k=101) == EINVAL
    assert knn(m=0) == 0 and knn(n=0) == 0 and knn(m=0, p=(None,) * 6) == 0
    nulls(lambda p: knn(p=p), 6)

    ball = lambda b=2, n=8, m=8, r=0.5, ns=4, p=(P,) * 5: lib.apn_po_ball_query(b, n, m, r, ns, *p, None)
    assert ball(b=0) == EINVAL and ball(n=big) == EINVAL and ball(m=-1) == EINVAL and ball(ns=0) == EINVAL
    assert ball(r=-1.0) == EINVAL and ball(r=float("nan")) == EINVAL
    assert ball(m=0) == 0 and ball(n=0) == 0
    nulls(lambda p: ball(p=p), 5)

    fps = lambda b=2, n_max=8, p=(P,) * 5: lib.apn_po_furthest_sampling(b, n_max, *p, None)
    assert fps(b=-1) == EINVAL and fps(n_max=-1) == EINVAL and fps(n_max=big) == EINVAL
    assert fps(b=0) == 0 and fps(n_max=0) == 0
    nulls(lambda p: fps(p=p), 5)

    csr = lambda n=8, m=8, k=3, p=(P,) * 4: lib.apn_po_csr(n, m, k, *p, None)
    assert csr(n=-1) == EINVAL and csr(m=big) == EINVAL and csr(k=0) == EINVAL and csr(m=big - 1, k=129) == EINVAL
    assert csr(n=0) == 0
    nulls(lambda p: csr(p=p), 4)

    feat = {   # name: (pointer count, takes w_c, no-op sizes)
        "apn_po_grouping_fwd": (3, False, (dict(n=0), dict(m=0))),
        "apn_po_grouping_bwd": (4, False, (dict(n=0),)),
        "apn_po_interpolation_fwd": (4, False, (dict(n=0), dict(m=0))),
        "apn_po_interpolation_bwd": (5, False, (dict(n=0),)),
        "apn_po_subtraction_fwd": (4, False, (dict(n=0), dict(m=0))),
        "apn_po_subtraction_bwd": (5, False, (dict(n=0, m=0),)),
        "apn_po_aggregation_fwd": (5, True, (dict(n=0), dict(m=0))),
        "apn_po_aggregation_bwd": (10, True, (dict(n=0),)),
    }
    for name, (count, has_wc, noops) in feat.items():
        fn = getattr(lib, name)

        def call(n=8, m=8, k=3, c=4, w_c=2, p=None, fn=fn, count=count, has_wc=has_wc):
            p = (P,) * count if p is None else p
            return fn(n, m, k, c, *((w_c,) if has_wc else ()), *p, None)
        for bad in (dict(n=-1), dict(m=-1), dict(n=big), dict(m=big), dict(k=0), dict(c=0), dict(c=65537),
                    dict(m=big - 1, k=129)):
            assert call(**bad) == EINVAL, (name, bad)
        if has_wc:
            assert call(w_c=0) == EINVAL and call(w_c=3) == EINVAL, name          # c % w_c != 0
        for sizes in noops:
            assert call(**sizes) == 0, (name, sizes)
        nulls(lambda p: call(p=p), count)
