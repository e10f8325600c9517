"""CPU suite of the voxel grid: the numpy statement of its contract (tests/voxel_grid_reference.py) reproduces the
reference's own `voxelize` on the golden scene (tests/golden/voxelize_golden.npz) exactly, its outputs satisfy the
contract's invariants, and the apn_vg_* entries validate their arguments before any HIP call."""
import os

import numpy as np
import pytest

import voxel_grid_reference as VR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "voxelize_golden.npz"))


@pytest.fixture(scope="module")
def scene():
    coord, offset = VR.golden_scene()
    return coord, offset, VR.statement(coord, VR.VOXEL, offset)


def ranges(offset):
    return list(zip(np.concatenate([[0], offset[:-1]]).tolist(), offset.tolist()))


def test_statement_reproduces_the_reference_partition_and_counts(gold, scene):
    """Every point of every cloud: same smallest same-voxel row as under the reference's voxelize(mode=1); the sorted
    counts and the voxel totals equal; the scene is the one the golden was made from."""
    coord, offset, st = scene
    assert np.array_equal(gold["offset"], offset) and float(gold["voxel"]) == VR.VOXEL
    assert st["bad"] == 0
    labels = st["first"].astype(np.int64)[st["voxel_of"]]            # the smallest row of every row's voxel
    ends = []
    for c, (lo, hi) in enumerate(ranges(offset)):
        assert np.array_equal(labels[lo:hi] - lo, gold[f"label_{c}"]), c
        mine = st["count"][(st["first"] >= lo) & (st["first"] < hi)]
        assert np.array_equal(np.sort(mine), gold[f"counts_{c}"]), c
        ends.append(len(gold[f"counts_{c}"]))
    assert np.array_equal(st["new_offset"], np.cumsum(ends))
    assert st["m"] == sum(ends) and st["count_max"] == max(int(gold[f"counts_{c}"].max()) for c in range(3))


def test_float32_division_would_move_face_points(gold, scene):
    coord = scene[0]
    moved = (np.floor(coord / np.float32(VR.VOXEL)) != VR.cells(coord, VR.VOXEL)).any(1).sum()
    assert moved == int(gold["moved_f32"]) and moved >= 100


def test_statement_invariants(scene):
    coord, offset, st = scene
    n, m = len(coord), st["m"]
    vo, cnt, start, order = st["voxel_of"], st["count"], st["start"], st["idx_sort"]
    assert np.array_equal(np.sort(order), np.arange(n))                                  # a permutation
    assert np.array_equal(order, np.argsort(vo, kind="stable"))
    assert (np.diff(vo[order]) >= 0).all()
    same = vo[order][1:] == vo[order][:-1]
    assert (np.diff(order)[same] > 0).all()                                             # ascending row inside a voxel
    assert np.array_equal(start, np.cumsum(cnt) - cnt) and cnt.sum() == n and (cnt >= 1).all()
    assert np.array_equal(cnt, np.bincount(vo, minlength=m))
    assert np.array_equal(st["first"], order[start]) and (np.diff(st["first"]) > 0).all()   # numbered by first row
    seen = np.maximum.accumulate(vo)
    assert vo[0] == 0 and (np.diff(seen) <= 1).all()                                    # a new number is the next number
    cloud = VR.clouds_of(n, offset)
    assert (np.diff(cloud[st["first"]]) >= 0).all()                                     # a cloud's voxels are contiguous
    cell = VR.cells(coord, VR.VOXEL)
    key = np.concatenate([cell, cloud[:, None].astype(np.float64)], 1)
    assert (key == key[st["first"][vo]]).all()                                          # a voxel has one (cloud, cell)
    assert len(np.unique(key, axis=0)) == m                                             # ... and no two share one


def test_statement_edge_cases():
    st = VR.statement(np.zeros((0, 3), np.float32), 0.1, np.array([0, 0], np.int32))
    assert st["m"] == 0 and st["count_max"] == 0 and np.array_equal(st["new_offset"], [0, 0])
    pts = np.array([[0.5, 0.5, 0.5], [-0.5, 0.5, 0.5], [0.5, 0.5, 0.5], [0.55, 0.5, 0.5]], np.float32)
    st = VR.statement(pts, 1.0, np.array([2, 2, 4], np.int32))                           # an empty middle cloud
    assert np.array_equal(st["voxel_of"], [0, 1, 2, 2]) and np.array_equal(st["new_offset"], [2, 2, 3])
    assert np.array_equal(st["count"], [1, 1, 2]) and np.array_equal(st["idx_sort"], [0, 1, 2, 3])
    st = VR.statement(np.array([[1e12, 0, 0], [np.nan, 0, 0], [0, 0, 0]], np.float32), 0.04)
    assert st["bad"] == 2
    vals = np.array([[1.0], [2.0], [4.0], [8.0]], np.float32)
    st = VR.statement(pts, 1.0)
    assert np.array_equal(st["voxel_of"], [0, 1, 0, 0])
    assert np.array_equal(VR.mean(vals, st), np.array([[13.0 / 3.0], [2.0]], np.float32))


def test_argument_validation_of_the_voxel_grid_entries_needs_no_gpu():
    """Every apn_vg_* entry returns APN_EINVAL for sizes outside its contract and for null pointers, and 0 for empty
    work, before any HIP call (P: a non-null, 16-byte aligned address that is never read)."""
    from adaptpoint_amd import _lib
    lib = _lib.load()
    EINVAL, P = -1, 4096
    ints = lib.apn_vg_scratch_ints
    assert ints(-1) == 0 and ints(1 << 27) == 0 and ints(0) > 0
    for n in (1, 1000, 10 ** 6, (1 << 27) - 1):
        # cells 4n, a table of at least 2n slots, two arrays of n, the digit counts: between 8n and 11n + 2^17, in an int
        assert 8 * n <= ints(n) <= 11 * n + (1 << 17) < 2 ** 31, n

    names = ("coord", "offset", "scratch", "voxel_of", "count", "start", "idx_sort", "new_offset", "stats")

    def vox(b=1, n=8, is_double=0, vs=(0.1, 0.1, 0.1), null=(), **ptr):
        p = {k: (None if k in null else ptr.get(k, P)) for k in names}
        return lib.apn_vg_voxelize(b, n, is_double, p["coord"], *vs, p["offset"], p["scratch"], p["voxel_of"], p["count"],
                                   p["start"], p["idx_sort"], p["new_offset"], p["stats"], None)
    assert vox(b=0) == EINVAL and vox(b=-1) == EINVAL
    assert vox(n=-1) == EINVAL and vox(n=1 << 27) == EINVAL
    assert vox(is_double=2) == EINVAL and vox(is_double=-1) == EINVAL
    for bad in (0.0, -0.1, float("nan"), float("inf")):
        for axis in range(3):
            vs = [0.1, 0.1, 0.1]
            vs[axis] = bad
            assert vox(vs=vs) == EINVAL, (bad, axis)
    assert vox(n=0, null=names) == 0                                   # no rows: a no-op
    for name in names:
        assert vox(null=(name,)) == EINVAL, name
    for off in (4, 8):
        assert vox(scratch=P + off) == EINVAL                          # the cells are int4

    def fwd(n=8, m=4, c=3, null=()):
        p = [None if k in null else P for k in ("values", "idx_sort", "start", "count", "out")]
        return lib.apn_vg_mean_fwd(n, m, c, *p, None)

    def bwd(n=8, m=4, c=3, null=()):
        p = [None if k in null else P for k in ("grad_out", "voxel_of", "count", "grad_values")]
        return lib.apn_vg_mean_bwd(n, m, c, *p, None)
    for entry, ptrs in ((fwd, ("values", "idx_sort", "start", "count", "out")),
                        (bwd, ("grad_out", "voxel_of", "count", "grad_values"))):
        assert entry(n=-1) == EINVAL and entry(n=1 << 27) == EINVAL
        assert entry(m=-1) == EINVAL and entry(m=9) == EINVAL          # m <= n
        assert entry(c=0) == EINVAL and entry(c=65537) == EINVAL
        assert entry(n=0, m=0, null=ptrs) == 0 and entry(m=0, null=ptrs) == 0
        for name in ptrs:
            assert entry(null=(name,)) == EINVAL, name
