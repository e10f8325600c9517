"""GPU suite: the device voxel grid (csrc/voxel_grid.hip through adaptpoint_amd/voxel_grid.py) against the numpy statement
of its contract (tests/voxel_grid_reference.py) and the reference's own `voxelize` on the golden scene
(tests/golden/voxelize_golden.npz).

Every comparison is exact: the outputs are integers, or float32 sums in a stated order with one correctly rounded
division.  Shapes are the smallest at which each kernel can go wrong: n around one wave (63 | 64 | 65), more than one scan
tile (2048) and more than one sort tile (1024) in the golden scene (3100 rows), two radix passes (n > 256) and three
(n > 65536: the 40^3 lattice, 70 400 rows), table probing among 64 000 distinct cells, and 20 000 rows in ONE voxel: the
case that a design with work non-linear in a voxel's population turns into minutes.
"""
import functools
import os

import numpy as np
import pytest
import torch

import voxel_grid_reference as VR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("voxel_of", "count", "start", "idx_sort", "new_offset", "first")


@functools.lru_cache(maxsize=None)
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "voxelize_golden.npz"))


@functools.lru_cache(maxsize=None)
def scene():
    coord, offset = VR.golden_scene()
    return coord, offset, VR.statement(coord, VR.VOXEL, offset)


def run(dev, coord, voxel_size, offset=None):
    from adaptpoint_amd.voxel_grid import voxel_grid
    off = None if offset is None else torch.from_numpy(np.asarray(offset, np.int32)).to(dev)
    return voxel_grid(torch.from_numpy(coord).to(dev), voxel_size, off)


def fields(grid):
    out = {k: getattr(grid, k).cpu().numpy() for k in FIELDS}
    out.update(m=grid.m, count_max=grid.count_max)
    return out


def assert_equals_statement(grid, st):
    got = fields(grid)
    assert got["m"] == st["m"] and got["count_max"] == st["count_max"]
    for k in FIELDS:
        assert got[k].dtype == np.int32 and np.array_equal(got[k], st[k]), k


def lattice(side, seed):
    """side^3 cell centres at voxel 1 in a seeded order, float32."""
    g = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float32) + 0.5
    return g[np.random.RandomState(seed).permutation(len(g))]


def test_golden_scene_stacked(dev):
    coord, offset, st = scene()
    grid = run(dev, coord, VR.VOXEL, offset)
    got = fields(grid)
    labels = got["first"].astype(np.int64)[got["voxel_of"]]
    ends, lo = [], 0
    for c, hi in enumerate(offset.tolist()):
        assert np.array_equal(labels[lo:hi] - lo, gold()[f"label_{c}"]), c                   # the reference's partition
        mine = got["count"][(got["first"] >= lo) & (got["first"] < hi)]
        assert np.array_equal(np.sort(mine), gold()[f"counts_{c}"]), c                       # ... and its counts
        ends.append(len(gold()[f"counts_{c}"]))
        lo = hi
    assert np.array_equal(got["new_offset"], np.cumsum(ends))
    assert_equals_statement(grid, st)


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_edge_sizes(dev, n):
    coord = np.random.RandomState(n).uniform(-1, 1, (n, 3)).astype(np.float32)
    assert_equals_statement(run(dev, coord, 0.5), VR.statement(coord, 0.5))


def test_no_rows(dev):
    grid = run(dev, np.zeros((0, 3), np.float32), 0.1, [0, 0])
    assert grid.m == 0 and grid.count_max == 0 and grid.new_offset.tolist() == [0, 0]
    assert all(getattr(grid, k).numel() == 0 for k in ("voxel_of", "count", "start", "idx_sort", "first"))


def test_empty_middle_cloud_negative_coordinates_anisotropic_size(dev):
    coord = np.random.RandomState(5).uniform(-2, 2, (700, 3)).astype(np.float32)
    offset, vs = [300, 300, 700], (0.5, 0.25, 1.0)
    st = VR.statement(coord, vs, offset)
    assert st["new_offset"][0] == st["new_offset"][1] < st["m"] and (VR.cells(coord, vs) < 0).any()
    assert_equals_statement(run(dev, coord, vs, offset), st)


def test_float64_input(dev):
    rng = np.random.RandomState(6)
    coord = rng.uniform(-1, 1, (500, 3))
    coord[::2] = rng.randint(-8, 8, (250, 3)) * 0.1                 # on or beside faces: only a double division is right
    st = VR.statement(coord, 0.1)
    assert not np.array_equal(st["voxel_of"], VR.statement(coord.astype(np.float32), 0.1)["voxel_of"])
    assert_equals_statement(run(dev, coord, 0.1), st)


def test_clouds_with_the_same_coordinates_are_not_merged(dev):
    one = np.random.RandomState(7).uniform(0, 1, (150, 3)).astype(np.float32)
    coord, offset = np.concatenate([one] * 3), [150, 300, 450]
    st, alone = VR.statement(coord, 0.2, offset), VR.statement(one, 0.2)
    assert st["m"] == 3 * alone["m"]
    grid = run(dev, coord, 0.2, offset)
    assert_equals_statement(grid, st)
    vo = grid.voxel_of.cpu().numpy()
    for c in range(3):
        assert np.array_equal(vo[150 * c:150 * (c + 1)], alone["voxel_of"] + c * alone["m"])
    assert grid.new_offset.tolist() == [alone["m"], 2 * alone["m"], 3 * alone["m"]]


def test_many_distinct_cells(dev):
    """A 40^3 lattice, one point per cell, every tenth point once more: 64 000 voxels among 70 400 rows."""
    g = lattice(40, 8)
    coord = np.concatenate([g, g[::10]])[np.random.RandomState(9).permutation(70400)]
    grid = run(dev, coord, 1.0)
    # the statement in closed form (the dict-based one is slow at this size): a voxel is a lattice cell
    cell = np.floor(coord.astype(np.float64)).astype(np.int64)
    lin = (cell[:, 0] * 40 + cell[:, 1]) * 40 + cell[:, 2]
    _, first, inverse = np.unique(lin, return_index=True, return_inverse=True)
    rank = np.empty(len(first), np.int64)
    rank[np.argsort(first)] = np.arange(len(first))
    voxel_of = rank[inverse]
    count = np.bincount(voxel_of)
    assert grid.m == 64000 and grid.count_max == 2
    assert np.array_equal(grid.voxel_of.cpu().numpy(), voxel_of)
    assert np.array_equal(grid.count.cpu().numpy(), count)
    assert np.array_equal(grid.start.cpu().numpy(), np.cumsum(count) - count)
    assert np.array_equal(grid.idx_sort.cpu().numpy(), np.argsort(voxel_of, kind="stable"))
    assert np.array_equal(grid.first.cpu().numpy(), np.sort(first)) and grid.new_offset.tolist() == [64000]


def test_one_voxel(dev):
    coord = np.random.RandomState(10).uniform(0.0, 1.0, (20000, 3)).astype(np.float32)
    grid = run(dev, coord, 4.0)
    assert grid.m == 1 and grid.count_max == 20000 and grid.count.tolist() == [20000] and grid.start.tolist() == [0]
    assert not grid.voxel_of.any() and torch.equal(grid.idx_sort, torch.arange(20000, dtype=torch.int32, device=dev))
    vals = torch.from_numpy(coord).to(dev)
    st = dict(m=1, idx_sort=np.arange(20000), start=np.array([0]), count=np.array([20000]))
    assert np.array_equal(grid.mean(vals).cpu().numpy(), VR.mean(coord, st))


def test_permuted_input_and_two_runs(dev):
    coord, offset, st = scene()
    lo, hi = int(offset[0]), int(offset[1])
    cloud = coord[lo:hi]
    perm = np.random.RandomState(11).permutation(len(cloud))
    a, b, a2 = run(dev, cloud, VR.VOXEL), run(dev, cloud[perm], VR.VOXEL), run(dev, cloud, VR.VOXEL)
    for k in FIELDS:
        assert torch.equal(getattr(a, k), getattr(a2, k)), k                                  # two runs, the same bits
    fa, fb = fields(a), fields(b)
    sets = lambda f, rows: sorted(tuple(sorted(rows[f["idx_sort"][s:s + c]].tolist())) for s, c in zip(f["start"], f["count"]))
    assert sets(fa, np.arange(len(cloud))) == sets(fb, perm)                                  # the same voxels as sets
    assert_equals_statement(b, VR.statement(cloud[perm], VR.VOXEL))


def test_parts_cover_every_row(dev):
    coord, offset, st = scene()
    grid = run(dev, coord, VR.VOXEL, offset)
    seen = np.zeros(len(coord), bool)
    for i in range(grid.count_max):
        part = grid.part(i).cpu().numpy()
        assert part.shape == (grid.m,) and np.array_equal(st["voxel_of"][part], np.arange(grid.m))   # one row per voxel
        seen[part] = True
    assert seen.all()
    draws = torch.arange(grid.m, device=dev) * 7
    pick = grid.pick(draws).cpu().numpy()
    assert np.array_equal(pick, st["idx_sort"][st["start"] + (np.arange(grid.m) * 7) % st["count"]])


def test_voxelize_mode0_consumes_the_host_stream_like_the_reference(dev):
    from adaptpoint_amd.voxel_grid import voxelize
    coord, offset, _ = scene()
    lo = 0
    for c, hi in enumerate(offset.tolist()):
        cloud = coord[lo:hi]
        st = VR.statement(cloud, VR.VOXEL)
        np.random.seed(int(gold()["seed"]) + c)
        picked = voxelize(torch.from_numpy(cloud).to(dev), VR.VOXEL, mode=0)
        assert np.random.randint(0, 2 ** 31 - 1) == int(gold()[f"next_{c}"]), c              # the next host draw
        assert picked.dtype == torch.int64 and picked.shape == (st["m"],)
        assert np.array_equal(st["voxel_of"][picked.cpu().numpy()], np.arange(st["m"]))      # each row in its own voxel
        lo = hi


def test_voxelize_mode1_and_device_draws(dev):
    from adaptpoint_amd.voxel_grid import voxelize
    coord, offset, st = scene()
    pos, off = torch.from_numpy(coord).to(dev), torch.from_numpy(offset).to(dev)
    idx_sort, voxel_idx, count = voxelize(pos, VR.VOXEL, hash_type='ravel', mode=1, offset=off)
    assert idx_sort.dtype == voxel_idx.dtype == count.dtype == torch.int64
    assert np.array_equal(idx_sort.cpu().numpy(), st["idx_sort"]) and np.array_equal(count.cpu().numpy(), st["count"])
    assert np.array_equal(voxel_idx.cpu().numpy(), st["voxel_of"][st["idx_sort"]])           # the reference's meaning
    for draws in ('device', torch.zeros(st["m"], dtype=torch.int64, device=dev)):
        picked = voxelize(pos, VR.VOXEL, offset=off, draws=draws).cpu().numpy()
        assert np.array_equal(st["voxel_of"][picked], np.arange(st["m"]))
    assert np.array_equal(picked, st["first"])                                               # draws of 0: the first rows


@pytest.mark.parametrize("c", [1, 3, 64, 65])
def test_mean_equals_the_sequential_float32_statement(dev, c):
    coord, offset, st = scene()
    grid = run(dev, coord, 0.12, offset)                          # counts up to a few dozen: the order of the adds shows
    st = VR.statement(coord, 0.12, offset)
    assert st["count_max"] >= 16
    vals = np.random.RandomState(c).standard_normal((len(coord), c)).astype(np.float32)
    got = grid.mean(torch.from_numpy(vals).to(dev)).cpu().numpy()
    assert got.dtype == np.float32 and np.array_equal(got, VR.mean(vals, st))


def test_mean_of_integer_features_and_barycentres(dev):
    coord, offset, _ = scene()
    st = VR.statement(coord, 0.12, offset)
    grid = run(dev, coord, 0.12, offset)
    ints = np.random.RandomState(12).randint(-50, 50, (len(coord), 5)).astype(np.float32)
    sums = np.zeros((st["m"], 5))
    np.add.at(sums, st["voxel_of"], ints.astype(np.float64))      # exact: small integers
    want = (sums / st["count"][:, None]).astype(np.float32)
    assert np.array_equal(grid.mean(torch.from_numpy(ints).to(dev)).cpu().numpy(), want)
    bary = grid.mean(torch.from_numpy(coord).to(dev)).cpu().numpy()
    assert np.array_equal(bary, VR.mean(coord, st))
    assert np.array_equal(np.floor(bary.astype(np.float64) / 0.12), VR.cells(coord, 0.12)[st["first"]])   # inside its cell


def test_mean_backward_is_the_exact_gather(dev):
    # voxels with 1, 2 and 4 members (divisions by powers of two: exact), rows interleaved
    cellx = np.array([0, 1, 2, 2, 1, 2, 2], np.float32)
    coord = np.stack([cellx + 0.5, np.full(7, 0.5, np.float32), np.full(7, 0.5, np.float32)], 1)
    grid = run(dev, coord, 1.0)
    assert grid.count.tolist() == [1, 2, 4] and grid.voxel_of.tolist() == [0, 1, 2, 2, 1, 2, 2]
    vals = torch.randn(7, 3, device=dev, requires_grad=True)
    g = torch.from_numpy(np.random.RandomState(13).standard_normal((3, 3)).astype(np.float32)).to(dev)
    (grid.mean(vals) * g).sum().backward()
    st = VR.statement(coord, 1.0)
    assert np.array_equal(vals.grad.cpu().numpy(), VR.mean_grad(g.cpu().numpy(), st))
    assert torch.equal(vals.grad, g[grid.voxel_of.long()] / grid.count[grid.voxel_of.long()].float().unsqueeze(1))


@pytest.mark.parametrize("value", [1e12, float("nan"), float("inf")])
def test_bad_input_raises(dev, value):
    coord = np.random.RandomState(14).uniform(0, 1, (100, 3)).astype(np.float32)
    coord[37, 1] = value
    with pytest.raises(ValueError, match="1 rows"):
        run(dev, coord, 0.04)
    from adaptpoint_amd.voxel_grid import voxel_grid
    with pytest.raises(ValueError):
        voxel_grid(torch.zeros(4, 3, device=dev), 0.0)
    with pytest.raises(ValueError):
        voxel_grid(torch.zeros(4, 3), 0.1)                        # not on the device: there is no CPU path
