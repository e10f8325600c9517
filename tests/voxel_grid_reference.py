"""The numpy statement of the voxel grid's contract (include/adaptpoint_amd.h, apn_vg_*; adaptpoint_amd/voxel_grid.py)
and the seeded scene of its golden (tests/golden/make_golden_voxelize.py).

    cell(i) = floor((double)coord[i] / (double)voxel_size)  per axis;  a voxel = rows with equal (cloud, cell);
    voxels numbered by their smallest member row;  idx_sort = the stable argsort of voxel_of;
    mean = sequential float32 adds in ascending row from the first term, then float32(float64(s) / float64(count)).
"""
import numpy as np

VOXEL = 0.04
SIZES = (1100, 700, 1300)
BOX = 0.5


def offsets(sizes):
    return np.cumsum(np.asarray(sizes, np.int64)).astype(np.int32)


def golden_scene(seed=2024):
    """-> coord (3100,3) float32, offset (3) int32: three clouds in a 0.5 box, each shifted to min = 0 (the reference's
    hashes need that); every third point of a cloud (rows 0, 3, 6, ... of the cloud) sits exactly on cell faces, at
    integer multiples of float32(0.04) on every axis: the points a float32 division would put into other cells."""
    rng = np.random.RandomState(seed)
    step = np.float32(VOXEL)
    clouds = []
    for size in SIZES:
        pts = rng.uniform(0.0, BOX, (size, 3)).astype(np.float32)
        faces = rng.randint(0, int(BOX / VOXEL) + 1, (size, 3)).astype(np.float32) * step      # one float32 product
        pts[::3] = faces[::3]
        pts[0] = 0.0                                             # min = 0 already: the shift below changes no bit
        pts -= pts.min(0)
        clouds.append(pts)
    return np.concatenate(clouds), offsets(SIZES)


def cells(coord, voxel_size):
    """(n,3) float64 cells (not yet integers: the caller checks the range) by IEEE double division."""
    vs = np.broadcast_to(np.asarray(voxel_size, np.float64).reshape(-1), (3,))
    with np.errstate(all="ignore"):
        return np.floor(coord.astype(np.float64) / vs)


def clouds_of(n, offset):
    """(n) the cloud of every row: the first c with i < offset[c]; rows at or past the last end belong to the last."""
    b = len(offset)
    return np.minimum(np.searchsorted(np.asarray(offset, np.int64), np.arange(n), side="right"), b - 1)


def statement(coord, voxel_size, offset=None):
    """-> dict of every field of the contract (int32 arrays, Python ints m / count_max / bad)."""
    n = coord.shape[0]
    offset = np.asarray([n], np.int32) if offset is None else np.asarray(offset, np.int32)
    b = len(offset)
    q = cells(coord, voxel_size)
    ok = np.isfinite(coord).all(1) & (q >= -2.0 ** 31).all(1) & (q <= 2.0 ** 31 - 1).all(1)
    bad = int((~ok).sum())
    key = np.zeros((n, 4), np.int64)
    key[ok, :3] = q[ok].astype(np.int64)
    key[:, 3] = clouds_of(n, offset)
    key[~ok] = (0, 0, 0, -1)
    first = {}
    rep = np.empty(n, np.int64)
    for i in range(n):                                           # the smallest row of i's voxel
        rep[i] = first.setdefault(tuple(key[i]), i)
    is_first = rep == np.arange(n)
    dense = np.cumsum(is_first) - is_first                       # exclusive
    voxel_of = dense[rep] if n else np.zeros(0, np.int64)
    m = int(is_first.sum())
    count = np.bincount(voxel_of, minlength=m)
    start = np.cumsum(count) - count
    idx_sort = np.argsort(voxel_of, kind="stable")
    new_offset = np.empty(b, np.int64)
    for c in range(b):
        end = int(offset[c])
        new_offset[c] = m if (c == b - 1 or end >= n) else int(is_first[:max(end, 0)].sum())
    i32 = lambda a: np.asarray(a, np.int64).astype(np.int32)
    return dict(voxel_of=i32(voxel_of), count=i32(count), start=i32(start), idx_sort=i32(idx_sort),
                new_offset=i32(new_offset), first=i32(idx_sort[start]) if m else i32([]), m=m,
                count_max=int(count.max()) if m else 0, bad=bad)


def partition_labels(voxel_idx_sorted, idx_sort):
    """From a (idx_sort, voxel_idx) pair in the reference's form (voxel_idx[j] = the voxel of idx_sort[j]): every row's
    smallest same-voxel row -- a labelling that does not depend on how the voxels are numbered or ordered."""
    n = len(idx_sort)
    label = np.empty(n, np.int64)
    label[idx_sort] = voxel_idx_sorted
    smallest = np.full(int(label.max()) + 1 if n else 0, n, np.int64)
    np.minimum.at(smallest, label, np.arange(n))
    return smallest[label]


def mean(values, st):
    """(m,c) float32: per voxel the sequential float32 sum in ascending row, one correctly rounded division."""
    m, c = st["m"], values.shape[1]
    out = np.zeros((m, c), np.float32)
    for v in range(m):
        rows = st["idx_sort"][st["start"][v]:st["start"][v] + st["count"][v]]
        s = values[rows[0]].astype(np.float32).copy()
        for r in rows[1:]:
            s = (s + values[r]).astype(np.float32)
        out[v] = (s.astype(np.float64) / np.float64(st["count"][v])).astype(np.float32)
    return out


def mean_grad(grad_out, st):
    """(n,c) float32: grad_out[voxel_of[i]] / count, correctly rounded."""
    v = st["voxel_of"]
    return (grad_out[v].astype(np.float64) / st["count"][v].astype(np.float64)[:, None]).astype(np.float32)
