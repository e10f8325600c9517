"""The Chamfer contract of `apn_chamfer_forward` / `apn_chamfer_backward` (include/adaptpoint_amd.h) stated in numpy
(tests/test_chamfer_cpu.py, tests/test_gpu_chamfer.py, tests/golden/make_golden_chamfer.py).

  nearest64   float64 squared distances by direct differences -- exact for the integer clouds of the exact cases -- and
              numpy's argmin, which returns the FIRST minimum: the smallest index among equally near points.
  backward32  the gradient's ordered float32 statement, written literally with np.float32 scalars (every operation
              rounds once): what the kernel must reproduce bit for bit.
  backward64  the same sum in float64, and for every output element the number of terms T and sum |term|: the error
              bar of an fp32 evaluation is (T + 2) 2^-24 sum |term| (one rounding in the difference, one in the product,
              T - 1 in the ordered sum)."""
import numpy as np

from knn_reference import dist2_64, integer_cloud  # noqa: F401  (integer_cloud: the exact cases' inputs)

TAU = 6 * 2.0 ** -24        # relative error bar of an fp32 squared distance at C = 3 (tests/test_gpu_knn.py: C + 3)


def nearest64(a, b):
    """a (B,n,3), b (B,m,3) -> (dist (B,n) float64, idx (B,n) int32): for every a the nearest b, first minimum."""
    d = dist2_64(b, a)                                            # (B, n, m): d[b,i,j] = |a_i - b_j|^2
    idx = np.argmin(d, axis=-1)
    return np.take_along_axis(d, idx[..., None], -1)[..., 0], idx.astype(np.int32)


def forward64(xyz1, xyz2):
    """The extension's forward: (dist1, dist2, idx1, idx2)."""
    d1, i1 = nearest64(xyz1, xyz2)
    d2, i2 = nearest64(xyz2, xyz1)
    return d1, d2, i1, i2


def _one_side32_many(own, oth, oidx, tidx, og, tg):
    """`_one_side32` for many small clouds: the same operations in the same order, as float32 array operations over the
    batch (numpy rounds every elementwise float32 operation once, as it does the scalars')."""
    B, no = own.shape[:2]
    two = np.float32(2)
    near = np.take_along_axis(oth, oidx.astype(np.int64)[..., None], 1)
    acc = (og * two)[..., None] * (own - near)
    for i in range(no):
        for j in range(oth.shape[1]):                             # ascending j
            hit = tidx[:, j] == i
            acc[hit, i] = acc[hit, i] - (tg[hit, j] * two)[:, None] * (oth[hit, j] - own[hit, i])
    assert acc.dtype == np.float32
    return acc


def _one_side32(own, oth, oidx, tidx, og, tg):
    B, no = own.shape[:2]
    if B >= 64:
        return _one_side32_many(own, oth, oidx, tidx, og, tg)
    out = np.empty((B, no, 3), np.float32)
    two = np.float32(2)
    for b in range(B):
        lists = [[] for _ in range(no)]
        for j, i in enumerate(tidx[b]):                           # ascending j
            lists[int(i)].append(j)
        for i in range(no):
            k = int(oidx[b, i])
            for c in range(3):
                acc = np.float32(np.float32(og[b, i] * two) * np.float32(own[b, i, c] - oth[b, k, c]))
                for j in lists[i]:
                    acc = np.float32(acc - np.float32(np.float32(tg[b, j] * two) * np.float32(oth[b, j, c] - own[b, i, c])))
                out[b, i, c] = acc
    return out


def backward32(xyz1, xyz2, idx1, idx2, grad_dist1, grad_dist2):
    """-> (grad_xyz1, grad_xyz2) float32: for every i and component
        acc = (grad_dist1[i] * 2) * (xyz1[i] - xyz2[idx1[i]])
        for j ascending with idx2[j] == i:   acc = acc - (grad_dist2[j] * 2) * (xyz2[j] - xyz1[i])
    each operation rounded to float32; grad_xyz2 with the roles swapped."""
    f = lambda a: np.ascontiguousarray(a, np.float32)
    x1, x2, g1, g2 = f(xyz1), f(xyz2), f(grad_dist1), f(grad_dist2)
    with np.errstate(over="ignore"):
        return _one_side32(x1, x2, idx1, idx2, g1, g2), _one_side32(x2, x1, idx2, idx1, g2, g1)


def _one_side64(own, oth, oidx, tidx, og, tg):
    B, no = own.shape[:2]
    first = (2 * og)[..., None] * (own - np.take_along_axis(oth, oidx.astype(np.int64)[..., None], 1))
    val, mag, cnt = first.copy(), np.abs(first), np.ones((B, no, 3), np.int64)
    for b in range(B):
        term = (2 * tg[b])[:, None] * (oth[b] - own[b][tidx[b]])  # (nt, 3): j's term for the point it chose
        np.subtract.at(val[b], tidx[b], term)
        np.add.at(mag[b], tidx[b], np.abs(term))
        np.add.at(cnt[b], tidx[b], 1)
    return val, cnt, mag


def backward64(xyz1, xyz2, idx1, idx2, grad_dist1, grad_dist2):
    """-> ((grad_xyz1, T1, S1), (grad_xyz2, T2, S2)): float64 gradients, the number of terms and sum |term| of every
    output element."""
    f = lambda a: np.asarray(a, np.float64)
    x1, x2, g1, g2 = f(xyz1), f(xyz2), f(grad_dist1), f(grad_dist2)
    return _one_side64(x1, x2, idx1, idx2, g1, g2), _one_side64(x2, x1, idx2, idx1, g2, g1)


# ---- the golden cases of tests/golden/chamfer_golden.npz: inputs are regenerated from seeds, the fixture stores outputs
GOLDEN_CASES = {                    # name: (B, n, m, seed, ignore_zeros, all-zero rows of xyz1, of xyz2)
    "clouds": (2, 128, 96, 9101, False, (), ()),
    "patches": (6, 32, 32, 9102, False, (), ()),
    "padded": (1, 80, 70, 9103, True, (3, 17, 18, 79), (0, 40, 41)),
}
LOSSES = ("l1", "l2", "l2_split")   # ChamferDistanceL1, ChamferDistanceL2, the sum of ChamferDistanceL2_split's pair


def golden_inputs(name):
    """-> (xyz1 (B,n,3), xyz2 (B,m,3)) float32 seeded normal clouds, (ignore_zeros, keep1, keep2): the rows the
    `ignore_zeros` filter keeps (all of them where it does not apply)."""
    B, n, m, seed, ignore, zero1, zero2 = GOLDEN_CASES[name]
    rng = np.random.default_rng(seed)
    xyz1 = rng.standard_normal((B, n, 3)).astype(np.float32)
    xyz2 = rng.standard_normal((B, m, 3)).astype(np.float32)
    xyz1[:, list(zero1)] = 0
    xyz2[:, list(zero2)] = 0
    keep1 = np.setdiff1d(np.arange(n), zero1) if ignore else np.arange(n)
    keep2 = np.setdiff1d(np.arange(m), zero2) if ignore else np.arange(m)
    return xyz1, xyz2, (ignore, keep1, keep2)


def loss_coefficients(loss, dist1, dist2):
    """d loss / d dist1, d loss / d dist2 in float64 for the three losses (dist: float64 squared distances)."""
    n, m = dist1.shape[1], dist2.shape[1]
    B = dist1.shape[0]
    if loss == "l1":
        return 1 / (4 * B * n * np.sqrt(dist1)), 1 / (4 * B * m * np.sqrt(dist2))
    return np.full_like(dist1, 1 / (B * n)), np.full_like(dist2, 1 / (B * m))
