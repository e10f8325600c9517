"""The earth mover's distance contract of csrc/emd.hip (include/adaptpoint_amd.h) stated in numpy
(tests/test_emd_cpu.py, tests/test_gpu_emd.py, tests/golden/make_golden_emd.py).

  ratios64 / match64 / cost64 / grad64   the statement in float64, with direct differences and np.exp.
  ratios32 / match32 / cost32 / grad32   the same statements with every operation rounded to float32: sums are
        sequential (np.cumsum, ascending index), the distance is the kernel's fma form, and exp is exp2 of the
        fp32-rounded product (level * d) * log2(e).  It is NOT a bit-for-bit model of the kernel (whose split form sums a
        row in four runs, and whose exp2 is the hardware's): its distance from the float64 statement, E32, measures how
        far apart two honest evaluations of this mildly ill-conditioned iteration lie, and is the yardstick of the GPU
        tests' bars.

`match` is (B,m,n): match[b,l,k] is the weight between xyz2[b,l] and xyz1[b,k], as in the reference."""
import numpy as np

LEVELS = tuple([-(4.0 ** j) for j in range(7, -2, -1)] + [0.0])      # level index 0 .. 9: the reference's j = 7 .. -2
EPS = 1e-9
LOG2E32 = np.float32(1.44269504088896340736)

# name -> (B, n, m, seed): uniform clouds in [-1, 1]^3
GOLDEN_CASES = {
    "equal": (2, 64, 64, 9101),
    "double": (2, 130, 65, 9102),
    "triple": (2, 300, 100, 9103),
    "tiny": (2, 7, 3, 9104),
    "split": (2, 140, 129, 9105),          # just above the one-launch form's limit of 128
}


def uniform_clouds(B, n, m, seed):
    rng = np.random.default_rng(seed)
    return (rng.uniform(-1, 1, (B, n, 3)).astype(np.float32), rng.uniform(-1, 1, (B, m, 3)).astype(np.float32))


def golden_inputs(name):
    B, n, m, seed = GOLDEN_CASES[name]
    return uniform_clouds(B, n, m, seed)


def multipliers(n, m):
    """(multiL, multiR) by integer division, as the reference's kernel computes them."""
    return (1, n // m) if n >= m else (m // n, 1)


def _sum(a, axis):
    """The sequential sum along `axis` in a's own precision."""
    return np.take(np.cumsum(a, axis=axis, dtype=a.dtype), -1, axis=axis)


def dist(xyz1, xyz2, f):
    """d (B,m,n): d[b,l,k] = |xyz2[b,l] - xyz1[b,k]|^2 in precision f; float32: fma(tz, tz, fma(ty, ty, tx * tx))."""
    t = xyz2.astype(f)[:, :, None, :] - xyz1.astype(f)[:, None, :, :]
    if f is np.float64:
        return (t * t).sum(-1)
    t = t.astype(np.float64)                                # products of two floats are exact in float64
    inner = (t[..., 1] * t[..., 1] + (t[..., 0] * t[..., 0]).astype(np.float32)).astype(np.float32)
    return (t[..., 2] * t[..., 2] + inner).astype(np.float32)


def _exp(level, d, f):
    if f is np.float64:
        return np.exp(level * d)
    with np.errstate(under="ignore"):
        return np.exp2(np.float32(level) * (d * LOG2E32))       # a level is a power of two or 0: the product is exact


def _ratios(xyz1, xyz2, f):
    B, n, m = xyz1.shape[0], xyz1.shape[1], xyz2.shape[1]
    d = dist(xyz1, xyz2, f)
    multi_l, multi_r = multipliers(n, m)
    rem_l, rem_r = np.full((B, n), multi_l, f), np.full((B, m), multi_r, f)
    eps, one, zero = f(EPS), f(1), f(0)
    ratio_l, ratio_r = np.empty((B, len(LEVELS), n), f), np.empty((B, len(LEVELS), m), f)
    for q, level in enumerate(LEVELS):
        e = _exp(level, d, f)
        rat_l = rem_l / (eps + _sum(e * rem_r[:, :, None], 1))
        sumr = _sum(e * rat_l[:, None, :], 2) * rem_r
        rat_r = np.minimum(rem_r / (sumr + eps), one) * rem_r
        rem_r = np.maximum(zero, rem_r - sumr)
        rem_l = np.maximum(zero, rem_l - _sum((e * rat_l[:, None, :]) * rat_r[:, :, None], 1))
        ratio_l[:, q], ratio_r[:, q] = rat_l, rat_r
    assert ratio_l.dtype == f and ratio_r.dtype == f
    return ratio_l, ratio_r


def _match(xyz1, xyz2, ratio_l, ratio_r, f):
    d = dist(xyz1, xyz2, f)
    match = np.zeros(d.shape, f)
    for q, level in enumerate(LEVELS):
        match = match + (_exp(level, d, f) * ratio_l[:, q, None, :].astype(f)) * ratio_r[:, q, :, None].astype(f)
    assert match.dtype == f
    return match


def _cost(xyz1, xyz2, match, f):
    B = xyz1.shape[0]
    return _sum((dist(xyz1, xyz2, f) * match.astype(f)).reshape(B, -1), 1)


def _grad(grad_cost, xyz1, xyz2, match, f):
    t = xyz1.astype(f)[:, None, :, :] - xyz2.astype(f)[:, :, None, :]         # (B,m,n,3): xyz1_k - xyz2_l
    w = (match.astype(f) * f(2))[..., None]
    g = grad_cost.astype(f)[:, None, None]
    return _sum(t * w, 1) * g, _sum(-t * w, 2) * g


def ratios64(xyz1, xyz2):
    return _ratios(xyz1, xyz2, np.float64)


def ratios32(xyz1, xyz2):
    return _ratios(xyz1, xyz2, np.float32)


def match64(xyz1, xyz2, ratios=None):
    return _match(xyz1, xyz2, *(ratios or ratios64(xyz1, xyz2)), np.float64)


def match32(xyz1, xyz2, ratios=None):
    return _match(xyz1, xyz2, *(ratios or ratios32(xyz1, xyz2)), np.float32)


def cost64(xyz1, xyz2, match):
    return _cost(xyz1, xyz2, match, np.float64)


def cost32(xyz1, xyz2, match):
    return _cost(xyz1, xyz2, match, np.float32)


def grad64(grad_cost, xyz1, xyz2, match):
    return _grad(grad_cost, xyz1, xyz2, match, np.float64)


def grad32(grad_cost, xyz1, xyz2, match):
    return _grad(grad_cost, xyz1, xyz2, match, np.float32)


def lattice_cloud(B, n, seed):
    """(B,n,3) float32: n DISTINCT integer points per cloud, of {-4..4}^3 up to 729 points and of {-8..8}^3 beyond."""
    side = 9 if n <= 729 else 17
    assert n <= side ** 3
    rng = np.random.default_rng(seed)
    out = np.empty((B, n, 3), np.float32)
    for b in range(B):
        cells = rng.permutation(side ** 3)[:n]
        out[b] = np.stack([cells // (side * side), (cells // side) % side, cells % side], -1) - side // 2
    return out


def permuted(xyz, seed):
    """(xyz with each cloud's points permuted, perm (B,n)): result[b,l] = xyz[b,perm[b,l]]."""
    rng = np.random.default_rng(seed)
    perm = np.stack([rng.permutation(xyz.shape[1]) for _ in range(xyz.shape[0])])
    return np.take_along_axis(xyz, perm[..., None], 1), perm
