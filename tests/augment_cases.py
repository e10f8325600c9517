"""The problems of tests/test_gpu_augment_cases.py and tests/test_augment_cases_cpu.py for the four kernels of
csrc/augment.hip, in numpy (float64 arrays holding float32 values, so that a cast to float32 loses nothing).

  switch_table()   all 64 keep x axes combinations (axes code 0 is one only a caller can pass)
  exact_deform()   E1 / E2: clouds whose every intermediate is exact in float32 (and float64), with planted farthest points
  DEFORM_TABLE     the random deformation cases: N x M x B x sigma x axis codes x mask kind, crossed, not the full product
  deform_case()    the inputs of one row

The conditions every random case must meet (tests/test_augment_cases_cpu.py asserts them for every row and for the fixture):
  1. the float64 gap between the largest and the second-largest centred radius is >= 1e-4 of the largest -- far above any
     bar on z, so float32 cannot pick another farthest point.  N = 2 is exempt: two points are equidistant from their mean
     by construction, either choice gives the same r and the same gradient (e flips sign together with the point it is
     credited to), and the GPU test takes the index the forward stored after checking that it is a farthest point;
  2. a hard mask is `draw < 0.8` of a uniform draw that keeps >= 1e-6 from 0.8: no mask bit depends on a rounding;
  3. the smallest weight sum of any point is >= 1e-30.
"""
import numpy as np

RANGES = {"project": (10.0, 3.0, 0.25), "wide": (180.0, 5.0, 1.0)}
GAP, MASK_CLEAR, WSUM_MIN = 1e-4, 1e-6, 1e-30


def f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def axis_bits(code):
    """1..7 (0 for a caller's "no axis") -> its three bits, least significant first (generator_component4_15.py:308-310)."""
    code = np.asarray(code)
    return ((code[..., None] >> np.arange(3)) & 1).astype(np.float64)


def switch_table():
    """keep (64,3), axes (64,3): every keep in {0,1}^3 with every axes code 0..7."""
    keep = np.array([[(k >> i) & 1 for i in range(3)] for k in range(8) for _ in range(8)], np.float64)
    axes = axis_bits(np.array([a for _ in range(8) for a in range(8)]))
    return keep, axes


def unit_ball_cloud(rng, B, N):
    d = rng.normal(size=(B, N, 3))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    return f32(d * rng.uniform(0.0, 1.0, (B, N, 1)) ** (1.0 / 3.0))


def masks(rng, B, N, kind):
    """-> mask (B,N) or None, the uniform draw behind a hard one (else None)."""
    if kind == "none":
        return None, None
    u = rng.uniform(0.0, 1.0, (B, N))
    if kind == "hard":
        return (u < 0.8).astype(np.float64), u
    return f32(0.05 + 0.9 * u), None


# N, M, B, sigma, axis codes (one per cloud), mask kind, seed
DEFORM_TABLE = [
    (2, 1, 1, 0.5, (7,), "soft", 1),
    (2, 2, 3, 0.2, (1, 2, 4), "none", 2),
    (63, 3, 3, 0.5, (3, 5, 6), "hard", 3),
    (64, 8, 1, 0.2, (7,), "soft", 4),
    (65, 4, 3, 0.2, (1, 6, 3), "hard", 5),
    (255, 2, 1, 0.5, (2,), "soft", 6),
    (256, 1, 3, 0.2, (4, 5, 7), "hard", 7),
    (257, 8, 3, 0.5, (6, 1, 2), "soft", 8),
    (777, 3, 1, 0.2, (5,), "hard", 9),
    (4095, 4, 3, 0.5, (7, 4, 3), "soft", 10),
    (4096, 8, 1, 0.2, (6,), "hard", 11),
    (4096, 1, 3, 0.5, (1, 2, 5), "none", 12),
    (4096, 2, 1, 0.5, (3,), "soft", 13),
]
DEFORM_IDS = [f"N{r[0]}-M{r[1]}-B{r[2]}-s{r[3]}-{r[5]}" for r in DEFORM_TABLE]


def deform_case(row):
    """One row of DEFORM_TABLE -> dict of float64 arrays: x, anchors (points of the cloud), lin, off, axes (B,3), mask,
    mask_draw, gout, and sigma."""
    N, M, B, sigma, codes, kind, seed = row
    rng = np.random.default_rng(1000 + seed)
    x = unit_ball_cloud(rng, B, N)
    pick = np.stack([rng.permutation(N)[:M] for _ in range(B)])
    anchors = np.take_along_axis(x, pick[..., None].repeat(3, -1), 1)
    lin = f32(np.eye(3) + 0.3 * rng.normal(size=(B, M, 3, 3)))
    off = f32(0.2 * rng.normal(size=(B, M, 3)))
    mask, draw = masks(rng, B, N, kind)
    return dict(x=x, anchors=anchors, lin=lin, off=off, axes=axis_bits(np.array(codes)), mask=mask, mask_draw=draw,
                gout=f32(rng.normal(size=(B, N, 3))), sigma=sigma)


def exact_deform(N, M, planted, seed, lin_spread=True):
    """E1 / E2.  The kernel axis is x alone and every point and anchor has x = 0, so every weight is exp(-0) = 1 and the
    normalised weight 1 / M (M a power of two).  The other coordinates are integers in [-1, 1], not both 0, in +- pairs (the
    cloud's mean is 0), `planted` maps an index to a point (0, +-4, 0) or (0, 0, +-4); the caller balances what it plants.  The
    matrices are integer with mean diag(., 2, 2) (rows y, z), the offsets multiples of 1/4: z = x . mean(A) + const with
    every partial result a small multiple of 1 / (4 M), its mean exact (N a power of two), the planted points at centred
    radius exactly 8 = 2^3 and every other point within 4 of the centre.
    -> dict: x (1,N,3), anchors, lin, off, axes, z, mu, r, kfar (the lowest planted index), all exact."""
    assert N & (N - 1) == 0 and M & (M - 1) == 0
    rng = np.random.default_rng(seed)
    free = [i for i in range(N) if i not in planted]
    assert len(free) % 2 == 0
    x = np.zeros((1, N, 3))
    grid = np.array([(y, z) for y in (-1.0, 0.0, 1.0) for z in (-1.0, 0.0, 1.0) if (y, z) != (0.0, 0.0)])
    half = grid[rng.integers(0, 8, len(free) // 2)]                 # no point at the centre: |z - mu| has no derivative there
    order = rng.permutation(len(free))
    for j, pt in enumerate(half):
        x[0, free[order[2 * j]], 1:] = pt
        x[0, free[order[2 * j + 1]], 1:] = -pt
    for i, pt in planted.items():
        x[0, i] = pt
    assert np.all(x.sum(1) == 0)
    anchors = x[:, [free[i] for i in range(M)]].copy()
    lin = np.zeros((1, M, 3, 3))
    lin[:] = np.diag([1.0, 2.0, 2.0])
    lin[0, :, 0] = rng.integers(-3, 4, (M, 3))                      # row x multiplies the zero x-difference
    if lin_spread and M > 1:
        d = rng.integers(-2, 3, (M // 2, 2, 3)).astype(np.float64)  # +d on one anchor, -d on its partner: the mean stays
        lin[0, 0::2, 1:] += d
        lin[0, 1::2, 1:] -= d
    off = rng.integers(-8, 9, (1, M, 3)) / 4.0
    axes = np.array([[1.0, 0.0, 0.0]])
    v = np.einsum("bmnr,bmrc->bmnc", x[:, None] - anchors[:, :, None], lin) + (off + anchors)[:, :, None]
    z = v.sum(1) / M
    mu = z.sum(1) / N
    rad = np.sqrt(((z - mu[:, None]) ** 2).sum(-1))
    assert np.array_equal(z.astype(np.float32).astype(np.float64), z) and np.array_equal(f32(mu), mu)
    return dict(x=x, anchors=anchors, lin=lin, off=off, axes=axes, z=z, mu=mu, r=rad.max(1), kfar=rad.argmax(1), rad=rad)


PLANT_Y, PLANT_Z = (0.0, 4.0, 0.0), (0.0, 0.0, 4.0)


def two_ties(a=5, b=70, balance=(60, 61, 62, 63)):
    """two farthest points (0,4,0) and (0,0,4), in different waves of the 256-thread block for the defaults; four points
    (0,-1,-1) keep the cloud's mean at 0.  Not an antipodal pair: with uniform weights the gradients with respect to the
    matrices under the two tie rules coincide when the tied points sum to twice the mean."""
    p = {a: PLANT_Y, b: PLANT_Z}
    p.update({i: (0.0, -1.0, -1.0) for i in balance})
    return p


def three_ties(a=5, b=70, c=300, balance=(301, 302, 303)):
    """three farthest points (0,4,0), (0,-4,0), (0,0,4); (0,0,-1) twice and (0,0,-2) keep the cloud's mean at 0"""
    p = {a: PLANT_Y, b: tuple(-v for v in PLANT_Y), c: PLANT_Z}
    p.update({balance[0]: (0.0, 0.0, -1.0), balance[1]: (0.0, 0.0, -1.0), balance[2]: (0.0, 0.0, -2.0)})
    return p
