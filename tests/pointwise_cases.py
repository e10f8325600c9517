"""Exact cases for the kernels of csrc/pointwise.hip around the contraction body: the tile statistics of the forward
product, BatchNorm + ReLU (apn_pw_bn_act, training and eval), BatchNorm's gradient on both of its routes
(apn_pw_bn_act_grad), the convolution + max pair (apn_pw_conv_max_forward / _backward) and the operand set-up of the three
convolution entries.  This module holds the case tables, the input builders and the numpy / float64 statement of every
operation; tests/test_pointwise_cases_cpu.py checks that they keep their promises, tests/test_gpu_pointwise_cases.py runs
the kernels against them.

The exactness argument: inputs are small integers and every scale a power of two (times a small integer), so every float32
sum, product and fma in the kernels is exact in any order, and a small integer (or a power of two) fits ONE bf16 plane: the
results must EQUAL the statements at precision 2 and 3 alike.  `check_*` functions assert the preconditions of that
argument on a case's own values.  Where exactness cannot hold (the M2 share of a tile, the folded variance, the training-mode
gradient over a count that is no power of two) the bar is derived where it is used.
"""
import numpy as np

F64 = np.float64
TILE = 128                       # PW_T: positions per statistics tile
U = 2.0 ** -24                   # half an ulp of float32, relative


def _rng(*key):
    return np.random.default_rng([int(k) & 0xFFFFFFFF for k in key])


def is_f32(a):
    """Every value of the float64 array is a float32 number."""
    a = np.asarray(a, dtype=F64)
    with np.errstate(over="ignore"):
        return bool(np.array_equal(a.astype(np.float32).astype(F64), a))


# ---- group 1 / 6: the convolution with the statistics epilogue, BatchNorm in training mode -----------------------------------

# (B, C_in, C_out, N).  N: one column; a ragged wave block; one column past a wave block; a ragged tile; exactly one full tile
# (the division-free path); one column past it; two full tiles and a column.  C_out = 130: a second row tile of two rows.
# C_in: 1, 3, and the 32-index chunk edge.  B = 3 > 1 gives three channel splits in apn_pw_bn_act (min(B, ceil(2048 / C))).
CONV_SHAPES = [(1, 1, 1, 1), (3, 3, 130, 31), (1, 33, 130, 33), (3, 32, 1, 127), (3, 32, 130, 128), (3, 33, 130, 129),
               (3, 3, 130, 257), (1, 3, 1, 257)]
CONV_AXES = dict(B={1, 3}, C_in={1, 3, 32, 33}, C_out={1, 130}, N={1, 31, 33, 127, 128, 129, 257})
OFFSETS = (0, 64, -64, 4096, -4096)          # the weight of the constant-1 input channel, per output channel
SPREAD = 4                                   # |y - offset| <= 4: two weights of +-1 on inputs in [-2, 2]
GAMMAS = (2, -1, 0, 3, -2)                   # positive, negative and exactly zero
BETAS = (-1, 0, 2, 1)
EPS = 1e-5
MOMENTUM = 0.5


def conv_id(shape):
    return "B%d-C%d-O%d-N%d" % tuple(shape)


def constant_channel(shape, o):
    """Output channel o is constant over all positions (variance exactly 0): no weight besides the offset's."""
    B, C, O, N = shape
    return C == 1 or (O > 1 and o % 7 == 3)


def conv_inputs(shape):
    """-> x (B, C, N), w (O, C) as float32 integers.  Input channel 0 is constant 1 and w[:, 0] the channel's offset; a
    channel that is not constant has two further weights of +1 / -1 on distinct inputs."""
    B, C, O, N = shape
    rng = _rng(1, *shape)
    x = rng.integers(-2, 3, size=(B, C, N))
    x[:, 0, :] = 1
    w = np.zeros((O, C), dtype=np.int64)
    for o in range(O):
        w[o, 0] = OFFSETS[(o + N) % len(OFFSETS)]
        if not constant_channel(shape, o):
            picks = rng.choice(np.arange(1, C), size=min(2, C - 1), replace=False)
            w[o, picks[0]] = 1
            if len(picks) > 1:
                w[o, picks[1]] = -1
    return x.astype(np.float32), w.astype(np.float32)


def conv_ref(x, w):
    """y[b, o, n] = sum_c w[o, c] x[b, c, n] in int64."""
    return np.einsum("oc,bcn->bon", w.astype(np.int64), x.astype(np.int64))


def conv_tiles(B, N):
    return B * ((N + TILE - 1) // TILE)


def part_ref(y):
    """The statistics rows of the forward product: part[b * tx + t] = {sum, M2 around the tile's own mean} of the columns
    [128 t, min(N, 128 t + 128)) of cloud b, per channel; float64 from exact integers, M2 = (n sum y^2 - (sum y)^2) / n."""
    B, O, N = y.shape
    tx = (N + TILE - 1) // TILE
    part = np.zeros((B * tx, 2, O), dtype=F64)
    for b in range(B):
        for t in range(tx):
            seg = y[b, :, TILE * t:min(N, TILE * (t + 1))].astype(np.int64)
            n = seg.shape[1]
            s, q = seg.sum(1), (seg * seg).sum(1)
            part[b * tx + t, 0] = s
            part[b * tx + t, 1] = (n * q - s * s).astype(F64) / n
    return part


def moments_ref(y):
    """-> (mean, biased variance, count) per channel over all B N values, float64 from exact integers."""
    B, O, N = y.shape
    cnt = B * N
    v = y.astype(np.int64).transpose(1, 0, 2).reshape(O, cnt)
    s, q = v.sum(1), (v * v).sum(1)
    return s.astype(F64) / cnt, (cnt * q - s * s).astype(F64) / (cnt * cnt), cnt


def bn_params(O, k):
    """gamma, beta (float32 integers; gamma of both signs and exactly 0), running_mean (integers), running_var (powers of
    two) for O channels; k shifts the cycles so that the one-channel cases differ."""
    o = np.arange(O) + k
    gamma = np.asarray(GAMMAS, dtype=np.float32)[o % len(GAMMAS)]
    beta = np.asarray(BETAS, dtype=np.float32)[o % len(BETAS)]
    rm = ((o % 7) - 3).astype(np.float32)
    rv = np.asarray((1.0, 4.0, 0.25), dtype=np.float32)[o % 3]
    return gamma, beta, rm, rv


def check_conv_exact(shape):
    """The preconditions of the exactness argument on the case's own values -> y."""
    x, w = conv_inputs(shape)
    B, C, O, N = shape
    assert np.array_equal(x, np.rint(x)) and np.abs(x).max() <= 2 and (x[:, 0] == 1).all()
    assert set(np.unique(w[:, 0])) <= set(OFFSETS) and np.abs(w[:, 1:]).max(initial=0) <= 1
    # every operand value fits one bf16 plane (8 significant bits)
    for a in (x, w):
        m, _ = np.frexp(a.astype(F64))
        assert np.array_equal(m * 256, np.rint(m * 256))
    # every partial sum of the contraction, in any order, is below 2^24
    assert (np.abs(w.astype(F64)) @ np.ones(C) * 2).max() < 2 ** 24
    y = conv_ref(x, w)
    assert np.abs(y).max() <= 2 ** 13
    # the tile sums are integers below 2^24; the deviations from any column of the tile and their squares' sum as well
    assert np.abs(part_ref(y)[:, 0]).max() < 2 ** 24
    assert TILE * (2 * SPREAD) ** 2 < 2 ** 24
    off = w[:, 0].astype(np.int64)[None, :, None]
    assert np.abs(y - off).max() <= SPREAD
    return y


# ---- group 2: BatchNorm + ReLU in eval mode --------------------------------------------------------------------------------

# (B, C, N): one value; odd N (scalar path); N % 4 == 0 (vector path); C = 1024: two channel splits serving 3 and 2 clouds
EVAL_SHAPES = [(1, 1, 1), (3, 7, 31), (2, 6, 64), (5, 1024, 4)]


def eval_inputs(shape, k=0):
    """y: integers in [-4, 4]; with eps = 0 and running_var in {1, 4, 1/4} invstd is 1, 1/2 or 2 and everything is exact.
    Many pre-activations are exactly 0 (y == running_mean where beta == 0), under both signs of gamma."""
    B, C, N = shape
    y = _rng(2, *shape).integers(-4, 5, size=(B, C, N)).astype(np.float32)
    return (y,) + bn_params(C, k)


def eval_ref(y, gamma, beta, rm, rv, relu):
    """-> stat (4, C) = {mean, invstd, scale, shift}, out; float64, eps = 0."""
    inv = 1.0 / np.sqrt(rv.astype(F64))
    sc = (np.ones_like(inv) if gamma is None else gamma.astype(F64)) * inv
    sh = (np.zeros_like(inv) if beta is None else beta.astype(F64)) - rm.astype(F64) * sc
    out = y.astype(F64) * sc[None, :, None] + sh[None, :, None]
    return np.stack([rm.astype(F64), inv, sc, sh]), (np.maximum(out, 0.0) if relu else out)


# ---- group 3: BatchNorm's gradient --------------------------------------------------------------------------------------------

FUSED_LIMIT = 32768              # B N <= 1024 threads x 8 float4: the fused route's limit
# (B, C, N) -> what it reaches
GRAD_SHAPES = [(1, 1, 4), (1, 1, 1), (3, 2, 5), (2, 3, 64), (3, 2, 100), (8, 1, 4096), (8, 1, 4100), (5, 1024, 6),
               (3, 2048, 2)]


def grad_id(shape):
    return "B%d-C%d-N%d" % tuple(shape)


def fused_route(shape):
    """The route apn_pw_bn_act_grad takes on 16-byte aligned operands."""
    B, C, N = shape
    return N % 4 == 0 and B * N <= FUSED_LIMIT


def channel_splits(B, C):
    return max(1, min(B, (2048 + C - 1) // C))


def grad_inputs(shape):
    """-> y, g (B, C, N), stat (4, C) = {mean, invstd, scale, shift}, all float32.  y in [-4, 4], g in [-3, 3]; integer
    mean, invstd in {1, 1/2, 2}, scale = gamma invstd with integer gamma of either sign or 0, shift = -scale y0 with y0 in
    {-4, 0, 4} (an integer): the pre-activation y scale + shift is exactly 0 wherever y == y0.  A channel with gamma == 0
    has shift 0 (nothing passes the ReLU) or 1 (everything passes)."""
    B, C, N = shape
    k = GRAD_SHAPES.index(tuple(shape))
    rng = _rng(3, *shape)
    y = rng.integers(-4, 5, size=(B, C, N)).astype(np.float32)
    g = rng.integers(-3, 4, size=(B, C, N)).astype(np.float32)
    c = np.arange(C) + k
    mean = ((c % 5) - 2).astype(F64)
    inv = np.asarray((1.0, 0.5, 2.0))[c % 3]
    gamma = np.asarray((2, -1, 0, 1, -2), dtype=F64)[c % 5]
    y0 = np.asarray((-4.0, 0.0, 4.0))[(c // 2) % 3]
    scale = gamma * inv
    shift = np.where(gamma == 0, (c // 5) % 2, -scale * y0)
    return y, g, np.stack([mean, inv, scale, shift]).astype(np.float32)


def grad_ref(y, g, stat, relu, training):
    """The float64 statement of BatchNorm's gradient behind an optional ReLU, on the statistics handed in:
        m = [y scale + shift > 0] (1 without ReLU),  yhat = (y - mean) invstd,
        g_gamma = sum g m yhat,  g_beta = sum g m,
        gy = scale (g m - mean(g m) - yhat mean(g m yhat))  (training)   or   scale g m  (running statistics).
    -> dict with gy, g_gamma, g_beta and the terms the element-wise bar of the rounded cases is made of."""
    B, C, N = y.shape
    y, g = y.astype(F64), g.astype(F64)
    mean, inv, sc, sh = (stat[i].astype(F64)[None, :, None] for i in range(4))
    pre = y * sc + sh
    m = (pre > 0).astype(F64) if relu else np.ones_like(y)
    gm = g * m
    yhat = (y - mean) * inv
    d1, d2 = gm.sum((0, 2)), (gm * yhat).sum((0, 2))
    res = dict(pre=pre, gm=gm, g_gamma=d2, g_beta=d1)
    if training:
        cnt = B * N
        m1, m2 = (d1 / cnt)[None, :, None], (d2 / cnt)[None, :, None]
        res["gy"] = sc * (gm - m1 - yhat * m2)
        # the kernels' form: gy = scale g m + k0 + k1 y
        res["k1"] = np.broadcast_to(-sc * inv * m2, y.shape)
        res["k0"] = np.broadcast_to(-sc * m1 + sc * inv * m2 * mean, y.shape)
        res["k0_terms"] = np.broadcast_to(np.abs(sc * m1) + np.abs(sc * inv * m2 * mean), y.shape)
    else:
        res["gy"] = sc * gm
        res["k0"] = res["k1"] = res["k0_terms"] = np.zeros_like(y)
    res["sgm"] = sc * gm
    return res


def grad_bar(ref, y):
    """Element-wise bound on |kernel gy - statement| in training mode when B N is no power of two.  The kernel forms
    k1 and k0 in float64 and rounds each ONCE to float32 (relative U = 2^-24 each), then gy = fma(g m, scale, fma(k1, y, k0)):
    two more roundings, of k1 y + k0 and of the result.  So
        |error| <= U (|k1 y| + |k0|)        the roundings of k1 and k0, carried through exactly
                 + U |k1 y + k0|            the inner fma
                 + U |gy|                   the outer fma
                 + 2^-45 (|scale g m| + |k1 y| + |k0| + the two terms k0 is the difference of)
    where the last line covers what is of second order in U (at most 3 U^2 of the magnitudes) and the float64 roundings of
    the kernel's own k0, k1 (a few 2^-53 of the TERMS of k0, which may cancel)."""
    y = y.astype(F64)
    k1y = np.abs(ref["k1"] * y)
    return (U * (k1y + np.abs(ref["k0"])) + U * np.abs(ref["k1"] * y + ref["k0"]) + U * np.abs(ref["gy"])
            + 2.0 ** -45 * (np.abs(ref["sgm"]) + k1y + np.abs(ref["k0"]) + ref["k0_terms"]))


def grad_exact(shape, training):
    """The case must equal the statement bit for bit: always with running statistics; in training mode where B N is a
    power of two (the two means are exact)."""
    B, C, N = shape
    return not training or (B * N) & (B * N - 1) == 0


def check_grad_exact(shape, relu, training):
    """The exactness preconditions on the case's own values: every sum below 2^24 in its own unit, and in training mode
    (power-of-two count) k0, k1, k1 y + k0 and the result all float32 numbers: each rounding of the kernel is exact."""
    y, g, stat = grad_inputs(shape)
    ref = grad_ref(y, g, stat, relu, training)
    mean, inv, sc, sh = (stat[i].astype(F64) for i in range(4))
    assert np.array_equal(mean, np.rint(mean)) and np.array_equal(sh, np.rint(sh))
    m, _ = np.frexp(inv)
    assert (m == 0.5).all()                                          # powers of two
    gamma = sc / inv
    assert np.array_equal(gamma, np.rint(gamma))
    # the sums: multiples of 1/4 (invstd >= 1/2, scale a multiple of 1/2), every partial sum below 2^22 in absolute value
    yhat = (y.astype(F64) - mean[None, :, None]) * inv[None, :, None]
    assert np.array_equal(yhat * 2, np.rint(yhat * 2))
    assert np.abs(g.astype(F64) * yhat).sum((0, 2)).max() < 2 ** 22 and np.abs(g).astype(F64).sum((0, 2)).max() < 2 ** 22
    assert is_f32(ref["g_gamma"]) and is_f32(ref["g_beta"])
    if grad_exact(shape, training):
        assert is_f32(ref["k0"]) and is_f32(ref["k1"]) and is_f32(ref["k1"] * y.astype(F64) + ref["k0"]) and is_f32(ref["gy"])
    return ref


# ---- group 4: convolution + bias + ReLU + max over the positions --------------------------------------------------------------

POOL_SHAPES = [(1, 1, 1, 1), (2, 3, 130, 129), (1, 33, 5, 33), (2, 4, 128, 257)]       # (B, C_in, C_out, N)
PEAK = 64                                    # the weight of the peak channel: above every other contribution (<= 32)
# cloud kinds: (name, positions of the peak) -- resolved against N by pool_peaks
POOL_KINDS = ("equal", "dup31", "dup127", "dupends", "last", "negative", "random")


def pool_peaks(kind, N):
    """The positions that hold the (duplicated) maximum of every channel with a positive peak weight, or None if the kind
    does not exist at this N."""
    if kind == "dup31":
        return (31, 32) if N > 32 else None
    if kind == "dup127":
        return (127, 128) if N > 128 else None
    if kind == "dupends":
        return (0, N - 1) if N > 1 else None
    if kind == "last":
        return (N - 1,)
    return ()


def pool_inputs(shape, kind):
    """-> x (B, C, N), w (O, C) float32 integers.  Input channel 0 is the peak channel h: 1 at the kind's positions, else 0
    (`negative`: 1 everywhere, with weight -64 on every output channel, so every product is negative; `equal`: all columns
    of a cloud equal; `random`: no peak channel, natural ties of small integers).  The columns at the peak positions are
    equal, so every channel ties there exactly; a channel with weight +64 on h has its maximum there and nowhere else,
    a channel with -64 somewhere among the other positions."""
    B, C, O, N = shape
    rng = _rng(4, POOL_KINDS.index(kind), *shape)
    x = rng.integers(-1, 2, size=(B, C, N))
    w = rng.integers(-1, 2, size=(O, C))
    if kind == "equal":
        x[:] = x[:, :, :1]
    elif kind == "negative":
        x[:, 0] = 1
        w[:, 0] = -PEAK
    elif kind != "random":
        peaks = pool_peaks(kind, N)
        x[:, 0] = 0
        x[:, 0, list(peaks)] = 1
        for p in peaks[1:]:
            x[:, :, p] = x[:, :, peaks[0]]
        w[:, 0] = np.where(np.arange(O) % 3 == 2, -PEAK, PEAK)
    return x.astype(np.float32), w.astype(np.float32)


def pool_bias(shape, y):
    """Integer bias that puts max + bias of cloud 0 below 0, at 0 and above 0 in turn over the channels."""
    O = shape[2]
    return (-y[0].max(1) + (np.arange(O) % 3 - 1)).astype(np.float32)


def pool_ref(y, bias, relu):
    """-> out (B, O) float64, idx (B, O): numpy's argmax is the FIRST maximum."""
    out = y.max(2).astype(F64) + (0.0 if bias is None else bias.astype(F64)[None])
    return (np.maximum(out, 0.0) if relu else out), y.argmax(2)


def pool_tiles_ref(y):
    """-> tile_val, tile_idx (B, tiles, O): every 128-column tile's maximum and its first position."""
    B, O, N = y.shape
    tx = (N + TILE - 1) // TILE
    val, idx = np.zeros((B, tx, O), dtype=F64), np.zeros((B, tx, O), dtype=np.int64)
    for t in range(tx):
        seg = y[:, :, TILE * t:min(N, TILE * (t + 1))]
        val[:, t], idx[:, t] = seg.max(2), seg.argmax(2) + TILE * t
    return val, idx


# ---- group 5: the convolution + max backward, on a supplied idx ---------------------------------------------------------------

POOLBWD_SHAPES = [(1, 1, 1, 1), (2, 128, 300, 65), (3, 5, 1024, 130)]                 # (B, C_in, C_out, N)
ALL_AT = 7                                   # the position every channel of a packed cloud picks
UNPICKED = 3                                 # a position no channel of a spread cloud picks


def poolbwd_inputs(shape):
    """-> x (B, C, N), w (O, C), g_out, out (B, O) float32 integers and idx (B, O) int32, every idx inside [0, N).
    Cloud 0 (where N > ALL_AT): all O channels at ONE position -- ceil(O / 256) ballot rounds and a list of O entries over
    both half-workgroups.  The last cloud is spread over all positions but UNPICKED, and includes 63, 64 and N - 1 (at
    N = 65 position 64 is the lone position of the second chunk).  A middle cloud has all channels at N - 1.
    out holds values <= 0 (no gradient under ReLU) and > 0."""
    B, C, O, N = shape
    rng = _rng(5, *shape)
    x = rng.integers(-2, 3, size=(B, C, N)).astype(np.float32)
    w = rng.integers(-2, 3, size=(O, C)).astype(np.float32)
    g_out = rng.integers(-3, 4, size=(B, O)).astype(np.float32)
    out = rng.integers(-2, 3, size=(B, O)).astype(np.float32)
    idx = rng.integers(0, N, size=(B, O))
    if N > ALL_AT:
        idx[idx == UNPICKED] = N - 1
        idx[-1, :3] = (63, 64, N - 1)
        idx[0] = ALL_AT
        if B > 2:
            idx[1] = N - 1
    return x, w, g_out, out, idx.astype(np.int32)


def poolbwd_ref(x, w, g_out, out, idx, relu):
    """-> xsel (B, O, C), g_x (B, C, N), g_w (O, C), g_bias (O,) in float64:
    gp = g_out [out > 0] (g_out without ReLU); xsel[b, o] = x[b, :, idx[b, o]];
    g_x[b, :, n] = sum over {o: idx[b, o] == n} of w[o, :] gp[b, o];  g_w[o] = sum_b gp[b, o] xsel[b, o];  g_bias = sum_b gp."""
    B, C, N = x.shape
    x, w = x.astype(F64), w.astype(F64)
    gp = g_out.astype(F64) * ((out > 0) if relu else 1.0)
    bi = np.arange(B)[:, None]
    xsel = x.transpose(0, 2, 1)[bi, idx]                              # (B, O, C)
    g_xt = np.zeros((B, N, C), dtype=F64)
    np.add.at(g_xt, (bi, idx), gp[:, :, None] * w[None])
    return xsel, g_xt.transpose(0, 2, 1), (gp[:, :, None] * xsel).sum(0), gp.sum(0)


# ---- group 6: the gradient products ---------------------------------------------------------------------------------------------

def conv_grad_inputs(shape):
    """gy (B, O, N): integers in [-2, 2] for apn_pw_conv_grad_input / _grad_weight on the inputs of conv_inputs."""
    B, C, O, N = shape
    return _rng(6, *shape).integers(-2, 3, size=(B, O, N)).astype(np.float32)


def conv_grad_ref(x, w, gy):
    """-> gx (B, C, N) = W^T gy, gw (O, C) = sum_b gy_b x_b^T, int64."""
    x, w, gy = (a.astype(np.int64) for a in (x, w, gy))
    return np.einsum("oc,bon->bcn", w, gy), np.einsum("bon,bcn->oc", gy, x)


def check_conv_grad_exact(shape):
    x, w = conv_inputs(shape)
    gy = conv_grad_inputs(shape)
    ax, aw, ag = (np.abs(a).astype(np.int64) for a in (x, w, gy))
    assert np.einsum("oc,bon->bcn", aw, ag).max() < 2 ** 24 and np.einsum("bon,bcn->oc", ag, ax).max() < 2 ** 24
    return conv_grad_ref(x, w, gy)
