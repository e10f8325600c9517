"""CPU suite: the case tables and the float64 statements of tests/pointwise_cases.py keep their own promises -- coverage of
what csrc/pointwise.hip treats differently, the exactness argument on every case's own values (so that the GPU suite needs
no exclusion anywhere), the tie clouds' ties, the zero pre-activations, and the statements against float64 PyTorch with
autograd (BatchNorm1d().double() + relu; max(dim) for the convolution + max pair).  No kernel runs."""
import numpy as np
import pytest
import torch

import pointwise_cases as P

TINY = 2.0 ** -80                # PyTorch refuses eps = 0; in float64 running_var + 2^-80 == running_var for the powers of two here


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double()


# ---- the tables ---------------------------------------------------------------------------------------------------------------

def test_the_conv_table_covers_every_axis_value():
    for i, name in enumerate(("B", "C_in", "C_out", "N")):
        assert {s[i] for s in P.CONV_SHAPES} == P.CONV_AXES[name], name
    assert P.CONV_AXES == dict(B={1, 3}, C_in={1, 3, 32, 33}, C_out={1, 130}, N={1, 31, 33, 127, 128, 129, 257})
    assert (1, 1, 1, 1) in P.CONV_SHAPES                                       # B = N = 1: the unbiased factor is 1
    # several workgroups see channel 0 of apn_pw_bn_act: a case with more than one channel split
    assert any(P.channel_splits(s[0], s[2]) > 1 for s in P.CONV_SHAPES)
    # a full tile on the division-free path (N >= 128) with B > 1, and ragged tiles behind full ones
    assert any(s[3] % P.TILE == 0 and s[0] > 1 for s in P.CONV_SHAPES) and any(s[3] > P.TILE and s[3] % P.TILE for s in P.CONV_SHAPES)
    assert len({P.conv_id(s) for s in P.CONV_SHAPES}) == len(P.CONV_SHAPES)
    # gamma: positive, negative and exactly zero -- over the channels of the wide cases and over the one-channel cases
    assert {np.sign(g) for g in P.GAMMAS} == {-1.0, 0.0, 1.0}
    ones = [P.bn_params(1, k)[0][0] for k, s in enumerate(P.CONV_SHAPES) if s[2] == 1]
    assert any(g > 0 for g in ones) and any(g <= 0 for g in ones)
    assert set(np.abs(P.OFFSETS)) == {0, 64, 4096} and P.MOMENTUM == 0.5


def test_the_grad_table_reaches_both_routes_and_the_limit():
    want = {(1, 1, 4): True, (1, 1, 1): False, (3, 2, 5): False, (2, 3, 64): True, (3, 2, 100): True, (8, 1, 4096): True,
            (8, 1, 4100): False, (5, 1024, 6): False, (3, 2048, 2): False}
    assert {s: P.fused_route(s) for s in P.GRAD_SHAPES} == want
    assert 8 * 4096 == P.FUSED_LIMIT and 8 * 4100 > P.FUSED_LIMIT and 4100 % 4 == 0         # the limit itself, and just over
    assert (3 * 100 // 4) == 75                                                          # 75 quads: lanes idle
    assert P.channel_splits(5, 1024) == 2 and P.channel_splits(3, 2048) == 1                # splits serving 3 + 2, and all, clouds
    assert P.channel_splits(5, 1024) < 5 and [s for s in P.EVAL_SHAPES if P.channel_splits(s[0], s[1]) < s[0]]
    # exact in training mode where the count is a power of two; rounded cases on both routes
    exact = {s for s in P.GRAD_SHAPES if P.grad_exact(s, True)}
    assert exact == {(1, 1, 4), (1, 1, 1), (2, 3, 64), (8, 1, 4096)}
    assert any(P.fused_route(s) for s in set(P.GRAD_SHAPES) - exact) and any(not P.fused_route(s) for s in set(P.GRAD_SHAPES) - exact)
    # gamma of both signs and zero over the table, also among the one-channel cases
    signs = set()
    for s in P.GRAD_SHAPES:
        stat = P.grad_inputs(s)[2]
        signs |= set(np.sign(stat[2]).tolist())
    assert signs == {-1.0, 0.0, 1.0}
    assert {np.sign(P.grad_inputs(s)[2][2][0]) for s in P.GRAD_SHAPES if s[1] == 1} >= {-1.0, 1.0}


def test_the_pool_tables():
    assert P.POOL_SHAPES == [(1, 1, 1, 1), (2, 3, 130, 129), (1, 33, 5, 33), (2, 4, 128, 257)]
    assert P.POOLBWD_SHAPES == [(1, 1, 1, 1), (2, 128, 300, 65), (3, 5, 1024, 130)]
    # every tie pair occurs: inside a wave block's neighbours (31, 32), across tiles (127, 128), first and last
    for kind, pair in (("dup31", (31, 32)), ("dup127", (127, 128))):
        assert [P.pool_peaks(kind, s[3]) for s in P.POOL_SHAPES if P.pool_peaks(kind, s[3])][0] == pair
    assert P.pool_peaks("dupends", 257) == (0, 256) and P.pool_peaks("dupends", 1) is None
    assert (300 + 255) // 256 == 2 and (1024 + 255) // 256 == 4 and 65 - 64 == 1
    assert all(s[1] <= 128 and s[2] < 2 ** 24 for s in P.POOLBWD_SHAPES)                       # the entry's own limits


# ---- the exactness preconditions, on every case's own values --------------------------------------------------------------------

@pytest.mark.parametrize("shape", P.CONV_SHAPES, ids=P.conv_id)
def test_conv_cases_are_exact_and_have_their_channels(shape):
    B, C, O, N = shape
    y = P.check_conv_exact(shape)
    mean, var, cnt = P.moments_ref(y)
    const = np.array([P.constant_channel(shape, o) for o in range(O)])
    spread = y.max((0, 2)) - y.min((0, 2))
    assert (spread[const] == 0).all() and (var[const] == 0).all()                 # variance exactly 0
    if B * N > 1:
        assert (spread[~const] > 0).all()
    if O > 1:
        assert const.any() and (~const).any()
    # the "mean 100x the spread" channels: a float32 sum of squares cannot resolve their variance
    big = np.abs(mean) >= 4000
    if O > 1:
        assert (big & ~const).any() and (100 * spread[big] <= np.abs(mean[big])).all()
        o = int(np.flatnonzero(big & ~const)[0])
        v = y[:, o].reshape(-1).astype(np.float32)
        s2 = np.float32(0)
        for e in v * v:
            s2 = np.float32(s2 + e)
        naive = float(s2) / cnt - float(np.float32(v.sum() / cnt)) ** 2
        assert abs(naive - var[o]) > 1e-3 * var[o]               # the sum-of-squares fold misses the 1e-6 bar by 1000x here
    # the statements: part folds to the moments; float64 BatchNorm1d agrees
    part = P.part_ref(y)
    assert part.shape == (P.conv_tiles(B, N), 2, O) and np.array_equal(part[:, 0].sum(0), y.sum((0, 2)))
    tx = (N + P.TILE - 1) // P.TILE
    nt = np.array([min(P.TILE, N - P.TILE * (i % tx)) for i in range(B * tx)], dtype=np.float64)[:, None]
    m2 = part[:, 1].sum(0) + (nt * (part[:, 0] / nt - mean[None]) ** 2).sum(0)
    assert np.allclose(m2 / cnt, var, rtol=1e-12, atol=1e-12)
    assert (part[:, 1][:, const] == 0).all()


@pytest.mark.parametrize("shape", P.CONV_SHAPES, ids=P.conv_id)
def test_batchnorm_statement_matches_float64_pytorch(shape):
    B, C, O, N = shape
    k = P.CONV_SHAPES.index(shape)
    y = P.conv_ref(*P.conv_inputs(shape))
    gamma, beta, rm, rv = P.bn_params(O, k)
    mean, var, cnt = P.moments_ref(y)
    bn = torch.nn.BatchNorm1d(O, eps=P.EPS, momentum=P.MOMENTUM).double()
    with torch.no_grad():
        bn.weight.copy_(_t(gamma)); bn.bias.copy_(_t(beta)); bn.running_mean.copy_(_t(rm)); bn.running_var.copy_(_t(rv))
    if cnt == 1:                                                    # PyTorch refuses one value per channel in training mode
        assert (var == 0).all()
        return
    out = torch.relu(bn(_t(y)))
    inv = 1.0 / np.sqrt(var + P.EPS)
    sc = gamma * inv
    want = np.maximum(y * sc[None, :, None] + (beta - mean * sc)[None, :, None], 0.0)
    assert np.allclose(out.detach().numpy(), want, rtol=1e-9, atol=1e-9)
    assert np.allclose(bn.running_mean.numpy(), 0.5 * rm + 0.5 * mean, rtol=1e-12, atol=1e-12)
    assert np.allclose(bn.running_var.numpy(), 0.5 * rv + 0.5 * var * cnt / (cnt - 1), rtol=1e-12, atol=1e-12)
    assert int(bn.num_batches_tracked) == 1


@pytest.mark.parametrize("shape", P.EVAL_SHAPES, ids=P.grad_id)
def test_eval_cases_are_exact_and_have_zero_preactivations(shape):
    B, C, N = shape
    y, gamma, beta, rm, rv = P.eval_inputs(shape)
    assert set(np.unique(rv)) <= {1.0, 4.0, 0.25} and np.array_equal(rm, np.rint(rm))
    for relu in (0, 1):
        stat, out = P.eval_ref(y, gamma, beta, rm, rv, relu)
        assert P.is_f32(stat) and P.is_f32(out) and set(np.unique(stat[1])) <= {1.0, 0.5, 2.0}
        bn = torch.nn.BatchNorm1d(C, eps=TINY).double().eval()
        with torch.no_grad():
            bn.weight.copy_(_t(gamma)); bn.bias.copy_(_t(beta)); bn.running_mean.copy_(_t(rm)); bn.running_var.copy_(_t(rv))
        ref = bn(_t(y)).detach()
        assert np.array_equal((torch.relu(ref) if relu else ref).numpy(), out)
    pre = P.eval_ref(y, gamma, beta, rm, rv, 0)[1]
    if C > 1:                                                       # ReLU at exactly 0 under both signs of gamma
        for sign in (1, -1):
            assert (pre[:, np.sign(gamma) == sign] == 0).any()
        assert (pre < 0).any() and (pre > 0).any()


@pytest.mark.parametrize("training", (0, 1))
@pytest.mark.parametrize("relu", (0, 1))
@pytest.mark.parametrize("shape", P.GRAD_SHAPES, ids=P.grad_id)
def test_grad_cases_are_exact_where_they_claim(shape, relu, training):
    ref = P.check_grad_exact(shape, relu, training)
    B, C, N = shape
    if relu and B * C * N >= 30:
        y, g, stat = P.grad_inputs(shape)
        zero = ref["pre"] == 0
        assert zero.mean() > 0.05                                   # many pre-activations exactly 0 ...
        assert not ref["gm"][zero].any() and (g[zero] != 0).any()   # ... which pass no gradient, though g has some there
    if not P.grad_exact(shape, training):
        y = P.grad_inputs(shape)[0]
        bar = P.grad_bar(ref, y)
        assert (bar >= 0).all() and (bar[ref["gy"] != 0] > 0).all()
        assert (bar <= 2.0 ** -21 * (np.abs(ref["sgm"]) + np.abs(ref["k1"] * y) + np.abs(ref["k0"]) + ref["k0_terms"]) + 1e-300).all()


@pytest.mark.parametrize("relu", (0, 1))
@pytest.mark.parametrize("shape", [(3, 2, 5), (2, 3, 64), (5, 8, 6)], ids=P.grad_id)
def test_grad_statement_matches_float64_autograd(shape, relu):
    """grad_ref on the batch's OWN statistics against BatchNorm1d().double() (+ relu) under autograd, in training and in eval
    mode (there on the integer statistics of grad_inputs, zeros of the pre-activation included: relu'(0) = 0)."""
    B, C, N = shape
    rng = np.random.default_rng(B * C * N)
    y, g = rng.standard_normal((B, C, N)), rng.standard_normal((B, C, N))
    gamma, beta = rng.standard_normal(C), rng.standard_normal(C)
    eps = 1e-5
    for training in (1, 0):
        if training:
            v = y.transpose(1, 0, 2).reshape(C, -1)
            mean, var = v.mean(1), v.var(1)
            yy, gg = y, g
        else:
            yi, gi, stat = (a.astype(np.float64) for a in P.grad_inputs((3, 2, 5) if shape[1] == 2 else (2, 3, 64))[:3])
            if yi.shape != y.shape:
                continue
            yy, gg = yi, gi
            mean, var, eps = stat[0], 1.0 / stat[1] ** 2, 0.0
            gamma = stat[2] / stat[1]
            beta = stat[3] + mean * stat[2]
        inv = 1.0 / np.sqrt(var + eps)
        stat64 = np.stack([mean, inv, gamma * inv, beta - mean * gamma * inv])
        bn = torch.nn.BatchNorm1d(C, eps=eps or TINY).double()
        with torch.no_grad():
            bn.weight.copy_(_t(gamma)); bn.bias.copy_(_t(beta)); bn.running_mean.copy_(_t(mean)); bn.running_var.copy_(_t(var))
        bn.train(bool(training))
        yt = _t(yy).requires_grad_(True)
        out = bn(yt)
        (torch.relu(out) if relu else out).backward(_t(gg))
        ref = P.grad_ref(yy, gg, stat64, relu, training)
        tol = dict(rtol=1e-9, atol=1e-9) if training else dict(rtol=0, atol=0)
        assert np.allclose(yt.grad.numpy(), ref["gy"], **tol)
        assert np.allclose(bn.weight.grad.numpy(), ref["g_gamma"], **tol) and np.allclose(bn.bias.grad.numpy(), ref["g_beta"], **tol)


# ---- the convolution + max pair -----------------------------------------------------------------------------------------------

def _pool_cases():
    return [(s, k) for s in P.POOL_SHAPES for k in P.POOL_KINDS if P.pool_peaks(k, s[3]) is not None]


@pytest.mark.parametrize("shape,kind", _pool_cases(), ids=lambda v: v if isinstance(v, str) else P.conv_id(v))
def test_pool_clouds_contain_their_ties(shape, kind):
    B, C, O, N = shape
    x, w = P.pool_inputs(shape, kind)
    y = P.conv_ref(x, w)
    assert np.abs(x).max() <= 1 and np.abs(w).max() <= P.PEAK and np.abs(y).max() < 2 ** 13
    out, idx = P.pool_ref(y, None, 0)
    peaks = P.pool_peaks(kind, N)
    if kind == "equal":
        assert (y == y[:, :, :1]).all() and (idx == 0).all()
    elif kind == "negative":
        assert (y < 0).all() and (out < 0).all() and not P.pool_ref(y, None, 1)[0].any()
    elif kind == "random":
        if N > 1:
            assert ((y == y.max(2, keepdims=True)).sum(2) > 1).any()           # natural ties
    else:
        up = w[:, 0] > 0
        assert up.any() and (O < 3 or (~up).any())
        hit = y == y.max(2, keepdims=True)
        mask = np.zeros(N, dtype=bool)
        mask[list(peaks)] = True
        assert (hit[:, up] == mask).all()                                      # the maximum at the peaks and nowhere else
        assert (idx[:, up] == peaks[0]).all()                                  # ... so the lowest of them wins
        if O >= 3 and N > 3:
            assert (idx[:, ~up] != peaks[0]).all()
    # the tile records fold to the result
    tv, ti = P.pool_tiles_ref(y)
    assert np.array_equal(tv.max(1), y.max(2))
    assert np.array_equal(np.take_along_axis(ti, tv.argmax(1)[:, None], 1)[:, 0], idx)
    # max + bias below, at and above 0
    bias = P.pool_bias(shape, y)
    pre = y.max(2)[0] + bias
    assert {np.sign(v) for v in pre} == ({-1.0, 0.0, 1.0} if O >= 3 else {-1.0})
    # float64 PyTorch: max(dim) returns the first maximum
    tout, tidx = torch.einsum("oc,bcn->bon", _t(w), _t(x)).max(2)
    assert np.array_equal(tidx.numpy(), idx)
    assert np.array_equal(torch.relu(tout + _t(bias)).numpy(), P.pool_ref(y, bias, 1)[0])


@pytest.mark.parametrize("shape,kind", [((2, 3, 130, 129), "dup127"), ((1, 33, 5, 33), "random"), ((1, 1, 1, 1), "last")],
                         ids=lambda v: v if isinstance(v, str) else P.conv_id(v))
@pytest.mark.parametrize("relu", (0, 1))
def test_pool_backward_statement_matches_float64_autograd(shape, kind, relu):
    B, C, O, N = shape
    x, w = P.pool_inputs(shape, kind)
    y = P.conv_ref(x, w)
    bias = P.pool_bias(shape, y)
    out, idx = P.pool_ref(y, bias, relu)
    g = np.random.default_rng(0).integers(-3, 4, size=(B, O)).astype(np.float64)
    xt, wt, bt = (_t(a).requires_grad_(True) for a in (x, w, bias))
    o = torch.einsum("oc,bcn->bon", wt, xt).max(2)[0] + bt
    (torch.relu(o) if relu else o).backward(_t(g))
    xsel, g_x, g_w, g_bias = P.poolbwd_ref(x, w, g, out, idx, relu)
    assert np.array_equal(xt.grad.numpy(), g_x) and np.array_equal(wt.grad.numpy(), g_w) and np.array_equal(bt.grad.numpy(), g_bias)


@pytest.mark.parametrize("shape", P.POOLBWD_SHAPES, ids=P.conv_id)
def test_poolbwd_cases_have_their_lists(shape):
    B, C, O, N = shape
    x, w, g_out, out, idx = P.poolbwd_inputs(shape)
    assert idx.dtype == np.int32 and idx.min() >= 0 and idx.max() < N          # never outside [0, N): the entry's contract
    assert (out <= 0).any() and (out > 0).any() or B * O == 1
    if N > P.ALL_AT:
        assert (idx[0] == P.ALL_AT).all()                                     # all O channels at one position
        assert not (idx[-1] == P.UNPICKED).any() and len(np.unique(idx[-1])) > N // 2
        assert {63, 64, N - 1} <= set(idx[-1].tolist())
    if B > 2:
        assert (idx[1] == N - 1).all()
    for relu in (0, 1):
        xsel, g_x, g_w, g_bias = P.poolbwd_ref(x, w, g_out, out, idx, relu)
        assert all(P.is_f32(a) for a in (xsel, g_x, g_w, g_bias))
        assert O * 2 * 3 < 2 ** 24 and B * 2 * 3 < 2 ** 24                      # every partial sum is a small integer
        if N > P.ALL_AT:
            picked = np.zeros((B, N), dtype=bool)
            picked[np.arange(B)[:, None], idx] = True
            assert not g_x.transpose(0, 2, 1)[~picked].any() and (~picked).any()   # zeros where no channel picks


@pytest.mark.parametrize("shape", P.CONV_SHAPES, ids=P.conv_id)
def test_conv_gradient_products_are_exact(shape):
    gx, gw = P.check_conv_grad_exact(shape)
    x, w = P.conv_inputs(shape)
    gy = P.conv_grad_inputs(shape)
    xt, wt = _t(x).requires_grad_(True), _t(w).requires_grad_(True)
    torch.nn.functional.conv1d(xt, wt.unsqueeze(-1)).backward(_t(gy))
    assert np.array_equal(xt.grad.numpy(), gx) and np.array_equal(wt.grad.numpy(), gw)
    assert np.array_equal(torch.nn.functional.conv1d(_t(x), _t(w).unsqueeze(-1)).numpy(), P.conv_ref(x, w))
