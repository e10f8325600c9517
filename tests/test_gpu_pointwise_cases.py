"""GPU suite: the kernels of csrc/pointwise.hip AROUND the contraction body, through their raw entries, on the exact cases of
tests/pointwise_cases.py (tests/test_pointwise_cases_cpu.py checks the cases and the statements on the CPU):

  group 1  apn_pw_conv_forward (y and the tile statistics `part`), then apn_pw_bn_act in training mode
  group 2  apn_pw_bn_act in eval mode
  group 3  apn_pw_bn_act_grad on both routes (one fused launch; sums + apply), and their agreement
  group 4  apn_pw_conv_max_forward: the tie rule inside a wave, across waves and across tiles
  group 5  apn_pw_conv_max_backward on a supplied idx
  group 6  apn_pw_conv_grad_input / apn_pw_conv_grad_weight and the scalar loaders of all three products

Inputs are small integers and the scales powers of two, so every float32 sum, product and fma is exact in any order and a
value fits one bf16 plane: results must EQUAL the float64 statement, at precision 2 and 3, with no element excluded.  The
bars that are not equalities stand where they are used, each with its derivation and -- as documentation only -- the worst
value measured on an MI355X (MEASURED below; test_zz prints the current ones).

Buffers: every output and scratch buffer is a view into a wider parent, prefilled with NaN (floats) or a sentinel (ints);
every element of a result must have been written and nothing outside the view may change.
"""
import numpy as np
import pytest
import torch

import pointwise_cases as P

pytestmark = pytest.mark.gpu

# Measured on an MI355X (whole-file run: 167 tests in 2.7 s, the slowest 0.3 s -- the first, which loads the library), the
# worst value against each bar that is not an equality.  Documentation only: no bar is taken from these.
MEASURED = """
    part M2            |kernel - float64| / (2^-23 float64)           0.48   B1-C33-O130-N33, precision 3
    stat mean          relative error / 1e-6                          0.059  B3-C33-O130-N129
    stat variance      relative error / 1e-6  (from invstd)           0.12   B3-C33-O130-N129
    invstd at var = 0  relative error / 1e-6                          0.054  B3-C3-O130-N257
    run_var            relative error / 1e-6                          0.088  B3-C32-O130-N128
    gy, rounded cases  |kernel - float64| / grad_bar                  0.92   B5-C1024-N6, two-pass route, no ReLU
"""
# gy sits just below its bar because the bar counts the four roundings that happen at half an ulp each and among 30 000
# elements some come close to every worst case at once.  Every other comparison in this file is an equality, and all of
# them held at precision 2 and 3: the kernels needed no change.
# Mutation check (one line of csrc/pointwise.hip changed in a scratch library, arithmetic only -- none can read or write
# outside an array; this file run once per library):
#   pool epilogue, cross-wave merge: `cand > best` -> `cand >= best`       34 fail: test_conv_max_forward_and_the_tie_rule,
#                                                                          every kind at N = 129 and 257, the tie kinds at N = 33
#   pw_bn_act_kernel: nt always 128                                        21 fail: test_bn_act_training at every N but 128
#   pw_bwd_fused_kernel: the `in &&` term of the mask dropped              12 fail: test_bn_act_grad_on_both_routes at
#                                                                          B1-C1-N4, B2-C3-N64 and B3-C2-N100 (idle slots)
# scale and shift: EQUAL, both.  scale = gamma * invstd is one multiplication; shift = beta - mean * scale is two operations
# in source order -- the library is built with -ffp-contract=off (a flag adaptpoint_amd/build.py requires and _lib.load()
# checks), so the product is rounded before the subtraction: shift == fl32(beta - fl32(mean * scale)).  (A contracted build
# would differ by far more than one ulp of a small shift: the product's rounding is relative to mean * scale.)

SENT = -7777
WORST = {}


def _note(name, value, what):
    if value >= WORST.get(name, (-1.0, None))[0]:
        WORST[name] = (float(value), what)


def _call(*a):
    from adaptpoint_amd.fused import _call as call
    return call(*a)


# ---- poisoned buffers ---------------------------------------------------------------------------------------------------------

class Box:
    """A tensor as a view `lead` elements into a poisoned parent: lead = 4 keeps a float view 16-byte aligned, lead = 1 puts
    it one float off (the kernels' scalar paths, the two-pass route of the gradient)."""

    def __init__(self, dev, shape, dtype=torch.float32, lead=4, data=None):
        self.n = int(np.prod(shape))
        self.lead, self.float = lead, dtype.is_floating_point
        self.parent = torch.full((self.n + lead + 4,), float("nan") if self.float else SENT, dtype=dtype, device=dev)
        self.t = self.parent[lead:lead + self.n].view(shape)
        if dtype == torch.float32:
            assert self.t.data_ptr() % 16 == (4 * lead) % 16
        if data is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(data)).to(dtype))

    @property
    def ptr(self):
        return self.t.data_ptr()

    def _poison(self, t):
        return torch.isnan(t) if self.float else t == SENT

    def intact(self):
        """Nothing outside the view changed."""
        return bool(self._poison(self.parent[:self.lead]).all()) and bool(self._poison(self.parent[self.lead + self.n:]).all())

    def result(self, what):
        """The view as float64 / int64 numpy, after the assertions of the buffer discipline."""
        assert self.intact(), f"{what}: written outside the buffer"
        assert not bool(self._poison(self.t).any()), f"{what}: an element was never written (or a NaN came out)"
        return self.t.cpu().numpy().astype(np.float64 if self.float else np.int64)

    def untouched(self):
        return self.intact() and bool(self._poison(self.t).all())


def _in(dev, a, lead=4):
    return Box(dev, a.shape, lead=lead, data=a)


def _p(box):
    return None if box is None else box.ptr


# ---- group 1: the forward product with its statistics, BatchNorm in training mode ---------------------------------------------

_FWD = {}


def _forward(dev, shape, precision, lead=4, with_part=True):
    B, C, O, N = shape
    x, w = P.conv_inputs(shape)
    xb, wb = _in(dev, x, lead), _in(dev, w, lead)
    y = Box(dev, (B, O, N))
    tiles = P.conv_tiles(B, N)
    part = Box(dev, (tiles, 2, O))
    _call("apn_pw_conv_forward", dev, B, C, O, N, precision, xb.ptr, wb.ptr, y.ptr, part.ptr if with_part else None)
    return y, part, tiles


def _forward_checked(dev, shape, precision):
    """The forward product of the case, checked once per (shape, precision) -> (y, part, tiles) for the BatchNorm tests."""
    key = (shape, precision)
    if key not in _FWD:
        from adaptpoint_amd import _lib
        B, C, O, N = shape
        y, part, tiles = _forward(dev, shape, precision)
        assert tiles == _lib.load().apn_pw_conv_tiles(B, N)
        ref = P.conv_ref(*P.conv_inputs(shape))
        assert np.array_equal(y.result("y"), ref)
        got, want = part.result("part"), P.part_ref(ref)         # no NaN, nothing outside tiles x 2 x C_out
        # the sum: an integer below 2^24 -- equal
        assert np.array_equal(got[:, 0], want[:, 0])
        # M2: float64 in the kernel, rounded ONCE to float32: relative 2^-23 (2^-24 for the rounding; the float64 steps
        # before it are 2^-29 of that); a channel that is constant on the tile has M2 exactly 0 (the bar is 0 there)
        err = np.abs(got[:, 1] - want[:, 1])
        assert (err <= 2.0 ** -23 * want[:, 1]).all(), (err / np.maximum(want[:, 1], 1e-300)).max()
        const = np.array([P.constant_channel(shape, o) for o in range(O)])
        assert not got[:, 1][:, const].any()
        pos = want[:, 1] > 0
        if pos.any():
            _note("part M2 / (2^-23 ref)", (err[pos] / (2.0 ** -23 * want[:, 1][pos])).max(), (P.conv_id(shape), precision))
        _FWD[key] = (y, part, tiles, ref)
    return _FWD[key]


@pytest.mark.parametrize("precision", (2, 3))
@pytest.mark.parametrize("shape", P.CONV_SHAPES, ids=P.conv_id)
def test_conv_forward_y_and_tile_statistics(dev, shape, precision):
    _forward_checked(dev, shape, precision)
    # part = null: y alone, the same bits
    y, part, _ = _forward(dev, shape, precision, with_part=False)
    assert torch.equal(y.t, _FWD[(shape, precision)][0].t) and y.intact() and part.untouched()


@pytest.mark.parametrize("precision", (2, 3))
@pytest.mark.parametrize("shape", [(3, 32, 130, 128), (3, 33, 130, 129), (1, 3, 1, 257)], ids=P.conv_id)
def test_conv_forward_from_operands_one_float_into_a_parent(dev, shape, precision):
    """x and w 4 bytes off a 16-byte boundary: the scalar loaders; y and part carry the same bits as the aligned run."""
    y0, part0, _, _ = _forward_checked(dev, shape, precision)
    y, part, _ = _forward(dev, shape, precision, lead=1)
    assert torch.equal(y.t, y0.t) and torch.equal(part.t, part0.t) and y.intact() and part.intact()


def _bn_train(dev, shape, gamma, beta, relu, buffers, k=5):
    B, C, O, N = shape
    y, part, tiles, ref = _forward_checked(dev, shape, 2)
    _, _, rm, rv = P.bn_params(O, P.CONV_SHAPES.index(shape))
    gb, bb = (None if a is None else _in(dev, a) for a in (gamma, beta))
    rmb, rvb = _in(dev, rm), _in(dev, rv)
    batches = Box(dev, (1,), dtype=torch.int64, lead=2, data=np.array([k]))
    stat, out = Box(dev, (4, O)), Box(dev, (B, O, N))
    _call("apn_pw_bn_act", dev, B, O, N, y.ptr, part.ptr, tiles, _p(gb), _p(bb), P.EPS, P.MOMENTUM, 1, relu,
          rmb.ptr if buffers else None, rvb.ptr if buffers else None, batches.ptr if buffers else None, stat.ptr, out.ptr)
    return ref, stat, out, rmb, rvb, batches, rm, rv


@pytest.mark.parametrize("variant", ("affine-relu", "affine", "null-relu"))
@pytest.mark.parametrize("shape", P.CONV_SHAPES, ids=P.conv_id)
def test_bn_act_training(dev, shape, variant):
    B, C, O, N = shape
    what = (P.conv_id(shape), variant)
    k = 5
    gamma, beta, _, _ = P.bn_params(O, P.CONV_SHAPES.index(shape))
    if variant.startswith("null"):
        gamma = beta = None
    relu = int(variant.endswith("relu"))
    ref, statb, outb, rmb, rvb, batches, rm, rv = _bn_train(dev, shape, gamma, beta, relu, True, k)
    stat = statb.result("stat")
    mean, var, cnt = P.moments_ref(ref)
    # mean and variance at rtol = 1e-6: the fold is float64 on exact tile sums and once-rounded M2 shares (2^-24 each), and
    # the mean is stored with one float32 rounding (6e-8); a zero sum gives an exact 0 (atol = 0)
    assert np.allclose(stat[0], mean, rtol=1e-6, atol=0), np.abs(stat[0] - mean).max()
    nz = mean != 0
    if nz.any():
        _note("stat mean rel / 1e-6", (np.abs(stat[0] - mean)[nz] / np.abs(mean[nz])).max() / 1e-6, what)
    # the variance is recovered from invstd = 1 / sqrt(var + eps), stored with one rounding: 1.2e-7 (var + eps), inside
    # 1e-6 var wherever var > eps / 7 -- integer data has var >= (cnt - 1) / cnt^2 > 1e-3 or exactly 0
    pos = var > 0
    assert (var[pos] > 1e-3).all()
    got_var = 1.0 / (stat[1] * stat[1]) - P.EPS
    assert np.allclose(got_var[pos], var[pos], rtol=1e-6, atol=0)
    assert np.allclose(stat[1][~pos], 1.0 / np.sqrt(P.EPS), rtol=1e-6, atol=0)
    if pos.any():
        _note("stat var rel / 1e-6", np.abs(got_var[pos] / var[pos] - 1).max() / 1e-6, what)
    if (~pos).any():
        _note("invstd at var = 0, rel / 1e-6", np.abs(stat[1][~pos] * np.sqrt(P.EPS) - 1).max() / 1e-6, what)
    # scale and shift from the RETURNED mean and invstd: equal (the note below MEASURED)
    g64 = np.ones(O) if gamma is None else gamma.astype(np.float64)
    b64 = np.zeros(O) if beta is None else beta.astype(np.float64)
    assert np.array_equal(stat[2], (g64 * stat[1]).astype(np.float32).astype(np.float64))
    product = (stat[0] * stat[2]).astype(np.float32).astype(np.float64)
    assert np.array_equal(stat[3], (b64 - product).astype(np.float32).astype(np.float64))
    # out = fl32(y scale + shift) from the returned scale and shift: the product is exact in float64 (13 x 24 bits), and the
    # sum is checked to be exact as well (its two-sum residual is zero), so one rounding to float32 is the fma's
    prod = ref.astype(np.float64) * stat[2][None, :, None]
    sh = np.broadcast_to(stat[3][None, :, None], prod.shape)
    s = prod + sh
    bv = s - prod
    assert not ((prod - (s - bv)) + (sh - bv)).any()
    want = s.astype(np.float32).astype(np.float64)
    out = outb.result("out")
    assert np.array_equal(out, np.maximum(want, 0.0) if relu else want)
    # the running buffers: momentum 1/2, integer running_mean, power-of-two running_var
    run_mean, run_var = rmb.result("run_mean"), rvb.result("run_var")
    assert np.array_equal(run_mean, (0.5 * rm.astype(np.float64) + 0.5 * stat[0]).astype(np.float32).astype(np.float64))
    factor = cnt / (cnt - 1.0) if cnt > 1 else 1.0
    want_rv = 0.5 * rv.astype(np.float64) + 0.5 * var * factor
    # rtol = 1e-6: the float64 variance above, rounded to float32 with its factor, halved (exact) and added: two roundings
    assert np.allclose(run_var, want_rv, rtol=1e-6, atol=0)
    _note("run_var rel / 1e-6", np.abs(run_var / want_rv - 1).max() / 1e-6, what)
    if cnt == 1:
        assert not var.any() and np.array_equal(run_var, 0.5 * rv.astype(np.float64))        # the unbiased factor is 1
    assert int(batches.result("batches")[0]) == k + 1                     # once, however many workgroups see channel 0
    # run_mean = run_var = batches = null: the same stat and out
    _, stat2, out2, rmb2, rvb2, batches2, _, _ = _bn_train(dev, shape, gamma, beta, relu, False, k)
    assert torch.equal(stat2.t, statb.t) and torch.equal(out2.t, outb.t) and stat2.intact() and out2.intact()
    assert np.array_equal(rmb2.result("rm"), rm) and np.array_equal(rvb2.result("rv"), rv) and int(batches2.result("b")[0]) == k


# ---- group 2: eval mode --------------------------------------------------------------------------------------------------------

def _bn_eval(dev, shape, relu, lead, affine=True):
    B, C, N = shape
    y, gamma, beta, rm, rv = P.eval_inputs(shape)
    yb, out, stat = _in(dev, y, lead), Box(dev, (B, C, N), lead=lead), Box(dev, (4, C))
    gb, bb = (_in(dev, gamma), _in(dev, beta)) if affine else (None, None)
    rmb, rvb = _in(dev, rm), _in(dev, rv)
    batches = Box(dev, (1,), dtype=torch.int64, lead=2, data=np.array([9]))
    _call("apn_pw_bn_act", dev, B, C, N, yb.ptr, None, 0, _p(gb), _p(bb), 0.0, P.MOMENTUM, 0, relu, rmb.ptr, rvb.ptr,
          batches.ptr, stat.ptr, out.ptr)
    want_stat, want = P.eval_ref(y, gamma if affine else None, beta if affine else None, rm, rv, relu)
    assert np.array_equal(stat.result("stat"), want_stat) and np.array_equal(out.result("out"), want)
    # the running buffers and the counter are untouched
    assert np.array_equal(rmb.result("rm"), rm) and np.array_equal(rvb.result("rv"), rv) and int(batches.result("b")[0]) == 9
    return stat, out


@pytest.mark.parametrize("relu", (0, 1))
@pytest.mark.parametrize("shape", P.EVAL_SHAPES, ids=P.grad_id)
def test_bn_act_eval(dev, shape, relu):
    stat, out = _bn_eval(dev, shape, relu, 4)
    _bn_eval(dev, shape, relu, 4, affine=False)
    if shape[2] % 4 == 0:
        # y and out one float into a parent: the scalar path, equal bits
        stat1, out1 = _bn_eval(dev, shape, relu, 1)
        assert torch.equal(stat1.t, stat.t) and torch.equal(out1.t, out.t)


# ---- group 3: BatchNorm's gradient ------------------------------------------------------------------------------------------------

def _bn_grad(dev, shape, relu, training, lead, sums=True):
    from adaptpoint_amd import _lib
    B, C, N = shape
    y, g, stat = P.grad_inputs(shape)
    yb, gb, sb = _in(dev, y, lead), _in(dev, g, lead), _in(dev, stat)
    splits = _lib.load().apn_pw_bn_act_grad_splits(B, C)
    assert splits == P.channel_splits(B, C)
    part_b = Box(dev, (splits, 2, C))
    gy, gg, gbeta = Box(dev, (B, C, N), lead=lead), Box(dev, (C,)), Box(dev, (C,))
    _call("apn_pw_bn_act_grad", dev, B, C, N, gb.ptr, yb.ptr, sb.ptr, training, relu, part_b.ptr, gy.ptr,
          gg.ptr if sums else None, gbeta.ptr if sums else None)
    assert part_b.intact()
    return gy, gg, gbeta


def _check_grad(shape, relu, training, gy, gg, gbeta, route):
    ref = P.grad_ref(*P.grad_inputs(shape), relu, training)
    assert np.array_equal(gg.result("g_gamma"), ref["g_gamma"]) and np.array_equal(gbeta.result("g_beta"), ref["g_beta"])
    got = gy.result("gy")
    if P.grad_exact(shape, training):
        assert np.array_equal(got, ref["gy"])                     # (the statement is a float32 number here: the CPU suite)
    else:
        bar = P.grad_bar(ref, P.grad_inputs(shape)[0])            # element-wise; derived at pointwise_cases.grad_bar
        err = np.abs(got - ref["gy"])
        assert (err <= bar).all(), (err / np.maximum(bar, 1e-300)).max()
        nzb = bar > 0
        if nzb.any():
            _note("gy |err| / grad_bar", (err[nzb] / bar[nzb]).max(), (P.grad_id(shape), relu, route))


@pytest.mark.parametrize("training", (0, 1))
@pytest.mark.parametrize("relu", (0, 1))
@pytest.mark.parametrize("shape", P.GRAD_SHAPES, ids=P.grad_id)
def test_bn_act_grad_on_both_routes(dev, shape, relu, training):
    fused = P.fused_route(shape)
    gy, gg, gbeta = _bn_grad(dev, shape, relu, training, 4)
    _check_grad(shape, relu, training, gy, gg, gbeta, "fused" if fused else "two-pass")
    # g_gamma = g_beta = null: the same gy, the two buffers untouched
    gy0, gg0, gbeta0 = _bn_grad(dev, shape, relu, training, 4, sums=False)
    assert torch.equal(gy0.t, gy.t) and gy0.intact() and gg0.untouched() and gbeta0.untouched()
    if fused:
        # g, y and gy one float into a parent: the alignment test sends the same values down the two-pass route
        gy1, gg1, gbeta1 = _bn_grad(dev, shape, relu, training, 1)
        _check_grad(shape, relu, training, gy1, gg1, gbeta1, "two-pass, unaligned")
        if P.grad_exact(shape, training):
            assert torch.equal(gy1.t, gy.t) and torch.equal(gg1.t, gg.t) and torch.equal(gbeta1.t, gbeta.t)


# ---- group 4: convolution + bias + ReLU + max ---------------------------------------------------------------------------------------

def _pool_cases():
    return [(s, k) for s in P.POOL_SHAPES for k in P.POOL_KINDS if P.pool_peaks(k, s[3]) is not None]


@pytest.mark.parametrize("precision", (2, 3))
@pytest.mark.parametrize("shape,kind", _pool_cases(), ids=lambda v: v if isinstance(v, str) else P.conv_id(v))
def test_conv_max_forward_and_the_tie_rule(dev, shape, kind, precision):
    from adaptpoint_amd import _lib
    B, C, O, N = shape
    x, w = P.pool_inputs(shape, kind)
    y = P.conv_ref(x, w)
    tiles = _lib.load().apn_pw_conv_max_tiles(N)
    want_tv, want_ti = P.pool_tiles_ref(y)
    assert want_tv.shape == (B, tiles, O)
    xb, wb = _in(dev, x), _in(dev, w)
    for bias in (None, P.pool_bias(shape, y)):
        for relu in (0, 1):
            tv, ti = Box(dev, (B, tiles, O)), Box(dev, (B, tiles, O), dtype=torch.int32)
            out, idx = Box(dev, (B, O)), Box(dev, (B, O), dtype=torch.int32)
            bb = None if bias is None else _in(dev, bias)
            _call("apn_pw_conv_max_forward", dev, B, C, O, N, precision, xb.ptr, wb.ptr, _p(bb), relu, tv.ptr, ti.ptr,
                  out.ptr, idx.ptr)
            want_out, want_idx = P.pool_ref(y, bias, relu)
            got_out, got_idx = out.result("out"), idx.result("idx")
            assert got_idx.min() >= 0 and got_idx.max() < N
            assert np.array_equal(got_idx, want_idx)                 # numpy's argmax: the first maximum
            assert np.array_equal(got_out, want_out)
            # the tiles' records: every real row written, each tile's maximum and its first position
            assert np.array_equal(tv.result("tile_val"), want_tv) and np.array_equal(ti.result("tile_idx"), want_ti)
            if kind == "negative" and bias is None:
                # a padded, zero-filled column that won the maximum would give 0 or an index >= N
                assert (got_out == 0).all() if relu else (got_out < 0).all()
            if kind == "equal":
                assert not got_idx.any()


# ---- group 5: the convolution + max backward ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("relu", (0, 1))
@pytest.mark.parametrize("shape", P.POOLBWD_SHAPES, ids=P.conv_id)
def test_conv_max_backward_on_a_supplied_idx(dev, shape, relu):
    """The raw entry on an idx of the test's own.  Every idx lies in [0, N): for an idx outside that range the entry leaves
    the row of xsel unwritten (and g_w then reads it) -- its documented contract, which the test does not probe."""
    B, C, O, N = shape
    x, w, g_out, out, idx = P.poolbwd_inputs(shape)
    assert idx.min() >= 0 and idx.max() < N
    xb, wb, gb, ob = (_in(dev, a) for a in (x, w, g_out, out))
    ib = Box(dev, (B, O), dtype=torch.int32, data=idx)
    want = P.poolbwd_ref(x, w, g_out, out, idx, relu)
    for full in (True, False):                                       # then with g_x = g_bias = null
        xsel, g_x, g_w, g_bias = Box(dev, (B, O, C)), Box(dev, (B, C, N)), Box(dev, (O, C)), Box(dev, (O,))
        _call("apn_pw_conv_max_backward", dev, B, C, O, N, gb.ptr, ob.ptr, ib.ptr, xb.ptr, wb.ptr, relu, xsel.ptr,
              g_x.ptr if full else None, g_w.ptr, g_bias.ptr if full else None)
        assert np.array_equal(xsel.result("xsel"), want[0])            # copied whatever the ReLU says
        assert np.array_equal(g_w.result("g_w"), want[2])
        if full:
            assert np.array_equal(g_x.result("g_x"), want[1])          # zeros WRITTEN where no channel picks
            assert np.array_equal(g_bias.result("g_bias"), want[3])
        else:
            assert g_x.untouched() and g_bias.untouched()


# ---- group 6: the gradient products and their operand set-up -----------------------------------------------------------------------

# every case aligned; three of them again with the operands one float into a parent (the scalar loaders)
_GRAD_PRODUCTS = [(s, 4) for s in P.CONV_SHAPES] + [(s, 1) for s in ((3, 32, 130, 128), (3, 33, 130, 129), (1, 1, 1, 1))]


@pytest.mark.parametrize("precision", (2, 3))
@pytest.mark.parametrize("shape,lead", _GRAD_PRODUCTS, ids=[P.conv_id(s) + ("" if l == 4 else "-one-float-off") for s, l in _GRAD_PRODUCTS])
def test_conv_gradient_products(dev, shape, lead, precision):
    from adaptpoint_amd import _lib
    B, C, O, N = shape
    x, w = P.conv_inputs(shape)
    gy = P.conv_grad_inputs(shape)
    want_gx, want_gw = P.conv_grad_ref(x, w, gy)
    xb, wb, gyb = _in(dev, x, lead), _in(dev, w, lead), _in(dev, gy, lead)
    gx = Box(dev, (B, C, N))
    _call("apn_pw_conv_grad_input", dev, B, C, O, N, precision, gyb.ptr, wb.ptr, gx.ptr)
    assert np.array_equal(gx.result("gx"), want_gx)
    splits = _lib.load().apn_pw_conv_grad_weight_splits(B, C, O, N)
    assert splits >= 1
    scratch, gw = Box(dev, (splits, O, C)), Box(dev, (O, C))          # the scratch: sized by the helper, only the result is read
    _call("apn_pw_conv_grad_weight", dev, B, C, O, N, precision, gyb.ptr, xb.ptr, scratch.ptr, gw.ptr)
    assert np.array_equal(gw.result("gw"), want_gw) and scratch.intact()


def test_zz_report_the_worst_values(dev):
    for name in sorted(WORST):
        print("MEASURED %-32s %.4g  %s" % (name, WORST[name][0], WORST[name][1]))
