"""The kernels of csrc/edge_conv.hip through their raw entries -- apn_ec_csr, apn_ec_pool_fwd (+ apn_la_stats_fold),
apn_ec_out_res, apn_ec_bwd_prep_act, apn_ec_pool_bwd, and the slope-guarded apn_ec_out / apn_ec_bwd_prep -- on the problems
of tests/edge_conv_cases.py against its reference (tests/test_edge_conv_cases_cpu.py checks both on the CPU).

Four kinds of check:
  exact       integer-valued inputs on which every float32 step of every kernel is exact: every output of the chain
              csr -> pool_fwd -> out_res -> bwd_prep_act -> pool_bwd, each stage reading the previous kernel's own output,
              must EQUAL the reference -- no tolerance -- in training and in eval mode, at every width, every way the
              loop over K ends, on kNN-like graphs, on ties between different neighbours, on reverse lists of chosen
              lengths and on indices outside the cloud (which must give what the host-clamped idx gives);
  float       Gaussian inputs: ext, sel, ysum, the eval-mode duv and each list's sum of u equal a float32 restatement
              bit for bit; the rest stays within element-wise bars derived from the arithmetic
              (edge_conv_cases.float_bars);
  containment every input lies in a NaN-filled parent (the pad columns of uv are NaN as well), every output in a
              sentinel-filled one (every raw call in this file): no sentinel outside changes, none inside is left
              (sel byte by byte, part double by double), no NaN comes out;
  invariants  results that must agree bit for bit: two runs, a cloud alone, the row pitch, the guarded entries at
              H = 512, a channel tile alone, power-of-two scaling of g.

No index leaves the arrays on the outside cases: ec_pool_fwd_kernel reads idx only at gq * K + lane with lane < K and
gq < nq, brings the value into [0, n - 1] with two comparisons that hold for every int32 (INT32_MIN < 0, INT32_MAX >= n)
before it is added to the cloud's first point (gq / n) * n <= nq - n, and ec_target applies the same two comparisons to
idx[pos], pos < npos, before adding ((pos / K) / n) * n: both addresses lie in [0, B N).

The measured worst ratios to the bars, the file's wall time and the mutation check stand below the imports; test_zz
prints the ratios for a whole-file run.
"""
import pytest
import torch

import edge_conv_cases as C
from attention_cases import SENTINEL, borders_intact, in_nan_parent, in_sentinel_parent

pytestmark = pytest.mark.gpu

# Measured on an MI355X (whole-file run), worst |kernel - float64| / bar over the twelve float cases:
#   out        0.981 (H128-B3N77-K20)    out_nores  0.998 (H256-B2N65-K64)    gsel   0.997 (H512-B3N77-K20)
#   partS      0.040 (H512-B2N65-K5)     part2      0.042 (H512-B2N65-K64)    duv    0.504 (H512-B2N65-K5, training mode)
#   part1, fold  0.000 (exact in float64)
# out, out_nores (the same entry with res = NULL) and gsel sit just below 1 because their bars count only the roundings
# that happen -- one where z > 0, two where the slope multiplies, one more for a residual -- at half an ulp each, and
# among 10^5 elements some come close to every worst case at once.  ext, sel, ysum, the eval-mode duv and the lists'
# sums of u matched the float32 restatement bit for bit, and all 123 exact cases matched the reference with no
# tolerance, H = 512 included: the kernels needed no change.
# Wall time of this file on an MI355X: 5 s (145 tests; 4.7, 5.2 and 5.4 s in three runs; the slowest test 0.4 s: the
# first one, which loads the library).  The GPU suite as it stood before -- this file and the new SHAPES row of
# tests/test_gpu_edge_conv.py left out, 1204 tests -- took 204 s in the same visit.
# Mutation check (each mutation of csrc/edge_conv.hip built into a scratch library, arithmetic only -- none can read or
# write outside an array; tests failing in this file / in tests/test_gpu_edge_conv.py, each file run once per library):
#   `t > best` -> `t >=`  (the LAST slot among equals)                      107 / 0
#   sg forced to 1  (the maximum under a negative gamma)                      56 / 1
#   the forward's `if (k + g >= K) break` removed                             94 / 1
#   the backward's `if (j + t >= chunk) break` removed                       132 / 10
#   du: `(float)K * E` -> `fc * E`                                           126 / 8
#   dv: `fc * E` -> `(float)K * E`                                           126 / 8
#   ec_act_slope: `z > 0.0f` -> `z >= 0.0f`                                  121 / 0
#   ec_bwd_prep: `tile[tx][pp]` -> `tile[pp][tx]`                            123 / 10
#   the partS row taken as blockIdx.x * gridDim.z + b                        112 / 0
#   ec_target: `n - 1` -> `0` for nb >= n  (the backward's clamp alone)       33 / 0
#   s2 accumulated from y instead of y * y                                   136 / 9
# Four of the eleven pass the older file untouched: which of two equal neighbours wins (only the exact cases see it: no
# float case has a tie), the activation's slope at z == 0, the order of the partS rows (their sum is all the module
# uses) and a backward clamp that differs from the forward's.

F32, F64 = torch.float32, torch.float64
SENTINEL64 = (SENTINEL << 32) | SENTINEL
WORST = {}                      # quantity -> [worst ratio to its bar, case]


def _call(*a):
    from adaptpoint_amd.fused import _call as call
    return call(*a)


# ---- poisoned buffers ---------------------------------------------------------------------------------------------------

def _in(dev, t):
    """A float32 input as a contiguous view into a NaN-filled parent on the device."""
    return in_nan_parent(t.to(dev))


def _in_int(dev, t):
    """An int32 input inside a NaN-filled parent (read as int32 the NaN is 0x7fc00000, an index far outside any cloud)."""
    view = in_nan_parent(torch.zeros(t.numel(), device=dev)).view(torch.int32)
    view.copy_(t.reshape(-1).to(dev))
    return view.view(t.shape)


class _Outputs:
    """The output buffers of one raw call, each in a sentinel-filled parent."""

    def __init__(self, dev):
        self.dev, self.bufs = dev, {}

    def new(self, name, shape, dtype, inside=True):
        size = {torch.uint8: 1, torch.float64: 8}.get(dtype, 4)
        n = 1
        for s in shape:
            n *= s
        view, parent = in_sentinel_parent((n * size + 3) // 4 * 4, self.dev)
        if dtype == torch.uint8:
            assert n % 4 == 0                                # (H is a multiple of 64: no padding bytes behind the tensor)
            view.fill_(-1)                                   # 0xff in every byte: no slot (sel < 64) takes it
        assert view.data_ptr() % 16 == 0 and view.data_ptr() != parent.data_ptr()
        self.bufs[name] = (view, parent, shape, dtype, inside)
        return view.data_ptr()

    def checked(self, what):
        """The containment assertions; -> {name: tensor}."""
        res = {}
        for name, (view, parent, shape, dtype, inside) in self.bufs.items():
            assert borders_intact(parent), f"{what}: {name}: a sentinel outside the buffer changed"
            if dtype == torch.uint8:
                t = view.view(torch.uint8)[:int(torch.tensor(shape).prod())].view(shape)
                written = bool((t != 0xFF).all())
            elif dtype == F64:
                t = view.view(F64).view(shape)
                written = bool((view.view(torch.int64) != SENTINEL64).all())
            else:
                t = view.view(dtype).view(shape)
                written = bool((view != SENTINEL).all())
            if inside:
                assert written, f"{what}: {name}: a part of the buffer was never written"
            if dtype.is_floating_point:
                assert not bool(torch.isnan(t).any()), f"{what}: {name}: a NaN came out"
            res[name] = t
        return res


# ---- the raw entries ----------------------------------------------------------------------------------------------------

def ec_csr(dev, idx):
    B, N, K = idx.shape
    o = _Outputs(dev)
    args = [o.new("pcnt_poff", (2, B * N), torch.int32), o.new("plist", (B * N * K,), torch.int32),
            o.new("scratch", (B * N * (K + 1),), torch.int32, inside=False)]
    _call("apn_ec_csr", dev, B, N, K, idx.data_ptr(), *args)
    return o.checked("apn_ec_csr")


def ec_pool_fwd(dev, uv, H, idx, gamma, train):
    from adaptpoint_amd import _lib
    B, N, K = idx.shape
    o = _Outputs(dev)
    ext, sel = o.new("ext", (B, N, H), F32), o.new("sel", (B, N, H), torch.uint8)
    ysum = part = None
    if train:
        rows = _lib.load().apn_ec_pool_rows(B, N)
        ysum, part = o.new("ysum", (B, N, H), F32), o.new("part", (rows, 2 * H), F64)
    _call("apn_ec_pool_fwd", dev, B, N, H, K, uv.data_ptr(), uv.shape[2], idx.data_ptr(),
          None if gamma is None else gamma.data_ptr(), ext, sel, ysum, part)
    return o.checked("apn_ec_pool_fwd")


def stats_fold(dev, part, count):
    rows, H = part.shape[0], part.shape[1] // 2
    o = _Outputs(dev)
    _call("apn_la_stats_fold", dev, part.data_ptr(), rows, H, float(count), o.new("sums", (2 * H + 2,), F64))
    return o.checked("apn_la_stats_fold")["sums"]


def ec_out(dev, ext, pack, slope, res, entry="apn_ec_out_res"):
    B, N, H = ext.shape
    o = _Outputs(dev)
    out = o.new("out", (B, H, N), F32)
    if entry == "apn_ec_out":
        _call(entry, dev, B, N, H, ext.data_ptr(), pack.data_ptr(), slope, out)
    else:
        rs = (0, 0, 0) if res is None else res.stride()
        _call(entry, dev, B, N, H, ext.data_ptr(), pack.data_ptr(), slope, None if res is None else res.data_ptr(), *rs, out)
    return o.checked(entry)["out"]


def ec_bwd_prep(dev, g, ext, pack, slope, entry="apn_ec_bwd_prep_act"):
    from adaptpoint_amd import _lib
    B, N, H = ext.shape
    rows = _lib.load().apn_ec_bwd_prep_rows(B, N)
    o = _Outputs(dev)
    gsel, partS = o.new("gsel", (B, N, H), F32), o.new("partS", (rows, 2 * H), F32)
    _call(entry, dev, B, N, H, g.data_ptr(), *g.stride(), ext.data_ptr(), pack.data_ptr(), slope, gsel, partS)
    return o.checked(entry)


def ec_pool_bwd(dev, gsel, sel, pcnt_poff, plist, uv, K, ysum, de):
    B, N, H = gsel.shape
    o = _Outputs(dev)
    duv = o.new("duv", (B, N, 2 * H), F32)
    _call("apn_ec_pool_bwd", dev, B, N, H, K, gsel.data_ptr(), sel.data_ptr(), pcnt_poff.data_ptr(), plist.data_ptr(),
          uv.data_ptr(), uv.shape[2], None if ysum is None else ysum.data_ptr(), de.data_ptr(), duv)
    return o.checked("apn_ec_pool_bwd")["duv"]


def _laid_out(dev, t, layout):
    """t (B,H,N) on the device in a NaN-filled parent, as its layout says: contiguous; a permuted view of a (B,N,H)
    buffer; one cloud expanded over the batch (batch stride 0); one scalar expanded (every stride 0)."""
    if t is None or layout == "none":
        return None
    if layout == "permuted":
        v = _in(dev, t.permute(0, 2, 1).contiguous()).permute(0, 2, 1)
        assert not v.is_contiguous() or 1 in v.shape
        return v
    if layout == "expanded":
        assert bool((t == t[:1]).all())
        v = _in(dev, t[:1].contiguous())
        return v.as_strided(t.shape, (0,) + v.stride()[1:])
    if layout == "scalar":
        assert bool((t == t.reshape(-1)[0]).all())
        return _in(dev, t.reshape(-1)[:1].contiguous()).as_strided(t.shape, (0, 0, 0))
    return _in(dev, t.contiguous())


def _chain(dev, H, inp, train, g_layout="contiguous", res_layout="contiguous", idx=None, de=None):
    """csr -> pool_fwd (-> stats_fold) -> out_res -> bwd_prep_act -> pool_bwd, each stage on the previous kernel's own
    output.  Eval mode: ysum = part = NULL and de = 0.  `de` may be a function of partS (the float cases).  -> dict."""
    idx = inp["idx"] if idx is None else idx
    B, N, K = idx.shape
    d_idx, d_uv = _in_int(dev, idx), _in(dev, inp["uv"])
    gamma = None if inp["gamma"] is None else _in(dev, inp["gamma"])
    pack = _in(dev, inp["pack"])
    got = dict(ec_csr(dev, d_idx))
    got.update(ec_pool_fwd(dev, d_uv, H, d_idx, gamma, train))
    if train:
        got["sums"] = stats_fold(dev, got["part"], B * N * K)
    got["out"] = ec_out(dev, got["ext"], pack, inp["slope"], _laid_out(dev, inp["res"], res_layout))
    got.update(ec_bwd_prep(dev, _laid_out(dev, inp["g"], g_layout), got["ext"], pack, inp["slope"]))
    if not train:
        de = torch.zeros(2 * H)
    elif de is None:
        de = inp["de"]
    elif callable(de):
        de = de(got["partS"].cpu())
    got["de"] = de
    got["duv"] = ec_pool_bwd(dev, got["gsel"], got["sel"], got["pcnt_poff"], got["plist"], d_uv, K,
                             got["ysum"] if train else None, _in(dev, de))
    return got


CHAIN_OUTPUTS = ("pcnt_poff", "plist", "ext", "sel", "ysum", "part", "sums", "out", "gsel", "partS", "duv")


def _same(a, b, names=CHAIN_OUTPUTS):
    return [n for n in names if n in a and not torch.equal(a[n], b[n])]


# ---- exact --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", C.CASES, ids=C.CASE_IDS)
def test_exact_cases_through_the_chain(dev, case):
    """Every output of every entry EQUALS the reference, training and eval mode; on the outside cases the chain on the
    host-clamped idx gives the same bits."""
    B, N, H, K = case.B, case.N, case.H, case.K
    inp = C.exact_inputs(case)
    want = C.expected(case, inp)
    for train in (True, False):
        got = _chain(dev, H, inp, train, case.g, case.res)
        eq = lambda name, ref: torch.equal(got[name].cpu().double(), ref.double())
        assert eq("pcnt_poff", torch.stack([want["pcnt"], want["poff"]])), (train, "pcnt_poff")
        assert eq("plist", want["plist"]), (train, "plist")
        names = ["ext", "sel", "out", "gsel", "partS"] + (["ysum", "part"] if train else [])
        for name in names:
            assert eq(name, want[name]), (train, name)
        assert eq("duv", want["duv"] if train else want["duv_eval"]), (train, "duv")
        if train:
            sums = torch.cat([want["part"].sum(0), torch.tensor([float(B * N * K), 1.0], dtype=F64)])
            assert eq("sums", sums), "apn_la_stats_fold"
        else:
            assert "ysum" not in got and "part" not in got
            assert torch.equal(got["duv"][..., :H], got["gsel"])
        if case.kind == "outside":
            assert not bool(((inp["idx"] >= 0) & (inp["idx"] < N)).all())
            inside = _chain(dev, H, inp, train, case.g, case.res, idx=C.clamped(inp["idx"]))
            assert not _same(got, inside), (train, "idx clamped on the host")


@pytest.mark.parametrize("shape", C.CSR_ONLY, ids=lambda s: "x".join(map(str, s)))
def test_reverse_lists_of_clouds_above_1024_points(dev, shape):
    """csr_scan_kernel with 2, 3 and 1 points per thread; indices outside the cloud among them."""
    B, N, K = shape
    idx = C.outside_graph(B, N, K, torch.Generator().manual_seed(N))
    got = ec_csr(dev, _in_int(dev, idx))
    pcnt, poff, plist = C.csr(idx)
    assert torch.equal(got["pcnt_poff"].cpu(), torch.stack([pcnt, poff]))
    assert torch.equal(got["plist"].cpu(), plist)


# ---- float --------------------------------------------------------------------------------------------------------------

def _ratio(case, name, got, ref, bar):
    r = float(((got.double().cpu() - ref).abs() / bar.clamp_min(1e-300)).max())
    w = WORST.setdefault(name, [0.0, ""])
    if r > w[0]:
        w[0], w[1] = r, case.name
    print(f"{case.name} {name}: worst |kernel - float64| / bar {r:.3f}")
    return r


@pytest.mark.parametrize("case", C.FLOAT, ids=C.FLOAT_IDS)
def test_float_cases(dev, case):
    """Bit for bit against the float32 restatement: ext, sel, ysum (one IEEE add per y, slot order) and the eval-mode duv
    (list order).  Element-wise against float64 within the derived bars: the y^2 sums, out, gsel, partS, the
    training-mode duv, the fold.  Each reference takes the kernels' own float32 outputs of the stage before."""
    B, N, H, K = case.B, case.N, case.H, case.K
    inp = C.float_inputs(case)
    got = _chain(dev, H, inp, True, de=lambda partS: C.float_dense(inp, partS))
    cpu = {n: t.cpu() for n, t in got.items() if torch.is_tensor(t)}
    ext, sel, ysum, p1, p2 = C.pool_fwd(inp["uv"], H, inp["idx"], inp["gamma"], dtype=F32)
    assert torch.equal(cpu["ext"], ext) and torch.equal(cpu["sel"], sel) and torch.equal(cpu["ysum"], ysum)
    bars = C.float_bars(H, K, inp["idx"], inp["uv"], inp["pack"], inp["slope"], inp["res"], inp["g"], cpu["ext"], cpu["gsel"],
                        cpu["sel"], cpu["ysum"], got["de"])
    gsel, partS = C.bwd_prep(inp["g"], cpu["ext"], inp["pack"], inp["slope"])
    checks = [("part1", cpu["part"][:, :H], p1, bars["part1"]), ("part2", cpu["part"][:, H:], p2, bars["part2"]),
              ("out", cpu["out"], C.out(cpu["ext"], inp["pack"], inp["slope"], inp["res"]), bars["out"]),
              ("out_nores", ec_out(dev, got["ext"], _in(dev, inp["pack"]), inp["slope"], None).cpu(),
               C.out(cpu["ext"], inp["pack"], inp["slope"], None), bars["out_nores"]),
              ("gsel", cpu["gsel"], gsel, bars["gsel"]), ("partS", cpu["partS"], partS, bars["partS"]),
              ("duv", cpu["duv"], C.pool_bwd(cpu["gsel"], cpu["sel"], inp["idx"], inp["uv"], H, cpu["ysum"], got["de"]), bars["duv"])]
    fold = cpu["part"].sum(0)
    checks.append(("fold", cpu["sums"][:2 * H], fold, cpu["part"].abs().sum(0) * 2.0 ** -40))
    bad = [(name, r) for name, r in ((name, _ratio(case, name, a, b, bar)) for name, a, b, bar in checks) if not r <= 1.0]
    assert not bad, (case.name, bad)
    assert cpu["sums"][2 * H:].tolist() == [float(B * N * K), 1.0]
    ev = _chain(dev, H, inp, False)
    assert not _same(got, ev, ("ext", "sel", "out", "gsel", "partS", "pcnt_poff", "plist"))
    want = C.pool_bwd(cpu["gsel"], cpu["sel"], inp["idx"], inp["uv"], H, None, torch.zeros(2 * H), dtype=F32)
    assert torch.equal(ev["duv"].cpu(), want), "eval-mode duv: acc in list order"
    # the list's sum of u alone: gsel = 0, v = 0, D = 1, E = 0 leave du = ysum and dv = fma(1, fma(cnt, 0, us), 0) = us
    uv0 = inp["uv"].clone()
    uv0[..., H:2 * H] = 0.0
    zero, de1 = torch.zeros(B, N, H), torch.cat([torch.ones(H), torch.zeros(H)])
    us = ec_pool_bwd(dev, _in(dev, zero), got["sel"], got["pcnt_poff"], got["plist"], _in(dev, uv0), K, got["ysum"], _in(dev, de1))
    want = C.pool_bwd(zero, cpu["sel"], inp["idx"], uv0, H, cpu["ysum"], de1, dtype=F32)
    assert torch.equal(us.cpu(), want) and torch.equal(us[..., :H], got["ysum"]), "the list's sum of u in list order"


# ---- invariants ---------------------------------------------------------------------------------------------------------

INVARIANT = [C.Float("inv-H64", 31, 3, 77, 64, 20), C.Float("inv-H128", 32, 2, 128, 128, 33),
             C.Float("inv-H256", 33, 3, 77, 256, 7), C.Float("inv-H512", 34, 2, 65, 512, 64)]


@pytest.mark.parametrize("case", INVARIANT, ids=[c.name for c in INVARIANT])
def test_bit_level_invariants(dev, case):
    """Two runs; cloud b alone against cloud b inside the batch, all five entries; ld = 2H against the padded pitches;
    g scaled by 2^+-7 scales gsel, partS and the eval-mode duv -- all bit for bit."""
    B, N, H, K = case.B, case.N, case.H, case.K
    inp = C.float_inputs(case)
    inp["de"] = torch.randn(2 * H, generator=torch.Generator().manual_seed(case.seed)) * 0.01
    full = _chain(dev, H, inp, True, res_layout="permuted", g_layout="permuted")
    assert not _same(full, _chain(dev, H, inp, True, res_layout="permuted", g_layout="permuted")), "two runs"
    assert not _same(full, _chain(dev, H, inp, True)), "g and the residual by strides"
    tiles, NK = (N + 63) // 64, N * K
    for b in sorted({0, B - 1}):
        one = dict(inp, uv=inp["uv"][b:b + 1], idx=inp["idx"][b:b + 1], g=inp["g"][b:b + 1], res=inp["res"][b:b + 1])
        alone = _chain(dev, H, one, True)
        for name in ("ext", "sel", "ysum", "out", "gsel", "duv"):
            assert torch.equal(alone[name][0], full[name][b]), ("cloud", b, name)
        assert torch.equal(alone["partS"], full["partS"][b * tiles:(b + 1) * tiles]), ("cloud", b, "partS")
        assert torch.equal(alone["pcnt_poff"][0], full["pcnt_poff"][0, b * N:(b + 1) * N]), ("cloud", b, "pcnt")
        assert torch.equal(alone["pcnt_poff"][1] + b * NK, full["pcnt_poff"][1, b * N:(b + 1) * N]), ("cloud", b, "poff")
        assert torch.equal(alone["plist"] + b * NK, full["plist"][b * NK:(b + 1) * NK]), ("cloud", b, "plist")
        if N % 64 == 0:
            assert torch.equal(alone["part"], full["part"][b * N // 64:(b + 1) * N // 64]), ("cloud", b, "part")
    for pad in (0, 64):
        uv = torch.full((B, N, 2 * H + pad), float("nan"))
        uv[..., :2 * H] = inp["uv"][..., :2 * H]
        assert not _same(full, _chain(dev, H, dict(inp, uv=uv), True)), ("ld", 2 * H + pad)
    ev = _chain(dev, H, inp, False)
    for s in (-7, 7):
        scaled = _chain(dev, H, dict(inp, g=inp["g"] * 2.0 ** s), False)
        for name in ("gsel", "partS", "duv"):
            assert torch.equal(scaled[name], ev[name] * 2.0 ** s), ("g scaled", s, name)
        assert not _same(scaled, ev, ("ext", "sel", "out"))


def test_the_slope_guarded_entries_equal_the_general_ones_at_the_widest_kernels(dev):
    """apn_ec_out against apn_ec_out_res(res = NULL), apn_ec_bwd_prep against apn_ec_bwd_prep_act, H = 512 (eight channel
    tiles), N = 65: the pair test of tests/test_gpu_edge_conv.py (H = 128) at the widest width."""
    inp = C.float_inputs(C.Float("pair", 41, 2, 65, 512, 5))
    H = 512
    pack = _in(dev, inp["pack"])
    ext = ec_pool_fwd(dev, _in(dev, inp["uv"]), H, _in_int(dev, inp["idx"]), _in(dev, inp["gamma"]), False)["ext"]
    assert torch.equal(ec_out(dev, ext, pack, 0.2, None, "apn_ec_out"), ec_out(dev, ext, pack, 0.2, None))
    g = _laid_out(dev, inp["g"], "permuted")
    a, b = (ec_bwd_prep(dev, g, ext, pack, 0.2, entry) for entry in ("apn_ec_bwd_prep", "apn_ec_bwd_prep_act"))
    assert torch.equal(a["gsel"], b["gsel"]) and torch.equal(a["partS"], b["partS"])


def test_a_channel_tile_alone_equals_the_tile_inside_the_full_width(dev):
    """ec_out and ec_bwd_prep at H = 64 on the columns [64 t, 64 t + 64) of an H = 256 problem."""
    case = C.Float("tile", 42, 3, 77, 256, 5)
    inp = C.float_inputs(case)
    H = 256
    full = _chain(dev, H, inp, False, res_layout="permuted")
    for t in range(4):
        cols = slice(64 * t, 64 * t + 64)
        ext = _in(dev, full["ext"][..., cols].contiguous())
        pack = _in(dev, torch.cat([inp["pack"][i * H:(i + 1) * H][cols] for i in range(4)]))
        res = _laid_out(dev, inp["res"][:, cols], "permuted")
        assert torch.equal(ec_out(dev, ext, pack, inp["slope"], res), full["out"][:, cols]), t
        got = ec_bwd_prep(dev, _laid_out(dev, inp["g"][:, cols], "contiguous"), ext, pack, inp["slope"])
        assert torch.equal(got["gsel"], full["gsel"][..., cols]), t
        assert torch.equal(got["partS"][:, :64], full["partS"][:, cols]), t
        assert torch.equal(got["partS"][:, 64:], full["partS"][:, H + 64 * t:H + 64 * t + 64]), t


def test_zz_worst_figures_of_this_run(dev):
    """A printing aid, after the pattern of tests/test_gpu_attention_cases.py: the worst ratio to each bar over whatever
    float cases ran before it in this process (the table in the header comes from a whole-file run).  It asserts
    nothing new -- test_float_cases has asserted every ratio already -- and nothing at all when no float case ran."""
    for name, (ratio, at) in sorted(WORST.items()):
        print(f"MEASURED {name:>6}: worst |kernel - float64| / bar {ratio:.3f} ({at})")
        assert ratio <= 1.0, (name, at)
