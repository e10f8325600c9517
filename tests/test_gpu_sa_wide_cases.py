"""The per-position kernels of csrc/sa_wide.hip through their raw entries -- apn_sa_wide_stats1, apn_sa_wide_fwd_main,
apn_sa_wide_bwd_main, apn_sa_wide_wgrad, with apn_sa_wide_image beside them -- on the exact cases of
tests/sa_wide_cases.py (tests/test_sa_wide_cases_cpu.py checks the cases and the statement on the CPU).

Every case is integer valued, so every output is compared with the float64 statement BIT FOR BIT (torch.equal, no
tolerance): the partial rows through their float64 column sum, after every one of them turned out finite -- each output
buffer is filled with NaN (ksel with 0xEE) before the call, so a row, an element or a whole idle workgroup's partial row
left unwritten shows, and so does a write to a padding row of GU or behind the tiles in use.  The weight images come from
`fused_wide.mfma_b_image`, the tile map from `fused_wide.tile_map` (asserted equal to the blob of sa_wide_cases on every
field the kernels read); ksel and goa of the backward entries are the case's own, not a forward run's.

Which variant of a kernel a width runs (the constexpr selectors of csrc/sa_wide.hip; RES: the whole weight image resident
in LDS, else two streaming slots fed through the cyclic chunk sequence; AHEADA: a1's rows requested one chunk step ahead;
OCC: waves per SIMD; WG: the weight-gradient products fused into the backward pass):

    H     stats1     fwd_main                    bwd_main                        wgrad
    32    PP 2 CPL 1 CT 2 RES                    CT 1 RES OCC 2 WG               (fused)
    64    PP 1 CPL 1 CT 4 RES                    CT 2 RES OCC 2                  6 waves, 1 row group
    128   PP 1 CPL 2 CT 4 streaming AHEADA       CT 4 streaming (NCB 1) OCC 1    8 waves, 2 row groups
    256   PP 1 CPL 4 CT 4 streaming AHEADA       CT 4 streaming (NCB 2) OCC 1    8 waves, 3 row groups

so `rounds` (2200 tiles on 2048 waves: 152 waves take a second tile) crosses a tile boundary in the resident form (32) and
in both streaming forms (128: one column block, the sequence wraps within it; 256: two), `rounds_folded` leaves 374 of 512
workgroups idle at 64, and `one`, `mixed`, `whole` run every variant on single, packed and whole-query tiles.

One float case per width keeps the split-operand path honest where lo parts are not zero: see
test_float_case_stays_within_the_derived_bars.  MEASURED holds what an MI355X gave (documentation, not asserted).
"""
import functools

import numpy as np
import pytest
import torch

import sa_wide_cases as C

pytestmark = pytest.mark.gpu

F32, U8 = torch.float32, torch.uint8
EINVAL = -1

# Measured on an MI355X: worst |kernel - float64| / bar of the float case per width -- pool: ysel (the same over the decided
# entries and over all of them), stat: sum y2 per channel; left_out: the share of pooled values the gap rule leaves out.
MEASURED = {
    32: dict(pool=0.251, stat=0.054, left_out=0.0006),
    64: dict(pool=0.242, stat=0.043, left_out=0.0006),
    128: dict(pool=0.150, stat=0.030, left_out=0.0011),
    256: dict(pool=0.085, stat=0.021, left_out=0.0014),
}
# All 66 exact comparisons matched the statement with no tolerance: csrc/sa_wide.hip needed no change.  Wall time of this
# file on an MI355X: 3.5 s (75 tests; the slowest 0.6 s: the first one, which loads the library).
# Mutation check (each mutation of csrc/sa_wide.hip built into a scratch library; arithmetic, selection, or a read of
# another chunk of the same image -- none leaves a buffer; tests failing in this file, of 75 / in
# tests/test_gpu_fused_wide.py, of 36):
#   pool, between the lane halves: `op < bslot` -> `op > bslot`                              10 / 0
#   pool, within a lane half: `v[i] > best` -> `>=`  (the last row among equals)            14 / 0
#   fwd_main: sum y2 without the multiplicity                                               13 / 23
#   fwd_main, streaming: the prefetch at the wrap asks for the last chunk again, not chunk 0  2 / 0   (rounds at 128, 256)
#   fwd_main: a workgroup without a tile leaves its partial row unwritten                     9 / 21
#   bwd_main: GU written on padding rows as well                                            25 / 18
#   bwd_main: evec added once per row, not once per position                                 9 / 15
#   Gram and suma without the multiplicity (bwd_main at 32, wgrad)                          11 / 13
#   bwd_main, streaming: the chunk behind the last one of a tile is the last one again       4 / 0   (rounds at 128, 256)
#   stats1 without the multiplicity                                                          9 / 9
#   bwd_main: HB without the multiplicity                                                   18 / 14
#   bwd_main: every cloud reads cloud 0's rows of U                                         20 / 16
# The module test is blind to both tie rules (its inputs never tie) and to both prefetches at the wrap (none of its waves
# takes a second tile); this file sees every one of the twelve and names the entry, the case and the width.


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _call(name, *args):
    from adaptpoint_amd.fused import _call as call
    call(name, _dev(), *args)


def _lib():
    from adaptpoint_amd import _lib
    return _lib.load()


def _f32(a):
    return torch.as_tensor(np.array(a), device=_dev()).to(F32).contiguous()


def _poison(*shape):
    return torch.full(shape, float("nan"), dtype=F32, device=_dev())


@functools.lru_cache(maxsize=None)
def _reference(name, H):
    """The checked case and its statement, evaluated once in float64 on the device: (inp, fwd, bwd, bwd without evec)."""
    inp, fwd, bwd, bwd0 = C.inputs(name, H, _dev())
    for b in (bwd, bwd0):
        assert torch.equal(b["GU"].float().double(), b["GU"])
        b["GU"] = b["GU"].float()
    return inp, fwd, bwd, bwd0


def _on_device(inp):
    """The operands of a case as the entries take them; the tile map built by the device, equal to the case's blob."""
    from adaptpoint_amd import fused_wide as FW
    H, O, B, M = inp["H"], inp["O"], inp["B"], inp["M"]
    d = {k: _f32(inp[k]) for k in ("U", "V", "pack1", "sgn2", "W2", "Qm", "evec", "goa")}
    d["idx"] = torch.as_tensor(np.array(inp["idx"]), device=_dev()).to(torch.int32).contiguous()
    d["ksel"] = torch.as_tensor(np.array(inp["ksel"]), device=_dev()).to(U8).contiguous()
    d["tmap"] = FW.tile_map(d["idx"], inp["fold"])
    lay = C.layout(inp["name"])
    got, blob, nt, bm = d["tmap"].cpu().numpy(), lay["blob"], lay["tm"]["nt"], B * M
    rows_off = 4 + ((bm + 3) & ~3)
    assert got.size >= blob.size and got[0] == blob[0] == nt
    for start, n in ((4, nt), (rows_off, 32 * nt), (rows_off + 32 * bm, 32 * nt)):          # tq0, rowinfo, rownn
        assert np.array_equal(got[start:start + n], blob[start:start + n]), start
    d["w2img"] = FW.mfma_b_image(d["W2"].t().contiguous(), min(4, O // 32))                  # W2^T (H x O)
    d["zimg"] = FW.mfma_b_image(torch.cat([d["W2"], d["Qm"]], 0).contiguous(), min(4, H // 32))     # [W2 ; Qm]
    d["grid"] = _lib().apn_sa_wide_grid(B, M)
    d["dims"] = (B, inp["N"], M, H)
    return d


@functools.lru_cache(maxsize=None)
def _operands(name, H):
    return _on_device(_reference(name, H)[0])


def _exact_rows(part, want, what):
    """Every partial row written and finite; their float64 column sum IS the statement."""
    assert bool(torch.isfinite(part).all()), what + ": a partial row (or a part of one) was left unwritten"
    assert torch.equal(part.double().sum(0), want), what


def _geometry(d):
    return [d["U"].data_ptr(), d["V"].data_ptr(), d["idx"].data_ptr(), d["tmap"].data_ptr()]


# ---- the weight images --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H", C.WIDTHS)
def test_image_is_byte_equal_to_the_tensor_statement_of_the_layout(H):
    from adaptpoint_amd import fused_wide as FW
    O, dev = 2 * H, _dev()
    g = torch.Generator(dev).manual_seed(H)
    W2, Qm = torch.randn(O, H, device=dev, generator=g), torch.randn(H, H, device=dev, generator=g)
    for src0, k0, trans0, src1, kd, nc, Bm in ((W2, H, 1, None, H, O, W2.t().contiguous()),
                                               (W2, O, 0, Qm, O + H, H, torch.cat([W2, Qm], 0).contiguous())):
        ct = min(4, nc // 32)
        img = torch.full((nc // (32 * ct), kd // 32, ct, 2, 2, 64, 8), float("nan"), dtype=torch.bfloat16, device=dev)
        _call("apn_sa_wide_image", src0.data_ptr(), k0, trans0, None if src1 is None else src1.data_ptr(), kd, nc, ct,
              img.data_ptr())
        want = FW.mfma_b_image(Bm, ct).contiguous()
        assert want.numel() == img.numel()
        assert torch.equal(img.view(torch.int16).reshape(-1), want.view(torch.int16).reshape(-1)), (H, kd, nc)


# ---- the four entries on the exact cases ------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,H", C.PAIRS)
def test_stats1_partial_rows_sum_to_the_statement(name, H):
    d, fwd = _operands(name, H), _reference(name, H)[1]
    part = _poison(d["grid"], 2 * H)
    _call("apn_sa_wide_stats1", *d["dims"], *_geometry(d), part.data_ptr())
    _exact_rows(part, fwd["stats1"], "stats1")


@pytest.mark.parametrize("name,H", C.PAIRS)
def test_fwd_main_pool_slots_and_statistics_equal_the_statement(name, H):
    d, fwd = _operands(name, H), _reference(name, H)[1]
    B, N, M, _ = d["dims"]
    O = 2 * H
    ysel, part = _poison(B * M, O), _poison(d["grid"], 2 * O)
    ksel = torch.full((B * M, O), 0xEE, dtype=U8, device=_dev())
    _call("apn_sa_wide_fwd_main", *d["dims"], O, *_geometry(d), d["w2img"].data_ptr(), d["pack1"].data_ptr(),
          d["sgn2"].data_ptr(), ysel.data_ptr(), ksel.data_ptr(), part.data_ptr())
    _exact_rows(part, fwd["stats2"], "fwd_main statistics")
    assert torch.equal(ysel.double(), fwd["ysel"])                 # (a NaN left in place equals nothing)
    assert torch.equal(ksel, fwd["ksel"])                          # (0xEE is no slot)


def _bwd_main(d, H, with_evec, r_part):
    B, N, M, _ = d["dims"]
    O = 2 * H
    out = dict(GU=_poison(B * M * 32, H), HA=_poison(B * M, H), HB=_poison(B * M, H), part=_poison(d["grid"], 2 * H))
    _call("apn_sa_wide_bwd_main", *d["dims"], O, *_geometry(d), d["zimg"].data_ptr(), d["pack1"].data_ptr(),
          d["evec"].data_ptr() if with_evec else None, d["goa"].data_ptr(), d["ksel"].data_ptr(), out["GU"].data_ptr(),
          out["HA"].data_ptr(), out["HB"].data_ptr(), out["part"].data_ptr(), None if r_part is None else r_part.data_ptr())
    return out


@pytest.mark.parametrize("with_evec", [True, False], ids=["evec", "noevec"])
@pytest.mark.parametrize("name,H", C.PAIRS)
def test_bwd_main_rows_sums_and_fused_products_equal_the_statement(name, H, with_evec):
    d = _operands(name, H)
    ref = _reference(name, H)[2 if with_evec else 3]
    O, RW = 2 * H, 3 * H * H + H
    r_part = _poison(d["grid"], RW) if H == 32 else None
    out = _bwd_main(d, H, with_evec, r_part)
    GU = out["GU"]
    assert torch.equal(GU[ref["rows"]], ref["GU"])                 # every row with a multiplicity
    untouched = torch.ones(GU.shape[0], dtype=torch.bool, device=GU.device)
    untouched[ref["rows"]] = False                                 # padding rows, and every row at or beyond 32 nt
    assert int(untouched.sum()) == GU.shape[0] - ref["rows"].numel() and bool(torch.isnan(GU[untouched]).all())
    assert torch.equal(out["HA"].double(), ref["HA"]) and torch.equal(out["HB"].double(), ref["HB"])
    _exact_rows(out["part"], ref["T"], "{T1, T2}")
    if H == 32:
        _exact_rows(r_part, ref["R"], "{R_S ; Gram ; suma} of the backward pass")


def _splits(name, H):
    c = C.CASES[name]
    return sorted({1, 3, _lib().apn_sa_wide_wgrad_splits(c["B"], c["M"], H)})


@pytest.mark.parametrize("name,H", [p for p in C.PAIRS if p[1] >= 64])
def test_wgrad_products_equal_the_statement_at_every_split(name, H):
    d, ref = _operands(name, H), _reference(name, H)[2]
    O, RW = 2 * H, 3 * H * H + H
    assert not _lib().apn_sa_wide_wgrad_fused(H) and _lib().apn_sa_wide_wgrad_fused(32)
    for splits in _splits(name, H):
        r_part = _poison(splits, RW)
        _call("apn_sa_wide_wgrad", *d["dims"], O, *_geometry(d), d["pack1"].data_ptr(), d["goa"].data_ptr(),
              d["ksel"].data_ptr(), splits, r_part.data_ptr())
        _exact_rows(r_part, ref["R"], "{R_S ; Gram ; suma} at %d splits" % splits)


# ---- argument checks --------------------------------------------------------------------------------------------------------

def test_bad_arguments_return_einval_and_launch_nothing():
    """A width outside {32, 64, 128, 256}, c_out != 2 c_mid, a null required pointer, H = 32 without r_part: APN_EINVAL from
    each entry, and not one byte of any output changes (every pointer that IS given is a real buffer of the H = 32 case)."""
    lib, d = _lib(), _operands("one", 32)
    B, N, M, H = d["dims"]
    O, RW = 2 * H, 3 * H * H + H
    st = torch.cuda.current_stream().cuda_stream
    outs = dict(part1=_poison(d["grid"], 2 * H), ysel=_poison(B * M, O), part2=_poison(d["grid"], 2 * O),
                GU=_poison(B * M * 32, H), HA=_poison(B * M, H), HB=_poison(B * M, H), partT=_poison(d["grid"], 2 * H),
                r_part=_poison(d["grid"], RW), ksel_out=torch.full((B * M, O), 0xEE, dtype=U8, device=_dev()))
    p = {k: v.data_ptr() for k, v in {**d, **outs}.items() if torch.is_tensor(v)}
    geo = ("U", "V", "idx", "tmap")

    def stats1(c_mid=H, **ptr):
        a = {**p, **ptr}
        return lib.apn_sa_wide_stats1(B, N, M, c_mid, *[a[k] for k in geo], a["part1"], st)

    def fwd(c_mid=H, c_out=O, **ptr):
        a = {**p, **ptr}
        return lib.apn_sa_wide_fwd_main(B, N, M, c_mid, c_out, *[a[k] for k in geo], a["w2img"], a["pack1"], a["sgn2"],
                                        a["ysel"], a["ksel_out"], a["part2"], st)

    def bwd(c_mid=H, c_out=O, **ptr):
        a = {**p, **ptr}
        return lib.apn_sa_wide_bwd_main(B, N, M, c_mid, c_out, *[a[k] for k in geo], a["zimg"], a["pack1"], a["evec"],
                                        a["goa"], a["ksel"], a["GU"], a["HA"], a["HB"], a["partT"], a["r_part"], st)

    def wgrad(c_mid=H, c_out=O, splits=1, **ptr):
        a = {**p, **ptr}
        return lib.apn_sa_wide_wgrad(B, N, M, c_mid, c_out, *[a[k] for k in geo], a["pack1"], a["goa"], a["ksel"], splits,
                                     a["r_part"], st)

    required = {stats1: geo + ("part1",),
                fwd: geo + ("w2img", "pack1", "sgn2", "ysel", "ksel_out", "part2"),
                bwd: geo + ("zimg", "pack1", "goa", "ksel", "GU", "HA", "HB", "partT", "r_part"),     # (r_part: at H = 32)
                wgrad: geo + ("pack1", "goa", "ksel", "r_part")}
    for entry, names in required.items():
        for bad in (0, -32, 16, 48, 96, 512):
            assert (entry(c_mid=bad) if entry is stats1 else entry(c_mid=bad, c_out=2 * bad)) == EINVAL, (entry.__name__, bad)
        if entry is not stats1:
            for c_mid, c_out in ((32, 32), (32, 128), (64, 64), (128, 64), (256, 256)):
                assert entry(c_mid=c_mid, c_out=c_out) == EINVAL, (entry.__name__, c_mid, c_out)
        for name in names:
            assert entry(**{name: None}) == EINVAL, (entry.__name__, name)
    assert wgrad(splits=0) == EINVAL and wgrad(splits=-1) == EINVAL
    torch.cuda.synchronize()
    for k, v in outs.items():
        assert bool((v == 0xEE).all() if v.dtype == U8 else torch.isnan(v).all()), k


# ---- the float case ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H", C.WIDTHS)
def test_float_case_stays_within_the_derived_bars(H):
    """The shape and indices of `mixed`, N(0,1) operands U, V, scale1, shift1, W2 (float32 values, so the float64 statement
    starts from the kernel's own inputs), against the float64 statement.  The bar of one element y2[p,c] = sum_k a1[p,k]
    w2[c,k], derived:

      a1      the kernel forms y1 = fl(u - v), pre1 = fl(fma(y1, scale1, shift1)), a1 = max(pre1, 0): one float32 rounding
              each (unit roundoff 2^-24), the first carried through the product: |da1| <= 2^-24 (|y1 scale1| + |pre1|)
              (relu moves a value no further than its argument moved);
      split   a float32 x becomes hi + lo, hi = bf16(x), lo = bf16(x - hi): |x - hi| <= 2^-8 |x| (half an ulp of 8
              significant bits), and what is left after lo is half an ulp of lo, <= 2^-17 |x|.  The bf16x3 product keeps
              hi hi + hi lo + lo hi, every one exact before it is added: it is x w less each operand's residual times
              the other operand, 2 * 2^-17 |x| |w|, and less the dropped lo lo, <= 2^-8 2^-8 |x| |w|: together
              (2^-17 + 2^-17 + 2^-16) |x| |w| = 2^-15 |a1| |w2| per product;
      sum     3 H / 16 accumulator updates of 16 products each: at most H roundings of 2^-24 on partial sums no larger
              than sum_k |a1| |w2|  (first order; the lo terms are 2^-8 of it)
          =>  bar[p,c] = (2^-15 + H 2^-24) sum_k |a1| |w2| + sum_k |da1| |w2|.

    ysel: the extreme over a query's positions moves no further than its most-moved candidate, so the bar of ysel[q,c] is
    the largest bar among the 32 positions -- compared on the entries the float64 statement DECIDES (the winner's gap to
    the best position gathering another point exceeds twice that bar; rows gathering the same point hold the same bits),
    where ksel must then be the statement's too.  The entries left out are at most 1 % (a condition; the seed is chosen on
    the CPU, tests/test_sa_wide_cases_cpu.py).  sum y2 per channel: the positions' bars added up, plus the float32 sum
    itself -- the product with the multiplicity, 15 additions in the lane, the lane halves, one update per tile the wave
    takes, two folds of the four waves: (20 + tiles per wave) 2^-24 sum |y2| -- the partial rows are added in float64."""
    inp = C.float_inputs(H, C.FLOAT_SEED)
    d = _on_device(inp)
    B, N, M, _ = d["dims"]
    O, dev = 2 * H, _dev()
    nt = C.layout("mixed")["tm"]["nt"]
    per_wave = -(-nt // (4 * d["grid"]))
    y2bar, statbar = C.float_bars(inp, dev, per_wave)
    ysel64, ksel64, bar, sure = C.float_pool(inp, dev, y2bar)
    left_out = 1.0 - sure.double().mean().item()
    ysel, part = _poison(B * M, O), _poison(d["grid"], 2 * O)
    ksel = torch.full((B * M, O), 0xEE, dtype=U8, device=dev)
    _call("apn_sa_wide_fwd_main", *d["dims"], O, *_geometry(d), d["w2img"].data_ptr(), d["pack1"].data_ptr(),
          d["sgn2"].data_ptr(), ysel.data_ptr(), ksel.data_ptr(), part.data_ptr())
    assert bool(torch.isfinite(part).all()) and bool(torch.isfinite(ysel).all())
    err = (ysel.double() - ysel64).abs()
    stat_err = (part.double().sum(0)[:O] - C.forward(inp, dev)["stats2"][:O]).abs()
    print("float case H = %d: pool %.3f (all entries %.3f), stat %.3f of the bar; left out %.4f"
          % (H, (err / bar)[sure].max(), (err / bar).max(), (stat_err / statbar).max(), left_out))
    assert left_out <= 0.01
    assert bool((err[sure] <= bar[sure]).all()) and torch.equal(ksel[sure], ksel64[sure])
    assert bool((err <= bar).all())            # (the extreme of moved candidates: no gap needed for the VALUE)
    assert bool((stat_err <= statbar).all())
