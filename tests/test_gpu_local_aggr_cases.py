"""The kernels of csrc/local_aggr.hip through their raw entries -- apn_la_pool_fwd, apn_la_stats_fold, apn_la_pool_bwd --
behind the index stage the device builds itself (apn_sa_wide_tilemap + apn_sa_wide_csr), on the problems of
tests/local_aggr_cases.py against its reference (tests/test_local_aggr_cases_cpu.py checks both on the CPU).

Four kinds of check:
  exact       integer / dyadic inputs on which every float32 step of both kernels is exact: the index the device built
              must EQUAL the host statement (decoded through plist / rowinfo / tq0: per point the rows (query, slot,
              multiplicity) that gather it, ascending; geo = {occ, SP}), and every output of the chain pool_fwd ->
              stats_fold -> pool_bwd -- the backward reading the forward's own sel and ysum and the device-built index --
              must EQUAL the reference: ext, sel, ysum, part row by row, sums, dU, dT, dp.  No tolerance.  At every
              width, every way the loop over a folded row's c rows ends, rows the fold predicate must keep whole, ties
              between different neighbours, waves that span clouds, reverse lists of chosen lengths, every gamma form,
              row pitch of wp, mode and dp form;
  float       Gaussian inputs: ext, sel, ysum, the eval-mode dU and dT equal a float32 restatement bit for bit; the rest
              stays within element-wise bars derived from the arithmetic (local_aggr_cases.float_bars);
  containment every input lies in a NaN-filled parent (the pad columns of wp are NaN as well), every output in a
              sentinel-filled one (every raw call in this file): no sentinel outside changes, none inside is left
              (sel byte by byte, part double by double; the tile map's blob and plist have unused tails), no NaN comes out;
  invariants  results that must agree bit for bit: two runs, a cloud alone, the row pitch of wp, dp given or NULL, a row
              folded against the same neighbourhood through all 32 slots, power-of-two scaling of gsel, D and E.

Indices outside the cloud reach apn_la_pool_fwd ALONE (test_forward_clamps_...): the index stage stores the raw idx and
adds it to the cloud's first point unclamped, so no such index is handed to the tile map, the csr entry or
apn_la_pool_bwd.  la_pool_fwd_kernel reads idx only at gq * 32 + (lane & 31) with gq < nq, brings the value into
[0, n - 1] with two comparisons that hold for every int32 (INT32_MIN < 0, INT32_MAX >= n) before anything else, and adds
it to the cloud's first point (gq / n) * n <= nq - n: the address lies in [0, B N).

The measured worst ratios to the bars, the file's wall time and the mutation check stand below the imports; test_zz
prints the ratios for a whole-file run.
"""
import numpy as np
import pytest
import torch

import local_aggr_cases as C
from test_gpu_edge_conv_cases import _Outputs, _in, _in_int

pytestmark = pytest.mark.gpu

# Measured on an MI355X (whole-file run), worst |kernel - float64| / bar over the twelve float cases:
#   ext    0.632 (H512-B5N13-mixed-r2.0)    part2  0.166 (H128-B5N13-mixed-r2.0)    geo      0.188 (H512-B2N65-ball-r0.25)
#   dU     0.098 (H256-B2N65-ball-r0.3)     dT     0.575 (H256-B3N77-whole-r0.5)    dp       0.053 (H64-B2N65-ball-r0.3)
#   part1, fold  0.000 (exact in float64)                                           dp_eval  0.074 (H64-B2N65-ball-r0.3)
# dU's bar counts one rounding per list entry on the whole sum of magnitudes, the sums of y^2 one per row: they are loose by
# construction; ext's and dT's are a handful of roundings at half an ulp each.  ext, sel, ysum and the eval-mode dU and dT
# matched the float32 restatement bit for bit in all twelve cases -- at r = 0.3 too: the device's float32 division is the
# correctly rounded one under this build's flags --, and all 76 exact cases matched the reference and the host statement of
# the index with no tolerance: neither csrc/local_aggr.hip nor the index stage needed a change.
# Wall time of this file on an MI355X: 4.6 s (98 tests; 5.8, 4.4 and 4.6 s in three runs; the slowest test 0.3 s: the first
# one, which loads the library).  The GPU suite without this file -- 1488 tests -- took 202 s in the same visit.
# Mutation check (each mutation of csrc/local_aggr.hip built into a scratch library, arithmetic only -- none changes an
# address, an index, a bound or a clamp; tests failing in this file, of 98 / in tests/test_gpu_invres.py, of 16; each file
# run once per library):
#   `t > best` -> `t >=`  (the LAST slot among equals)                        84 / 0
#   sg forced to 1  (the maximum under a negative gamma)                      51 / 2
#   mult0 forced to 1  (a folded row's slot 0 counted once)                   66 / 12
#   s2 accumulated from y instead of y * y                                    71 / 12
#   the forward's `if (k + g >= rows) break` removed                          48 / 12
#   the backward's `if (j + t >= chunk) break` removed                        89 / 13
#   dT: `(float)LA_K * E` -> `ge.x * E`                                       66 / 10
#   dU: `ge.x * E` -> `(float)LA_K * E`                                       66 / 11
#   rx: `ge.x * px - ge.y` -> `ge.y - ge.x * px`                              66 / 10
#   dp without `* inv_r`                                                      46 / 12
#   part: `red[2][col] + red[3][col]` -> `red[2][col]`                        64 / 12
#   `(int)sb == sj ? g : 0` -> `g`  (every row of a list takes the gradient)  84 / 13
# The module test sees eleven of the twelve (its inputs have no tie, so which of two equal neighbours wins is invisible to
# it); this file sees each in at least 46 tests, and names the output and the case.

F32, F64, I32, U8 = torch.float32, torch.float64, torch.int32, torch.uint8
WORST = {}                      # quantity -> [worst ratio to its bar, case]


def _call(*a):
    from adaptpoint_amd.fused import _call as call
    return call(*a)


# ---- the raw entries ----------------------------------------------------------------------------------------------------

def index_stage(dev, idx, p):
    """apn_sa_wide_tilemap (mode 1) + apn_sa_wide_csr on idx (B,N,32) around p itself -> tmap, pcnt_poff, plist, geo."""
    from adaptpoint_amd import _lib
    B, N, _ = idx.shape
    o = _Outputs(dev)
    tmap = o.new("tmap", (_lib.load().apn_sa_wide_tilemap_ints(B, N),), I32, inside=False)
    _call("apn_sa_wide_tilemap", dev, B, N, 1, idx.data_ptr(), tmap)
    args = [o.new("pcnt_poff", (2, B * N), I32), o.new("plist", (32 * B * N,), I32, inside=False), o.new("geo", (B, N, 4), F32)]
    _call("apn_sa_wide_csr", dev, B, N, N, idx.data_ptr(), p.data_ptr(), tmap, *args, None, None)
    return o.checked("index stage")


def la_pool_fwd(dev, U, p, wp, idx, gamma, r, train):
    B, N, H = U.shape
    o = _Outputs(dev)
    ext, sel = o.new("ext", (B, N, H), F32), o.new("sel", (B, N, H), U8)
    ysum = part = None
    if train:
        ysum, part = o.new("ysum", (B, N, H), F32), o.new("part", (C.part_rows(B, N), 2 * H), F64)
    _call("apn_la_pool_fwd", dev, B, N, H, C.K, float(r), U.data_ptr(), p.data_ptr(), wp.data_ptr(), wp.shape[1],
          idx.data_ptr(), None if gamma is None else gamma.data_ptr(), ext, sel, ysum, part)
    return o.checked("apn_la_pool_fwd")


def stats_fold(dev, part, count):
    rows, H = part.shape[0], part.shape[1] // 2
    o = _Outputs(dev)
    _call("apn_la_stats_fold", dev, part.data_ptr(), rows, H, float(count), o.new("sums", (2 * H + 2,), F64))
    return o.checked("apn_la_stats_fold")["sums"]


def la_pool_bwd(dev, gsel, sel, ix, U, p, ysum, de, wp, r, with_dp):
    B, N, H = U.shape
    o = _Outputs(dev)
    dU, dT = o.new("dU", (B, N, H), F32), o.new("dT", (B, N, H), F32)
    dp = o.new("dp", (B, N, 3), F32) if with_dp else None
    _call("apn_la_pool_bwd", dev, B, N, H, C.K, float(r), gsel.data_ptr(), sel.data_ptr(), ix["tmap"].data_ptr(),
          ix["pcnt_poff"].data_ptr(), ix["plist"].data_ptr(), ix["geo"].data_ptr(), U.data_ptr(), p.data_ptr(),
          None if ysum is None else ysum.data_ptr(), de.data_ptr(), wp.data_ptr(), wp.shape[1], dU, dT, dp)
    return o.checked("apn_la_pool_bwd")


def _chain(dev, inp, train, with_dp, idx=None, wp=None, gsel=None, de=None):
    """index stage -> pool_fwd (-> stats_fold) -> pool_bwd on the forward's own sel and ysum.  Eval mode: ysum = part = NULL
    and de = 0.  -> dict (the index under "ix")."""
    idx = inp["idx"] if idx is None else idx
    B, N, _ = idx.shape
    H = inp["U"].shape[2]
    d_idx, U, p = _in_int(dev, idx), _in(dev, inp["U"]), _in(dev, inp["p"])
    d_wp = _in(dev, inp["wp"] if wp is None else wp)
    gamma = None if inp["gamma"] is None else _in(dev, inp["gamma"])
    got = {"ix": index_stage(dev, d_idx, p)}
    got.update(la_pool_fwd(dev, U, p, d_wp, d_idx, gamma, inp["r"], train))
    if train:
        got["sums"] = stats_fold(dev, got["part"], B * N * C.K)
    de = (inp["de"] if de is None else de) if train else torch.zeros(2 * H)
    got.update(la_pool_bwd(dev, _in(dev, inp["gsel"] if gsel is None else gsel), got["sel"], got["ix"], U, p,
                           got["ysum"] if train else None, _in(dev, de), d_wp, inp["r"], with_dp))
    return got


CHAIN_OUTPUTS = ("ext", "sel", "ysum", "part", "sums", "dU", "dT", "dp")


def _same(a, b, names=CHAIN_OUTPUTS):
    return [n for n in names if n in a and n in b and not torch.equal(a[n], b[n])]


def check_index(ix, idx, p, rows, geo_exact=True):
    """What the device built against the host statement `rows` (local_aggr_cases.gather_rows) and the oracle's blob; geo to
    equality where its sums are exact (the float cases hold it to its bar)."""
    from oracle import oracle as O
    B, N, _ = idx.shape
    BN = B * N
    t = ix["tmap"].cpu()
    want = O.tile_map(idx.numpy())
    nt, off = int(t[0]), 4 + ((BN + 3) & ~3)
    assert nt == want["nt"]
    tq0, info = t[4:4 + nt].long(), t[off:off + 32 * nt].long() & 0xffffffff
    rownn = t[off + 32 * BN:off + 32 * BN + 32 * nt].long()
    assert np.array_equal(tq0.numpy(), want["tq0"]) and np.array_equal(info.numpy(), want["rowinfo"].reshape(-1))
    assert np.array_equal(rownn.numpy(), want["rownn"].reshape(-1))
    pcnt, poff = ix["pcnt_poff"].cpu().long()
    assert torch.equal(pcnt, rows["cnt"]), "rows per point"
    point = rows["point"]
    rank = torch.arange(len(point)) - (torch.cumsum(pcnt, 0) - pcnt)[point]
    e = ix["plist"].cpu().long()[poff[point] + rank]                           # the row ids, list by list
    assert bool((e >= 0).all()) and bool((e < 32 * nt).all())
    same = point[1:] == point[:-1]
    assert bool((e[1:][same] > e[:-1][same]).all()), "a list is not ascending"
    i = info[e]
    q = tq0[e >> 5] + (i & 0xff)
    assert torch.equal(q, rows["query"]) and torch.equal((i >> 8) & 0xff, rows["slot"]), "the (query, slot) of a list"
    assert torch.equal((i >> 16) & 0xff, rows["mult"]), "multiplicities"
    assert torch.equal(rownn[e] + (q // N) * N, point), "a row's neighbour is not the list's point"
    geo = ix["geo"].cpu().double().reshape(BN, 4)
    assert not geo_exact or torch.equal(geo, torch.cat([rows["occ"].view(BN, 1), rows["sp"]], 1)), "geo = {occ, SP}"


# ---- exact --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", C.CASES, ids=C.CASE_IDS)
def test_exact_cases_through_the_chain(dev, case):
    """The device-built index EQUALS the host statement and every output of the chain EQUALS the reference."""
    B, N, H = case.B, case.N, case.H
    inp = C.exact_inputs(case)
    want = C.expected(case, inp)
    got = _chain(dev, inp, case.train, case.dp)
    check_index(got["ix"], inp["idx"], inp["p"], want["rows"])
    names = ["ext", "sel", "dU", "dT"] + (["ysum", "part", "sums"] if case.train else []) + (["dp"] if case.dp else [])
    for name in names:
        assert torch.equal(got[name].cpu().double(), want[name].double()), name
    assert case.dp or "dp" not in got
    if not case.train:
        assert "ysum" not in got and "part" not in got


@pytest.mark.parametrize("H", C.WIDTHS)
def test_a_folded_row_equals_the_same_neighbourhood_through_all_32_slots(dev, H):
    """Every query as a ball row (c hits, then copies of slot 0) and as a row with the same 32-slot multiset, slot 0 in
    place, the other slots permuted (kept whole): ext, ysum and part agree, sel points at the same neighbour wherever one
    neighbour alone attains the extremum -- and both equal the reference."""
    case = C.Case(f"fold-H{H}", 400 + H, 3, 77, H, "ball", 0, 4, "mixed", True, True, 0.5)
    inp = C.exact_inputs(case)
    gen = torch.Generator().manual_seed(H)
    idx = torch.stack([C.ball_row(77, int(torch.randint(2, 32, (1,), generator=gen)), gen) for _ in range(3 * 77)]).view(3, 77, C.K).int()
    perm = torch.cat([torch.zeros(3, 77, 1, dtype=torch.long), 1 + torch.rand(3, 77, C.K - 1, generator=gen).argsort(-1)], -1)
    whole = torch.gather(idx, 2, perm)
    assert bool(C.ball_structure(idx)[0].all()) and float(C.ball_structure(whole)[0].double().mean()) < 0.2
    a, b = (_chain(dev, inp, True, True, idx=g) for g in (idx, whole))
    assert not _same(a, b, ("ext", "ysum", "part", "sums"))
    ref = C.pool_fwd(inp["U"], inp["p"], inp["W"][:, :3], idx, inp["gamma"], inp["r"])
    C.exact_range(case, dict(inp, idx=idx), dict(ref, **dict(zip(("dU", "dT", "dp"), C.pool_bwd(
        ref["y"], inp["gsel"], ref["sel"], ref["ysum"], idx, inp["de"], inp["W"][:, :3], inp["r"]))), rows=C.gather_rows(idx, inp["p"])))
    for name in ("ext", "sel", "ysum", "part"):
        assert torch.equal(a[name].cpu().double(), ref[name].double()), name
    t = ref["y"] * C.sign_of(inp["gamma"], H)
    at = t == t.max(2, keepdim=True)[0]
    who = idx.long().unsqueeze(-1).expand(-1, -1, -1, H)
    alone = torch.where(at, who, 77).min(2)[0] == torch.where(at, who, -1).max(2)[0]
    na = torch.gather(idx.long(), 2, a["sel"].cpu().long())                  # (B,N,H): the neighbour sel points at
    nb = torch.gather(whole.long(), 2, b["sel"].cpu().long())
    assert torch.equal(na[alone], nb[alone]) and float(alone.double().mean()) > 0.3


def test_forward_clamps_indices_outside_the_cloud(dev):
    """apn_la_pool_fwd alone (see the head of this file for the address argument): -1, N, N + 5, INT32_MIN and INT32_MAX in
    an eighth of the positions give the bits of the host-clamped graph."""
    for H, (B, N) in ((64, (3, 7)), (512, (2, 65))):
        inp = C.exact_inputs(C.Case("outside", 77 + H, B, N, H, "mixed", 0, 4, "mixed", True, True, 1.0))
        idx = C.outside_graph(B, N, torch.Generator().manual_seed(H))
        assert not bool(((idx >= 0) & (idx < N)).all())
        U, p, wp, gamma = (_in(dev, inp[k]) for k in ("U", "p", "wp", "gamma"))
        for train in (True, False):
            a = la_pool_fwd(dev, U, p, wp, _in_int(dev, idx), gamma, 1.0, train)
            b = la_pool_fwd(dev, U, p, wp, _in_int(dev, C.clamped(idx)), gamma, 1.0, train)
            assert not _same(a, b) and ("ysum" in a) == train
        ref = C.pool_fwd(inp["U"], inp["p"], inp["W"][:, :3], C.clamped(idx), inp["gamma"], 1.0)
        assert torch.equal(b["ext"].cpu().double(), ref["ext"]) and torch.equal(b["sel"].cpu(), ref["sel"])


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
    """Bit for bit against the float32 restatement: ext, sel, ysum, the eval-mode dU (list order) and dT.  Element-wise
    against float64 within the derived bars: ext and (where the float64 margin is positive) sel, part, sums, geo, the
    training-mode dU and dT, dp.  The backward's reference takes the forward kernel's own sel and ysum."""
    B, N, H = case.B, case.N, case.H
    inp = C.float_inputs(case)
    Wp, idx, r = inp["W"], inp["idx"], inp["r"]
    got = _chain(dev, inp, True, True)
    cpu = {n: t.cpu() for n, t in got.items() if torch.is_tensor(t)}
    rows = C.gather_rows(idx, inp["p"])
    check_index(got["ix"], idx, inp["p"], rows, geo_exact=False)
    ext, sel, ysum = C.pool_fwd_f32(inp["U"], inp["p"], Wp, idx, inp["gamma"], r)
    for name, t in (("ext", ext), ("sel", sel), ("ysum", ysum)):
        differ = int((cpu[name] != t).sum())
        print(f"{case.name} {name}: {differ} of {t.numel()} elements differ from the float32 restatement")
        assert differ == 0, name
    ref = C.pool_fwd(inp["U"], inp["p"], Wp, idx, inp["gamma"], r)
    bars = C.float_bars(inp, rows, cpu["ysum"], cpu["sel"])
    margin = C.sel_margin(ref["y"], bars["ybar"], idx, C.sign_of(inp["gamma"], H))
    assert float((margin <= 0).double().mean()) <= C.SEL_DROP_CAP
    assert torch.equal(cpu["sel"][margin > 0], ref["sel"][margin > 0]), "sel against float64"
    dU, dT, dp = C.pool_bwd(ref["y"], inp["gsel"], cpu["sel"], cpu["ysum"], idx, inp["de"], Wp, r)
    part1 = C._by_workgroup(cpu["ysum"].double())
    geo = torch.cat([rows["occ"].view(-1, 1), rows["sp"]], 1)
    checks = [("ext", cpu["ext"], ref["ext"], bars["ybar"].max(2)[0]),
              ("part1", cpu["part"][:, :H], part1, bars["part1"]), ("part2", cpu["part"][:, H:], ref["part"][:, H:], bars["part2"]),
              ("fold", cpu["sums"][:2 * H], cpu["part"].sum(0), cpu["part"].abs().sum(0) * 2.0 ** -40),
              ("geo", got["ix"]["geo"].reshape(B * N, 4), geo, bars["geo"]),
              ("dU", cpu["dU"], dU, bars["dU"]), ("dT", cpu["dT"], dT, bars["dT"]), ("dp", cpu["dp"], dp, bars["dp"])]
    bad = [(name, x) for name, x in ((name, _ratio(case, name, a, b, bar)) for name, a, b, bar in checks) if not x <= 1.0]
    assert not bad, (case.name, bad)
    assert cpu["sums"][2 * H:].tolist() == [float(B * N * C.K), 1.0]
    assert torch.equal(got["ix"]["geo"].cpu()[..., 0].double().reshape(-1), rows["occ"]), "occ is exact"
    ev = _chain(dev, inp, False, True)
    assert not _same(got, ev, ("ext", "sel")) and not _same(got["ix"], ev["ix"], ("pcnt_poff", "geo"))
    want = C.du_eval_f32(inp["gsel"], cpu["sel"], rows)
    assert torch.equal(ev["dU"].cpu(), want), "eval-mode dU: every list in ascending row id"
    assert torch.equal(ev["dT"].cpu(), want - inp["gsel"]), "eval-mode dT = dU - gsel"
    zero = torch.zeros(2 * H)
    e64 = C.pool_bwd(ref["y"], inp["gsel"], cpu["sel"], cpu["ysum"], idx, None, Wp, r)[2]
    ebar = C.float_bars(dict(inp, de=zero), rows, cpu["ysum"] * 0, cpu["sel"])["dp"]
    assert _ratio(case, "dp_eval", ev["dp"], e64, ebar) <= 1.0


# ---- invariants ---------------------------------------------------------------------------------------------------------

INVARIANT = [C.Float("inv-H64", 51, 5, 13, 64, "mixed", 0.3), C.Float("inv-H128", 52, 2, 128, 128, "ball", 0.5),
             C.Float("inv-H256", 53, 3, 77, 256, "whole", 0.3), C.Float("inv-H512", 54, 2, 65, 512, "mixed", 2.0)]


@pytest.mark.parametrize("case", INVARIANT, ids=[c.name for c in INVARIANT])
def test_bit_level_invariants(dev, case):
    """Two runs; cloud b alone against cloud b inside the batch (forward and backward; part where the cloud boundary is a
    workgroup boundary); the row pitch of wp; dp given or NULL; gsel, D and E scaled by 2^+-6 scale dU, dT and dp -- all
    bit for bit."""
    B, N, H = case.B, case.N, case.H
    inp = C.float_inputs(case)
    full = _chain(dev, inp, True, True)
    assert not _same(full, _chain(dev, inp, True, True)), "two runs"
    assert not _same(full["ix"], _chain(dev, inp, True, True)["ix"], ("pcnt_poff", "geo")), "two runs of the index stage"
    for b in sorted({0, B - 1}):
        one = dict(inp, U=inp["U"][b:b + 1], p=inp["p"][b:b + 1], idx=inp["idx"][b:b + 1], gsel=inp["gsel"][b:b + 1])
        alone = _chain(dev, one, True, True)
        for name in ("ext", "sel", "ysum", "dU", "dT", "dp"):
            assert torch.equal(alone[name][0], full[name][b]), ("cloud", b, name)
        assert torch.equal(alone["ix"]["geo"][0], full["ix"]["geo"][b]), ("cloud", b, "geo")
        if N % 64 == 0:
            assert torch.equal(alone["part"], full["part"][b * N // 64:(b + 1) * N // 64]), ("cloud", b, "part")
    for ldw in (3, 67):
        wp = torch.full((H, ldw), float("nan"))
        wp[:, :3] = inp["W"]
        assert not _same(full, _chain(dev, inp, True, True, wp=wp)), ("ldw", ldw)
    nodp = _chain(dev, inp, True, False)
    assert "dp" not in nodp and not _same(full, nodp), "dp = NULL"
    for train in (True, False):
        base = full if train else _chain(dev, inp, False, True)
        for s in (-6, 6):
            scaled = _chain(dev, inp, train, True, gsel=inp["gsel"] * 2.0 ** s, de=inp["de"] * 2.0 ** s)
            for name in ("dU", "dT", "dp"):
                assert torch.equal(scaled[name], base[name] * 2.0 ** s), ("scaled", train, s, name)
            assert not _same(scaled, base, ("ext", "sel", "ysum", "part", "sums"))


def test_zz_worst_figures_of_this_run(dev):
    """A printing aid, after the pattern of tests/test_gpu_edge_conv_cases.py: the worst ratio to each bar over whatever
    float cases ran before it in this process (the table in the header comes from a whole-file run).  It asserts
    nothing new -- test_float_cases has asserted every ratio already -- and nothing at all when no float case ran."""
    for name, (ratio, at) in sorted(WORST.items()):
        print(f"MEASURED {name:>8}: worst |kernel - float64| / bar {ratio:.3f} ({at})")
        assert ratio <= 1.0, (name, at)
