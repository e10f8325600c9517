"""Exact cases for the per-position kernels of csrc/sa_wide.hip -- apn_sa_wide_stats1, apn_sa_wide_fwd_main,
apn_sa_wide_bwd_main, apn_sa_wide_wgrad -- and the plain statement of what each of them computes.

The inputs of a case (B, N, M, H, O = 2H) are small integers: idx (B,M,32), U (B,N,H), V (B,M,H), pack1 = {scale1, shift1,
mean1, invstd1}[H], W2 (O,H), sgn2 (O) = +-1, Qm (H,H), evec (H), goa (B,M,O), ksel (B,M,O).  Then every quantity of the
chain is an integer (a half-integer where invstd1 = 1/2): the split-bf16 operands hold such integers exactly (hi + lo: 16
significant bits), the one product the bf16x3 form drops (lo * lo) is zero as long as one operand of every product has at
most 8 significant bits, and a float32 accumulator holds exact integers in any summation order.  So every output of every
kernel is pinned BIT FOR BIT, and the pool meets ties at every turn -- which float inputs never produce.

The statement is written over the B * M * 32 POSITIONS of idx:

    y1[q,k] = U[idx[q,k]] - V[q]      a1 = relu(fma(y1, scale1, shift1))      y2 = a1 W2^T      yhat1 = (y1 - mean1) invstd1

A position belongs to a ROW of its query, named by the row's slot (`position_slots`: its own index k, except that the
trailing repeats of slot 0 in a ball-query row belong to slot 0); a row's multiplicity is the number of its positions.
Only where an output is indexed by a row of the tile map -- GU, and the mutations that speak of lane halves or padding --
does the statement read `oracle.tile_map`, the plain-Python definition of the map.

    stats1     per channel  sum y1, sum y1^2 over the positions
    fwd_main   per channel  sum y2, sum y2^2;  ysel[q,c] = the extreme of y2[q,:,c] (maximum where sgn2[c] = +1, minimum
               where -1);  ksel[q,c] = the LOWEST slot attaining it
    bwd_main   S = goa[q,c] on the row whose slot is ksel[q,c], 0 elsewhere; per row (multiplicity mult)
                   g = [fma(y1, scale1, shift1) > 0] (S W2 + mult (a1 Qm + evec))          (evec None: g = [..] S W2)
               GU[tile * 32 + row] = g,  T1 = sum_rows g,  T2 = sum_rows g yhat1,  HA[q] = sum_{rows of q} g,
               HB[q] = sum_{rows of q} mult yhat1
    wgrad      R_S[c,:] = sum_q goa[q,c] a1[row (q, ksel[q,c]), :],  Gram = sum_rows mult a1^T a1,  suma = sum_rows mult a1

`inputs(name, H)` draws a case and RAISES unless it is exact (`check_exact`) and tells kernels apart (`check_telling`);
`MUTATIONS` are wrong statements that tests/test_sa_wide_cases_cpu.py proves the table distinguishes from the true one.
Nothing here needs a GPU; the tensors live wherever `dev` says (the GPU suite evaluates the statement in float64 there).
"""
import functools
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.oracle import tile_map  # noqa: E402

K = 32
WIDTHS = (32, 64, 128, 256)
F64 = torch.float64
LIMIT = float(2 ** 24)

# name -> shape, the widths it runs at, whether the map folds ball-query rows, the value ranges (chosen per case so that
# `check_exact` holds: U, V in [-u, u], shift1 / mean1 in [-sh, sh], W2 with `w2n` entries per row in [-w2, w2] \ {0}, Qm
# with `qmn` per row in [-qm, qm] \ {0}, evec in [-ev, ev], goa in [-goa, goa]) and whether a pool can tie at all.
CASES = {
    # a single query whose 32 slots are one point: one row of multiplicity 32, 31 padding rows, three idle waves
    "one": dict(B=1, N=1, M=1, widths=WIDTHS, fold=True, ties=False,
                rng=dict(u=8, scales=(1, -1, 2, -2), sh=4, w2=4, w2n=3, qm=2, qmn=2, ev=2, goa=64)),
    # queries cycle through: 32 distinct hits; 1, 2, 7, 31 hits then the fill; a row with repeats that is no ball-query row
    # (kept whole): tiles of one and of several queries, padding rows, far fewer tiles than queries, idle workgroups
    "mixed": dict(B=3, N=40, M=37, widths=WIDTHS, fold=True, ties=True,
                  rng=dict(u=5, scales=(1, -1, 2, -2), sh=3, w2=4, w2n=2, qm=2, qmn=2, ev=2, goa=64)),
    # one tile per query, a tile count that is no multiple of the four waves
    "whole": dict(B=2, N=40, M=33, widths=(32, 128), fold=False, ties=True,
                  rng=dict(u=5, scales=(1, -1, 2, -2), sh=3, w2=4, w2n=2, qm=2, qmn=2, ev=2, goa=64)),
    # B M = 2200 > 2048 tiles: 152 waves take a second tile -- the cyclic chunk sequence and the one-step-ahead prefetches
    # across a tile boundary, resident and streaming
    "rounds": dict(B=2, N=64, M=1100, widths=(32, 128, 256), fold=False, ties=True,
                   rng=dict(u=2, scales=(1, -1), sh=1, w2=2, w2n=2, qm=1, qmn=2, ev=1, goa=8)),
    # the same queries with 8 hits each: about a quarter as many tiles as queries, so most workgroups are idle and must
    # still write zero partial rows
    "rounds_folded": dict(B=2, N=64, M=1100, widths=(64,), fold=True, ties=True,
                          rng=dict(u=2, scales=(1, -1), sh=1, w2=2, w2n=2, qm=1, qmn=2, ev=1, goa=8)),
}
PAIRS = [(name, H) for name, c in CASES.items() for H in c["widths"]]
MIXED_KINDS = (32, 1, 2, 7, 31, 0)          # hits of a query of "mixed", by q % 6 (0: the row with repeats)

FLOAT_SEED = 5          # of the float case (tests/test_sa_wide_cases_cpu.py: its gap rule leaves out at most 1 % at every width)

MUTATIONS = ("tie_highest", "tie_lower_half", "stats_no_mult", "padding_counted", "cloud0", "ksel_row_in_tile",
             "evec_no_mult", "gram_no_mult")


def _seed(name, H):
    return 1000 * (list(CASES).index(name) + 1) + H


# ---- indices and the rows of a query ------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def make_idx(name):
    """The crafted neighbour indices of a case, (B,M,32) int32 (the same at every width)."""
    c = CASES[name]
    B, N, M = c["B"], c["N"], c["M"]
    rng = np.random.default_rng(7 + list(CASES).index(name))
    if name == "one":
        idx = np.zeros((B, M, K), np.int64)
    elif name == "mixed":
        idx = np.zeros((B, M, K), np.int64)
        for b in range(B):
            for q in range(M):
                hits = MIXED_KINDS[q % len(MIXED_KINDS)]
                perm = rng.permutation(N)
                if hits:
                    idx[b, q] = perm[0]
                    idx[b, q, :hits] = perm[:hits]
                else:                                   # 16 points twice, slot 0 again at slot 16: no ball-query row
                    idx[b, q] = np.concatenate([perm[:16], perm[:16]])
    elif name in ("whole", "rounds"):
        idx = rng.integers(0, N, size=(B, M, K))
    else:                                               # rounds_folded: 8 distinct hits, then the fill
        hits = rng.random((B, M, N)).argsort(-1)[..., :8]
        idx = np.repeat(hits[..., :1], K, axis=-1)
        idx[..., :8] = hits
    idx = np.ascontiguousarray(idx.astype(np.int32))
    idx.setflags(write=False)
    return idx


def position_slots(idx, fold):
    """idx (B,M,32) -> slot (B,M,32): the slot of the row every position belongs to.  With `fold`, a ball-query row -- its
    c leading slots differ from slot 0, every later one repeats it -- has the rows 0..c-1 and its trailing positions belong
    to row 0; any other row of idx, and every row without `fold`, has one row per position."""
    idx = np.asarray(idx)
    k = np.arange(K)
    slot = np.broadcast_to(k, idx.shape).copy()
    if fold:
        differ = idx != idx[..., :1]
        c0 = differ.sum(-1, keepdims=True) + 1
        ball = (differ == ((k >= 1) & (k < c0)))[..., 1:].all(-1, keepdims=True)
        slot[np.broadcast_to(ball & (k >= c0), idx.shape)] = 0
    return slot


def blob(tm, B, M):
    """The int32 blob the kernels read, from `oracle.tile_map`'s dict: [nt, 0, 0, 0], tq0 at int 4, rowinfo at
    4 + ((B M + 3) & ~3), rownn 32 B M ints behind it (room for B M tiles each; the tiles beyond nt stay 0)."""
    bm, nt = B * M, tm["nt"]
    rows_off = 4 + ((bm + 3) & ~3)
    out = np.zeros(rows_off + 64 * bm, np.int32)
    out[0] = nt
    out[4:4 + nt] = tm["tq0"]
    out[rows_off:rows_off + 32 * nt] = tm["rowinfo"].astype(np.uint32).view(np.int32).reshape(-1)
    out[rows_off + 32 * bm:rows_off + 32 * bm + 32 * nt] = tm["rownn"].reshape(-1)
    return out


@functools.lru_cache(maxsize=None)
def layout(name):
    """What the statement needs of a case's rows: slot (B M,32) of every position, rep (B M,32): the position is its row's
    first, mult (B M,32): the row's multiplicity at its first position (0 elsewhere), nslots (B M), and from the tile map
    tm: tile (B M) and row0 (B M), the tile of a query and its first row there, pad = (tile, row, query, neighbour) of
    every padding row as the kernels address them (query 0 of the tile)."""
    c = CASES[name]
    B, M = c["B"], c["M"]
    idx = make_idx(name)
    slot = position_slots(idx, c["fold"]).reshape(B * M, K)
    rep = slot == np.arange(K)
    mult = np.zeros_like(slot)
    for s in range(K):
        mult[:, s] = (slot == s).sum(1)
    mult = mult * rep
    tm = tile_map(idx, c["fold"])
    tile = np.full(B * M, -1, np.int64)
    row0 = np.full(B * M, -1, np.int64)
    pad = []
    for t in range(tm["nt"]):
        for r in range(32):
            info = int(tm["rowinfo"][t, r])
            if (info >> 16) & 0xff:
                q = int(tm["tq0"][t]) + (info & 0xff)
                if ((info >> 8) & 0xff) == 0:
                    tile[q], row0[q] = t, r
            else:
                pad.append((t, r, int(tm["tq0"][t]), int(tm["rownn"][t, r])))
    return dict(idx=idx, slot=slot, rep=rep, mult=mult, nslots=rep.sum(1), tm=tm, tile=tile, row0=row0,
                pad=np.array(pad, np.int64).reshape(-1, 4), blob=blob(tm, B, M))


# ---- inputs -------------------------------------------------------------------------------------------------------------

def _sparse(rng, rows, cols, per_row, bound):
    out = np.zeros((rows, cols))
    for r in range(rows):
        at = rng.choice(cols, size=min(per_row, cols), replace=False)
        out[r, at] = rng.integers(1, bound + 1, size=at.size) * rng.choice([-1, 1], size=at.size)
    return out


def draw(name, H):
    """The integer inputs of (case, width) as float64 / integer numpy arrays (not yet checked: `inputs`)."""
    c, r = CASES[name], CASES[name]["rng"]
    B, N, M, O = c["B"], c["N"], c["M"], 2 * H
    rng = np.random.default_rng(_seed(name, H))
    lay = layout(name)
    sgn2 = rng.choice([-1.0, 1.0], size=O)
    sgn2[:2] = (1.0, -1.0)
    scale1 = rng.choice(np.array(r["scales"], np.float64), size=H)
    scale1[:len(r["scales"])] = r["scales"]
    return dict(
        name=name, H=H, O=O, B=B, N=N, M=M, fold=c["fold"], idx=lay["idx"],
        U=rng.integers(-r["u"], r["u"] + 1, size=(B, N, H)).astype(np.float64),
        V=rng.integers(-r["u"], r["u"] + 1, size=(B, M, H)).astype(np.float64),
        pack1=np.concatenate([scale1, rng.integers(-r["sh"], r["sh"] + 1, size=H).astype(np.float64),
                              rng.integers(-r["sh"], r["sh"] + 1, size=H).astype(np.float64),
                              rng.choice([0.5, 1.0, 2.0], size=H)]),
        W2=_sparse(rng, O, H, r["w2n"], r["w2"]), sgn2=sgn2, Qm=_sparse(rng, H, H, r["qmn"], r["qm"]),
        evec=rng.integers(-r["ev"], r["ev"] + 1, size=H).astype(np.float64),
        goa=rng.integers(-r["goa"], r["goa"] + 1, size=(B, M, O)).astype(np.float64),
        ksel=(rng.integers(0, 1 << 30, size=(B * M, O)) % lay["nslots"][:, None]).astype(np.uint8).reshape(B, M, O))


def float_inputs(H, seed):
    """The float case of a width: the shape and indices of "mixed", N(0,1) operands (goa, ksel, Qm, evec as in `draw`: the
    float case covers the forward only)."""
    inp = draw("mixed", H)
    rng = np.random.default_rng(seed)
    f32 = lambda a: a.astype(np.float32).astype(np.float64)          # (what the kernel is handed: float32 values)
    inp.update(U=f32(rng.standard_normal(inp["U"].shape)), V=f32(rng.standard_normal(inp["V"].shape)),
               W2=f32(rng.standard_normal(inp["W2"].shape)),
               pack1=f32(np.concatenate([rng.standard_normal(2 * H), np.zeros(H), np.ones(H)])))
    return inp


def _t(a, dev, dtype=F64):
    return torch.as_tensor(np.array(a), device=dev).to(dtype)


# ---- the statement --------------------------------------------------------------------------------------------------------

def positions(inp, dev, mutate=None):
    """y1, pre1 = fma(y1, scale1, shift1), a1, yhat1 at every position, (B M, 32, H) float64 on `dev`."""
    B, M, H = inp["B"], inp["M"], inp["H"]
    U, V, pack1 = _t(inp["U"], dev), _t(inp["V"], dev), _t(inp["pack1"], dev)
    idx = _t(inp["idx"], dev, torch.int64)
    cloud = torch.arange(B, device=dev).view(B, 1, 1)
    if mutate == "cloud0":
        cloud = torch.zeros_like(cloud)
    y1 = (U[cloud, idx] - V.unsqueeze(2)).reshape(B * M, K, H)
    pre1 = y1 * pack1[:H] + pack1[H:2 * H]
    return y1, pre1, torch.relu(pre1), (y1 - pack1[2 * H:3 * H]) * pack1[3 * H:]


def _padding(inp, lay, dev):
    """y1 and y2 of the tile map's padding rows as the kernels would address them (for the mutation that counts them)."""
    H = inp["H"]
    pad = lay["pad"]
    U, V, pack1 = _t(inp["U"], dev).reshape(-1, H), _t(inp["V"], dev).reshape(-1, H), _t(inp["pack1"], dev)
    q = torch.as_tensor(pad[:, 2], device=dev)
    y1 = U[(q // inp["M"]) * inp["N"] + torch.as_tensor(pad[:, 3], device=dev)] - V[q]
    return y1, torch.relu(y1 * pack1[:H] + pack1[H:2 * H]) @ _t(inp["W2"], dev).t()


def forward(inp, dev="cpu", mutate=None, telling=False):
    """stats1 (2H), stats2 (2O), ysel (B M,O) float64, ksel (B M,O) uint8.  With `telling` also what `check_telling` and
    `check_exact` ask about: gates, ties, the lane halves of tied rows, the sums of absolute terms."""
    lay = layout(inp["name"])
    y1, pre1, a1, _ = positions(inp, dev, mutate)
    W2, sgn2 = _t(inp["W2"], dev), _t(inp["sgn2"], dev)
    y2 = a1 @ W2.t()                                                       # (B M, 32, O)
    slot = _t(lay["slot"], dev, torch.int64)
    rep = _t(lay["rep"], dev, torch.bool)
    wpos = rep.to(F64).unsqueeze(2) if mutate == "stats_no_mult" else torch.ones(1, 1, 1, dtype=F64, device=dev)
    stats1 = torch.cat([(wpos * y1).sum((0, 1)), (wpos * y1 * y1).sum((0, 1))])
    stats2 = torch.cat([(wpos * y2).sum((0, 1)), (wpos * y2 * y2).sum((0, 1))])
    if mutate == "padding_counted" and len(lay["pad"]):
        p1, p2 = _padding(inp, lay, dev)
        stats1 = stats1 + torch.cat([p1.sum(0), (p1 * p1).sum(0)])
        stats2 = stats2 + torch.cat([p2.sum(0), (p2 * p2).sum(0)])
    v = y2 * sgn2
    best = v.max(1)[0]                                                     # (B M, O)
    attain = v == best.unsqueeze(1)                                        # (B M, 32, O)
    rowpos = _t(lay["row0"], dev, torch.int64).unsqueeze(1) + slot         # the position's row within its tile
    half = (rowpos >> 2) & 1                                               # acc row = (i&3) + 8(i>>2) + 4h: h = bit 2
    key = slot
    if mutate == "tie_highest":
        key = -slot
    elif mutate == "tie_lower_half":
        key = half * 256 + slot
    pick = torch.where(attain, key.unsqueeze(2), 1 << 20).min(1)[0]
    ksel = (-pick if mutate == "tie_highest" else pick) & 255
    if mutate == "ksel_row_in_tile":
        ksel = _t(lay["row0"], dev, torch.int64).unsqueeze(1) + ksel
    out = dict(stats1=stats1, stats2=stats2, ysel=best * sgn2, ksel=ksel.to(torch.uint8))
    if telling:
        assert mutate is None
        arow = attain & rep.unsqueeze(2)                                   # attaining ROWS
        tie = arow.sum(1) >= 2
        win_half = torch.gather(half, 1, ksel)           # (a row's first position is its slot: the winner's lane half)
        in0 = (arow & (half == 0).unsqueeze(2)).any(1)
        in1 = (arow & (half == 1).unsqueeze(2)).any(1)
        out.update(
            gate_open=(pre1 > 0).any(1).any(0), gate_closed=(pre1 <= 0).any(1).any(0), tie_per_channel=tie.sum(0),
            lower_in_upper=int((in0 & in1 & (win_half == 1)).sum()), lower_in_lower=int((in0 & in1 & (win_half == 0)).sum()),
            a1_max=float(a1.max()),
            sums=dict(stat1=float(torch.maximum(y1.abs().sum((0, 1)), (y1 * y1).sum((0, 1))).max()),
                      stat2=float(torch.maximum(y2.abs().sum((0, 1)), (y2 * y2).sum((0, 1))).max()),
                      mfma_fwd=float((a1 @ W2.abs().t()).max())))
    return out


def backward(inp, dev="cpu", with_evec=True, mutate=None, telling=False):
    """rows (R) = tile * 32 + row of every live row, GU (R,H) in that order, T (2H) = {T1, T2}, HA, HB (B M,H),
    R ((O+H) H + H) = {R_S ; Gram ; suma}, all float64.  ksel and goa are the case's own."""
    lay = layout(inp["name"])
    H, O, BM = inp["H"], inp["O"], inp["B"] * inp["M"]
    y1, pre1, a1, yhat = positions(inp, dev, mutate)
    W2, Qm, evec = _t(inp["W2"], dev), _t(inp["Qm"], dev), _t(inp["evec"], dev)
    goa, ksel = _t(inp["goa"], dev).reshape(BM, 1, O), _t(inp["ksel"], dev, torch.int64).reshape(BM, 1, O)
    slot = _t(lay["slot"], dev, torch.int64)
    rep = _t(lay["rep"], dev, torch.bool)
    mult = _t(lay["mult"], dev).unsqueeze(2)                               # (B M, 32, 1), 0 off a row's first position
    S = torch.where(rep.unsqueeze(2) & (slot.unsqueeze(2) == ksel), goa, torch.zeros((), dtype=F64, device=dev))
    dA = S @ W2
    if with_evec:
        dA = dA + mult * (a1 @ Qm) + (rep.to(F64).unsqueeze(2) if mutate == "evec_no_mult" else mult) * evec
    g = torch.where((pre1 > 0) & rep.unsqueeze(2), dA, torch.zeros((), dtype=F64, device=dev))
    rows = (_t(lay["tile"], dev, torch.int64) * 32 + _t(lay["row0"], dev, torch.int64)).unsqueeze(1) + slot
    gram_w = rep.to(F64).unsqueeze(2) if mutate == "gram_no_mult" else mult
    a1f = a1.reshape(-1, H)
    out = dict(rows=rows[rep], GU=g[rep], T=torch.cat([g.sum((0, 1)), (g * yhat).sum((0, 1))]), HA=g.sum(1),
               HB=(mult * yhat).sum(1),
               R=torch.cat([(S.reshape(-1, O).t() @ a1f).reshape(-1), ((gram_w * a1).reshape(-1, H).t() @ a1f).reshape(-1),
                            (mult * a1).sum((0, 1))]))
    if telling:
        gran = torch.clamp(_t(inp["pack1"], dev)[3 * H:], max=1.0)         # T2 and HB count in units of 1/2 where invstd1 = 1/2
        gabs = S.abs() @ W2.abs() + mult * (a1 @ Qm.abs() + evec.abs())       # the absolute terms of one element of g
        out["sums"] = dict(
            mfma_bwd=float((S.abs() @ W2.abs() + mult * (a1 @ Qm.abs())).max()), T1=float(gabs.sum((0, 1)).max()),
            T2=float(((gabs * yhat.abs()).sum((0, 1)) / gran).max()), HB=float(((mult * yhat.abs()).sum(1) / gran).max()),
            R_S=float((S.abs().reshape(-1, O).t() @ a1f).max()), gram_suma=float(out["R"][O * H:].max()),
            goa=float(goa.abs().max()), mult_a1=float((mult * a1).max()))
    return out


# ---- the conditions -------------------------------------------------------------------------------------------------------

def check_exact(inp, fwd, bwd):
    """Raise unless every float32 step of the kernels is exact on this case (see the header): fwd, bwd = `forward` and
    `backward` (with evec) evaluated with `telling`."""
    why = []
    if max(np.abs(inp["W2"]).max(), np.abs(inp["Qm"]).max()) >= 256:
        why.append("a weight has a lo part")
    if fwd["a1_max"] > 255:
        why.append("a1 has a lo part (it sits on both sides of the Gram product)")
    if bwd["sums"]["goa"] >= 2 ** 16 or bwd["sums"]["mult_a1"] >= 2 ** 16:
        why.append("goa or mult a1 needs more than hi + lo")
    for k, v in list(fwd["sums"].items()) + list(bwd["sums"].items()):
        if not v < LIMIT:
            why.append("the accumulator %s may pass 2^24: sum of absolute terms %.3g" % (k, v))
    lay = layout(inp["name"])
    if not (inp["ksel"].reshape(-1, inp["O"]) < lay["nslots"][:, None]).all():
        why.append("ksel names a slot its query does not have")
    if why:
        raise ValueError("%s at H = %d is not exact: %s" % (inp["name"], inp["H"], "; ".join(why)))


def check_telling(inp, fwd):
    """Raise unless the case can tell kernels apart: open and closed ReLU gates on every mid channel, a tie in every output
    channel's pool (where the case has more than one row), both signs of sgn2 and of scale1."""
    why = []
    several = CASES[inp["name"]]["ties"]           # (a case of ONE row: a channel's gate has one state, its pool one candidate)
    both = fwd["gate_open"].all() and fwd["gate_closed"].all() if several else fwd["gate_open"].any() and fwd["gate_closed"].any()
    if not bool(both):
        why.append("a mid channel's gate is always open or always closed")
    if several and not bool((fwd["tie_per_channel"] > 0).all()):
        why.append("an output channel's pool never ties")
    for what, v in (("sgn2", inp["sgn2"]), ("scale1", inp["pack1"][:inp["H"]])):
        if not ((v > 0).any() and (v < 0).any()):
            why.append("one sign of %s is missing" % what)
    if why:
        raise ValueError("%s at H = %d tells too little: %s" % (inp["name"], inp["H"], "; ".join(why)))


def inputs(name, H, dev="cpu"):
    """The checked inputs of (case, width) with their statement: (inp, fwd, bwd, bwd_noevec); raises if a condition fails."""
    inp = draw(name, H)
    fwd = forward(inp, dev, telling=True)
    bwd = backward(inp, dev, True, telling=True)
    check_exact(inp, fwd, bwd)
    check_telling(inp, fwd)
    return inp, fwd, bwd, backward(inp, dev, False)


# ---- the float case's bar -------------------------------------------------------------------------------------------------

def float_bars(inp, dev, rounds=1):
    """Element-wise bars of the float case (derivation: tests/test_gpu_sa_wide_cases.py::test_float_case...):
    y2 (B M,32,O): |kernel y2 - float64 y2| <= (2^-15 + H 2^-24) sum_k |a1| |w2| + sum_k da1 |w2|,
    da1 = 2^-24 (|y1 scale1| + |pre1|);  stat (O): the bar of sum y2 = sum over positions of y2's + (20 + rounds) 2^-24 sum |y2|."""
    H = inp["H"]
    y1, pre1, a1, _ = positions(inp, dev)
    W2a, pack1 = _t(inp["W2"], dev).abs().t(), _t(inp["pack1"], dev)
    da1 = 2.0 ** -24 * ((y1 * pack1[:H]).abs() + pre1.abs())
    y2bar = (2.0 ** -15 + H * 2.0 ** -24) * (a1 @ W2a) + da1 @ W2a
    y2 = a1 @ _t(inp["W2"], dev).t()
    return y2bar, y2bar.sum((0, 1)) + (20 + rounds) * 2.0 ** -24 * y2.abs().sum((0, 1)) * (1 + 2.0 ** -10)


def float_pool(inp, dev, y2bar):
    """The float64 pool of the float case and where it is decided: ysel, ksel (B M,O), bar (B M,O) = the largest bar among
    the query's positions, sure (B M,O): the winner's gap to the best position gathering ANOTHER point exceeds 2 bar (rows
    gathering the same point hold the same bits in the kernel too: between them the lowest slot wins on both sides)."""
    f = forward(inp, dev)
    _, _, a1, _ = positions(inp, dev)
    v = (a1 @ _t(inp["W2"], dev).t()) * _t(inp["sgn2"], dev)
    idx = _t(inp["idx"], dev, torch.int64).reshape(-1, K)
    first = f["ksel"].long()                             # (a row's first position is its slot: the winner's position)
    other = idx.unsqueeze(2) != torch.gather(idx, 1, first).unsqueeze(1)
    runner = torch.where(other, v, torch.full((), -float("inf"), dtype=F64, device=dev)).max(1)[0]
    bar = y2bar.max(1)[0]
    return f["ysel"], f["ksel"], bar, (v.max(1)[0] - runner) > 2 * bar
