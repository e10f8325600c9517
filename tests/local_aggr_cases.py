"""The problems tests/test_gpu_local_aggr_cases.py gives the raw entries of csrc/local_aggr.hip (apn_la_pool_fwd,
apn_la_stats_fold, apn_la_pool_bwd) behind the index stage (apn_sa_wide_tilemap, apn_sa_wide_csr), in plain torch (no
extension): the case table, the graph and input generators, a reference of every entry, the per-case range proofs and
the float bars.  tests/test_local_aggr_cases_cpu.py checks the table and the reference on the CPU.

REFERENCE -- written from the header comment of csrc/local_aggr.hip and the LocalAggregation block of
include/adaptpoint_amd.h as gathers over (b, q, k), all 32 slots of every query (`pool_fwd`, `pool_bwd`): nothing of
waves, channels per lane, rows in flight, folded rows or the tile map.

    y[q,k,c]     = U[idx[q,k],c] + Wp[c,:] . (p[idx[q,k]] - p[q]) / r
    ext[q,c]     = max_k y where gamma[c] >= 0 (-0.0 included) or gamma is None, min_k y elsewhere
    sel[q,c]     = the first of the 32 slots that attains it
    ysum[q,c]    = sum_k y;   part[w] = {sum y, sum y^2} over the positions of the flat queries [64 w, 64 w + 64)
    sums         = {column sums of part, count, 1}
    dL/dy[q,k,c] = gsel[q,c] [k == sel[q,c]] + D_c y[q,k,c] + E_c           (D = E = 0 in eval mode)
    dU[n,c]      = the sum of dL/dy over the positions with idx[q,k] == n
    dT[n]        = dU[n] - (gsel[n] + D ysum[n] + 32 E);   dp[n] = dT[n] Wp / r

It runs in float64.  Where the order of float32 operations is part of the contract there is a float32 form, used by the
float cases only (`pool_fwd_f32`: y as the header states it -- the relative position formed first and divided by r, the
three coordinate products chained by fma from the x column on, U added last --, ext, sel, and ysum as (33 - c) y0 then the
slots 1..c-1 for a row with the ball-query structure and in slot order for any other row; `du_eval_f32`: every reverse
list added in ascending row id).  An fma is formed in float64 and rounded once more: two float32 factors multiply
exactly there, and the second rounding differs from the fused one only on a 2^-29 tie of the float64 sum.

THE INDEX STAGE's statement (`gather_rows`): a query with the ball-query structure -- the slots that differ from slot 0
are exactly 1..c-1 -- has the rows (slot 0, multiplicity 33 - c), (slot 1, 1) .. (slot c-1, 1); any other query one row
of multiplicity 1 per slot.  A point's list holds the rows that gather it in ascending (query, slot);
geo = {sum of multiplicities, sum of multiplicity * the gathering query's coordinates}.

EXACT cases -- one wrong, missing or doubled term anywhere shows, because every float32 step of both kernels is exact
whatever its order:
    p in [-2, 2]^3 integers, r in {1/2, 1, 2} (1.0f / r exact): relative positions / r are multiples of 1/2, |.| <= 8;
    Wp in [-1, 1], Wf in [-2, 2] and f in [-2, 2]^4 integers: U = Wf f an integer, |U| <= 16, |y| <= 40;
    gsel an integer in [-16, 16]; D in +-{0, 1/8, 1/4} (zero in half of the channels); E a multiple of 1/8, |E| <= 1.
y is a multiple of 1/2, y^2 of 1/4, D y + E of 1/16, dU, dT and dp's channel sum of 1/16.  `exact_range` proves per case,
from the case's own values, that every sum of magnitudes stays below 2^24 of its unit.  Points come as f with an integer
Wf (4 feature channels) so that the literal composed statement -- gather, concatenate, multiply by W = [Wp | Wf], take the
extremum -- can be evaluated beside the reference.

Graph kinds (K = 32, every index in [0, N)):
    ball     rows with the ball-query structure: c distinct hits, then copies of slot 0 (c fixed per case, or drawn per
             row: `c == 0` in the table);
    whole    row q takes form q mod 5:  [a, b, a, c, ...] (slot 0's point recurs among the hits: kept whole),
             [a, a, b, a, ...] (a copy of slot 0 before the first hit: kept whole), [a, b, b, c, a, a, ...] (a repeat
             among the hits: the differing slots are contiguous, so the row FOLDS, with b in two rows), a permutation of
             32 distinct points (N >= 32; else as the next), random slots with repeats;
    mixed    every query draws one of the six forms above;
    ties     the cloud holds N // 3 distinct points, every one under at least three indices (coordinates and U rows
             alike).  Row q takes form q mod 4:  0, 2: slot k and slot k + 16 hold the same point under different indices
             (all 32 slots run); 1: ball-query structure whose hits come in pairs of one point under two indices (folded);
             3: all 32 slots hold ONE point under its different indices, so every y of the row is equal in every channel
             and sel == 0.  The channels [0, 16) have Wp = Wf = 0 besides: y == 0 there in every row;
    ladder   chosen points are gathered by exactly 0, 1, 2, 3, 5, 63, 64, 65, 127, 128, 129 rows (as many as the cloud's N
             queries hold, rotated from cloud to cloud), at most once per query, in slots >= 1 of queries scattered over
             the cloud; the other positions hold random other points;
    outside  (forward only) a ball / whole mix with -1, N, N + 5, INT32_MIN and INT32_MAX in an eighth of the positions.

FLOAT cases -- Gaussian U, p, Wp and g; D, E from BatchNorm's backward constants of the problem's own float64
statistics.  What must equal the float32 restatement bit for bit and the element-wise bars of everything else are
derived at `float_bars`.
"""
import collections

import torch

F64, F32 = torch.float64, torch.float32
EPS = 2.0 ** -24                 # the relative error of one float32 rounding
UP = 1.0 + 2.0 ** -10            # covers the second-order terms of a bar
K = 32
QPB = 64                         # queries per `part` row
C_F = 4                          # feature channels of the exact cases
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1

WIDTHS = (64, 128, 256, 512)
SHAPES = ((1, 1), (5, 13), (3, 7), (1, 63), (2, 65), (3, 77), (2, 128), (2, 200))
LADDER_SHAPES = ((2, 200), (3, 77))
KINDS = ("ball", "whole", "mixed", "ties", "ladder")
BALL_C = (1, 2, 3, 4, 5, 6, 7, 8, 31, 32, 0)             # 0: drawn per row
GAMMAS = ("null", "pos", "mixed", "zeros")
LDWS = (3, 4, 67)
RADII = (0.5, 1.0, 2.0)
LADDER = (0, 1, 2, 3, 5, 63, 64, 65, 127, 128, 129)

Case = collections.namedtuple("Case", "name seed B N H kind c ldw gamma train dp r")


def rows_in_flight(H):
    """G of la_pool_fwd_kernel / la_pool_bwd_kernel: rows (list entries) loaded per step."""
    return 2 if H // 64 >= 8 else 4


def tail_class(H, c):
    """(c mod G, c < G): how the loop over a folded row's c rows ends."""
    G = rows_in_flight(H)
    return c % G, c < G


def _table():
    cases = []
    for h, H in enumerate(WIDTHS):
        plan = [("ball", c) for c in BALL_C] + [(kind, 0) for kind in KINDS[1:] for _ in range(2)]
        for j, (kind, c) in enumerate(plan):
            i = len(cases)
            if kind == "ladder":
                B, N = LADDER_SHAPES[j % 2]
            else:
                fit = [s for s in SHAPES[:7] if s[1] >= max(c, 1 if kind == "ball" else 7)]
                B, N = fit[(i + h) % len(fit)]
            ldw, gamma = LDWS[i % 3], GAMMAS[(i + i // 4) % 4]
            train, dp, r = (i // 2 + i // 8) % 4 != 0, (i + i // 3) % 2 == 0, RADII[(i + i // 3) % 3]
            if kind == "ladder":                               # the long lists in both modes at every width
                train = (j + h) % 2 == 0
            name = (f"H{H}-{kind}{c if kind == 'ball' else ''}-B{B}N{N}-ldw{ldw}-{gamma}-{'train' if train else 'eval'}"
                    f"-{'dp' if dp else 'nodp'}-r{r}")
            cases.append(Case(name, 900 + i, B, N, H, kind, c, ldw, gamma, train, dp, r))
    return cases


CASES = _table()
CASE_IDS = [c.name for c in CASES]


# ---- graphs -------------------------------------------------------------------------------------------------------------

def _distinct(N, gen):
    """A random order of the cloud's points, repeated to at least 32 entries."""
    perm = torch.randperm(N, generator=gen)
    return perm.repeat((K + N - 1) // N + 1)


def ball_row(N, c, gen):
    """c distinct hits (capped by N), then copies of slot 0."""
    c = max(1, min(c, N, K))
    pts = torch.randperm(N, generator=gen)[:c]
    return torch.cat([pts, pts[:1].expand(K - c)])


def whole_row(N, form, gen):
    """The `whole` forms 0..4 of the header; N >= 4."""
    pts = _distinct(N, gen)
    a, b, c = pts[0], pts[1], pts[2]
    rest = lambda n: pts[3:3 + n] if N >= K else pts[3 + torch.randint(0, max(1, N - 3), (n,), generator=gen)]
    if form == 0:
        return torch.cat([torch.stack([a, b, a, c]), rest(K - 4)])
    if form == 1:
        return torch.cat([torch.stack([a, a, b, a]), rest(K - 4)])
    if form == 2:
        return torch.cat([torch.stack([a, b, b, c]), a.expand(K - 4)])
    if form == 3 and N >= K:
        return pts[:K].clone()
    return torch.randint(0, N, (K,), generator=gen)


def ball_graph(B, N, c, gen):
    rows = [ball_row(N, c if c else int(torch.randint(1, K + 1, (1,), generator=gen)), gen) for _ in range(B * N)]
    return torch.stack(rows).view(B, N, K).int()


def whole_graph(B, N, gen):
    return torch.stack([whole_row(N, q % 5, gen) for q in range(B * N)]).view(B, N, K).int()


def mixed_graph(B, N, gen):
    rows = []
    for _ in range(B * N):
        form = int(torch.randint(0, 6, (1,), generator=gen))
        rows.append(ball_row(N, int(torch.randint(1, K + 1, (1,), generator=gen)), gen) if form == 5 else whole_row(N, form, gen))
    return torch.stack(rows).view(B, N, K).int()


def palette(N):
    """ties: point j is a copy of point j mod P, P = N // 3 distinct points (every one held by >= 3 indices)."""
    return max(1, N // 3)


def ties_graph(B, N, gen):
    P = palette(N)
    members = torch.tensor([(N - p + P - 1) // P for p in range(P)])             # copies of palette point p: p, p + P, ...
    k = torch.arange(K)
    rows = []
    for q in range(B * N):
        form = q % 4
        start = int(torch.randint(0, 3, (1,), generator=gen))
        if form in (0, 2):
            pal = torch.randint(0, P, (K // 2,), generator=gen)[k % (K // 2)]
            row = pal + ((k // (K // 2) + start) % members[pal]) * P
        elif form == 1:
            m = int(torch.randint(1, min(P, K // 2) + 1, (1,), generator=gen))
            pal = torch.randperm(P, generator=gen)[:m][torch.arange(2 * m) // 2]
            hits = pal + ((torch.arange(2 * m) % 2 + start) % members[pal]) * P
            row = torch.cat([hits, hits[:1].expand(K - 2 * m)])
        else:
            pal = torch.randint(0, P, (1,), generator=gen).expand(K)
            row = pal + ((k + start) % members[pal]) * P
        rows.append(row)
    return torch.stack(rows).view(B, N, K).int()


def ladder_graph(B, N, gen, rotate=0):
    """-> idx, and per cloud {point: rows that gather it} of the ladder's points."""
    idx = torch.empty(B, N, K, dtype=torch.int64)
    made = []
    for b in range(B):
        pts = torch.randperm(N, generator=gen).tolist()
        r = (rotate + 4 * b) % len(LADDER)
        taken = {}
        for cnt in LADDER[r:] + LADDER[:r]:
            if cnt <= N and len(pts) > N // 2:
                taken[pts.pop()] = cnt
        others = torch.tensor(pts)
        rows = others[torch.randint(0, len(pts), (N, K), generator=gen)]
        free = [torch.randperm(K - 1, generator=gen).tolist() for _ in range(N)]          # slots 1..31 of every query
        for p, cnt in taken.items():
            for q in torch.randperm(N, generator=gen)[:cnt].tolist():
                rows[q, 1 + free[q].pop()] = p
        idx[b] = rows
        made.append(taken)
    return idx.int(), made


def outside_values(N):
    return (-1, N, N + 5, INT32_MIN, INT32_MAX)


def outside_graph(B, N, gen):
    idx = mixed_graph(B, N, gen).long().reshape(-1)
    where = torch.randperm(idx.numel(), generator=gen)[:max(5, idx.numel() // 8)]
    idx[where] = torch.tensor(outside_values(N))[torch.arange(len(where)) % 5]
    return idx.view(B, N, K).int()


def clamped(idx):
    """idx with every entry brought into its cloud, as apn_la_pool_fwd does before anything else."""
    return idx.clamp(0, idx.shape[1] - 1)


# ---- the index stage's statement ----------------------------------------------------------------------------------------

def ball_structure(idx):
    """-> (has the ball-query structure (B,N) bool, c (B,N) = 1 + the slots that differ from slot 0)."""
    differ = idx != idx[..., :1]
    c = differ.sum(-1) + 1
    k = torch.arange(K)
    return (differ == ((k >= 1) & (k < c.unsqueeze(-1)))).all(-1), c


def gather_rows(idx, p=None):
    """The rows of the index stage, by the point they gather -> dict: cnt (B N,) rows per point; point, query, slot, mult
    (rows,) sorted by (point, query, slot) -- global ids b N + .; occ (B N,) float64 = sum of mult; sp (B N, 3) float64 = sum
    of mult * p[query] (with p); spabs = the same over |p|."""
    B, N, _ = idx.shape
    folded, c = ball_structure(idx)
    k = torch.arange(K)
    live = torch.where(folded.unsqueeze(-1), k < c.unsqueeze(-1), torch.ones((), dtype=torch.bool)).reshape(-1)
    mult = torch.where(folded.unsqueeze(-1) & (k == 0), (K + 1 - c).unsqueeze(-1), torch.ones((), dtype=torch.long)).reshape(-1)
    tgt = (idx.long() + torch.arange(B).view(B, 1, 1) * N).reshape(-1)
    pos = torch.nonzero(live).reshape(-1)                                      # ascending (query, slot)
    order = pos[torch.sort(tgt[pos], stable=True)[1]]
    res = dict(cnt=torch.bincount(tgt[pos], minlength=B * N), point=tgt[order], query=order // K, slot=order % K,
               mult=mult[order])
    res["occ"] = torch.zeros(B * N, dtype=F64).index_add_(0, res["point"], res["mult"].double())
    if p is not None:
        pq = p.double().reshape(B * N, 3)[res["query"]] * res["mult"].double().unsqueeze(-1)
        res["sp"] = torch.zeros(B * N, 3, dtype=F64).index_add_(0, res["point"], pq)
        res["spabs"] = torch.zeros(B * N, 3, dtype=F64).index_add_(0, res["point"], pq.abs())
    return res


# ---- exact inputs -------------------------------------------------------------------------------------------------------

def _choice(values, shape, gen):
    return torch.tensor(values, dtype=F32)[torch.randint(0, len(values), shape, generator=gen)]


def gamma_of(kind, H, gen):
    """-> gamma (H,) float32 or None.  mixed: every third channel negative (both signs in every 64-channel tile); zeros:
    mixed with +0.0 at c % 8 == 0 and -0.0 at c % 8 == 4 (`>= 0` takes the maximum for both)."""
    if kind == "null":
        return None
    gamma = 0.5 + torch.rand(H, generator=gen)
    if kind in ("mixed", "zeros"):
        gamma[torch.arange(H) % 3 == 1] *= -1.0
    if kind == "zeros":
        gamma[torch.arange(H) % 8 == 0] = 0.0
        gamma[torch.arange(H) % 8 == 4] = -0.0
    return gamma


def graph_of(kind, B, N, c, gen, rotate=0):
    if kind == "ball":
        return ball_graph(B, N, c, gen), None
    if kind == "whole":
        return whole_graph(B, N, gen), None
    if kind == "mixed":
        return mixed_graph(B, N, gen), None
    if kind == "ties":
        return ties_graph(B, N, gen), None
    return ladder_graph(B, N, gen, rotate)


def exact_inputs(case):
    """-> dict of CPU tensors: p (B,N,3), f (B,N,4), W (H,7) = [Wp | Wf], U (B,N,H) = Wf f, wp (H,ldw) = Wp with NaN in
    every column at or past 3, idx (B,N,32) int32, gamma (H,) | None, gsel (B,N,H), de (2H,) = {D, E} (the training-mode
    values: eval mode runs with zeros), r, and for a ladder graph `ladder`: per cloud {point: rows that gather it}."""
    B, N, H = case.B, case.N, case.H
    gen = torch.Generator().manual_seed(case.seed)
    p = torch.randint(-2, 3, (B, N, 3), generator=gen).float()
    f = torch.randint(-2, 3, (B, N, C_F), generator=gen).float()
    Wp = torch.randint(-1, 2, (H, 3), generator=gen).float()
    Wf = torch.randint(-2, 3, (H, C_F), generator=gen).float()
    if case.kind == "ties":
        P = palette(N)
        p, f = p[:, torch.arange(N) % P], f[:, torch.arange(N) % P]
        Wp[:16], Wf[:16] = 0.0, 0.0
    wp = torch.full((H, case.ldw), float("nan"))
    wp[:, :3] = Wp
    idx, ladder = graph_of(case.kind, B, N, case.c, gen, rotate=case.seed)
    D = _choice([0.0, 0.0, 0.0, 0.0, 0.125, -0.125, 0.25, -0.25], (H,), gen)
    E = torch.randint(-8, 9, (H,), generator=gen).float() / 8.0
    inp = dict(p=p, f=f, W=torch.cat([Wp, Wf], 1), U=f @ Wf.t(), wp=wp, idx=idx, gamma=gamma_of(case.gamma, H, gen),
               gsel=torch.randint(-16, 17, (B, N, H), generator=gen).float(), de=torch.cat([D, E]), r=case.r)
    if ladder is not None:
        inp["ladder"] = ladder
    return inp


# ---- reference ----------------------------------------------------------------------------------------------------------

def _take(t, j):
    """t (B,N,C), j (B,N,K) -> t[b, j[b,q,k]] (B,N,K,C)."""
    B, N, C = t.shape
    return torch.gather(t.unsqueeze(1).expand(-1, N, -1, -1), 2, j.unsqueeze(-1).expand(-1, -1, -1, C))


def positions(U, p, Wp, idx, r):
    """y (B,N,32,H) float64."""
    j = idx.long()
    return _take(U.double(), j) + ((_take(p.double(), j) - p.double().unsqueeze(2)) / float(r)) @ Wp.double().t()


def sign_of(gamma, H, dtype=F64):
    return torch.ones(H, dtype=dtype) if gamma is None else torch.where(gamma >= 0, 1.0, -1.0).to(dtype)


def _extremum(y, sign):
    """y (B,N,32,H) -> ext, sel (first slot that attains it)."""
    t = y * sign
    best = t.max(2)[0]
    slots = torch.arange(K).view(1, 1, K, 1).expand_as(t)
    sel = torch.where(t == best.unsqueeze(2), slots, K).min(2)[0]
    return best * sign, sel.to(torch.uint8)


def part_rows(B, N):
    return (B * N + QPB - 1) // QPB


def _by_workgroup(t):
    """t (B,N,H) float64 -> (rows, H): summed over every 64 consecutive flat queries."""
    B, N, H = t.shape
    return torch.zeros(part_rows(B, N), H, dtype=F64).index_add_(0, torch.arange(B * N) // QPB, t.reshape(B * N, H))


def pool_fwd(U, p, Wp, idx, gamma, r):
    """-> dict: y (B,N,32,H), ext, sel, ysum (B,N,H), part (rows, 2H), sums (2H + 2,) -- float64."""
    B, N, H = U.shape
    y = positions(U, p, Wp, idx, r)
    ext, sel = _extremum(y, sign_of(gamma, H))
    ysum = y.sum(2)
    part = torch.cat([_by_workgroup(ysum), _by_workgroup((y * y).sum(2))], 1)
    sums = torch.cat([part.sum(0), torch.tensor([float(B * N * K), 1.0], dtype=F64)])
    return dict(y=y, ext=ext, sel=sel, ysum=ysum, part=part, sums=sums)


def pool_bwd(y, gsel, sel, ysum, idx, de, Wp, r):
    """y (B,N,32,H) float64; gsel, ysum (B,N,H); de (2H,) or None (eval mode: D = E = 0) -> dU, dT (B,N,H), dp (B,N,3)."""
    B, N, _, H = y.shape
    g = gsel.double()
    hit = sel.unsqueeze(2) == torch.arange(K, dtype=torch.uint8).view(1, 1, K, 1)
    dy = torch.where(hit, g.unsqueeze(2), torch.zeros((), dtype=F64))
    own = g
    if de is not None:
        D, E = de[:H].double(), de[H:].double()
        dy = dy + D * y + E
        own = g + D * ysum.double() + K * E
    tgt = (idx.long() + torch.arange(B).view(B, 1, 1) * N).reshape(-1)
    dU = torch.zeros(B * N, H, dtype=F64).index_add_(0, tgt, dy.reshape(B * N * K, H)).view(B, N, H)
    dT = dU - own
    return dU, dT, dT @ Wp.double() / float(r)


def expected(case, inp):
    """Every entry's answer for a case in the case's own mode: dict of float64 / integer tensors (and `rows`, the index
    stage's statement)."""
    Wp = inp["W"][:, :3]
    want = pool_fwd(inp["U"], inp["p"], Wp, inp["idx"], inp["gamma"], inp["r"])
    de = inp["de"] if case.train else None
    want["dU"], want["dT"], want["dp"] = pool_bwd(want["y"], inp["gsel"], want["sel"], want["ysum"], inp["idx"], de, Wp, inp["r"])
    want["rows"] = gather_rows(inp["idx"], inp["p"])
    return want


def exact_range(case, inp, want):
    """The exactness argument checked on the case's own values: every input has the stated form, and every sum a kernel
    forms in float32 -- bounded by its sum of magnitudes, so in any order -- is below 2^24 of the unit all its terms are
    multiples of.  -> {accumulation: largest sum of magnitudes in its unit}; raises AssertionError otherwise."""
    B, N, H = case.B, case.N, case.H
    whole = lambda t, unit: bool((t / unit == torch.round(t / unit)).all())
    p, U, Wp, g = inp["p"].double(), inp["U"].double(), inp["W"][:, :3].double(), inp["gsel"].double()
    r = float(inp["r"])
    assert r in RADII and whole(p, 1) and float(p.abs().max()) <= 2 and whole(U, 1) and float(U.abs().max()) <= 16
    assert whole(Wp, 1) and float(Wp.abs().max()) <= 1 and whole(g, 1) and float(g.abs().max()) <= 16
    assert torch.equal(inp["wp"][:, :3].double(), Wp) and bool(torch.isnan(inp["wp"][:, 3:]).all())
    assert bool(((inp["idx"] >= 0) & (inp["idx"] < N)).all())
    D, E = inp["de"][:H].double().abs(), inp["de"][H:].double().abs()
    assert set(D.tolist()) <= {0.0, 0.125, 0.25} and whole(E, 0.125) and float(E.max()) <= 1
    if not case.train:
        D, E = D * 0, E * 0
    y = want["y"]
    assert whole(y, 0.5)
    sums = {}
    # la_pool_fwd: per query the sums over the 32 positions (a folded row: the same terms, slot 0's taken 33 - c times)
    sums["ysum"] = float(y.abs().sum(2).max()) * 2
    sums["y^2"] = float((y * y).sum(2).max()) * 4
    # the index stage: geo = {occ, SP}, integers
    rows = want["rows"]
    occ, spabs = rows["occ"].view(B * N, 1), rows["spabs"]
    sums["geo"] = float(max(occ.max(), spabs.max()))
    # la_pool_bwd: occ p - SP (integers), the gathered sum of y (unit 1/2), dU, dT (unit 1/16), dp's channel sum (1/16)
    flat = lambda t: t.reshape(B * N, -1)
    rel = (occ * flat(p).abs() + spabs) / r                                      # (B N, 3)
    sums["occ p - SP"] = float((occ * flat(p).abs() + spabs).max())
    sums["occ U"] = float((occ * flat(U).abs()).max())
    ygath = occ * flat(U).abs() + rel @ Wp.abs().t()
    sums["gathered y"] = float(ygath.max()) * 2
    hit = want["sel"].unsqueeze(2) == torch.arange(K, dtype=torch.uint8).view(1, 1, K, 1)
    contrib = torch.where(hit, g.abs().unsqueeze(2), torch.zeros((), dtype=F64)).reshape(B * N * K, H)
    tgt = (inp["idx"].long() + torch.arange(B).view(B, 1, 1) * N).reshape(-1)
    acc = torch.zeros(B * N, H, dtype=F64).index_add_(0, tgt, contrib)
    du = acc + D * ygath + occ * E
    dt = du + flat(g).abs() + D * flat(want["ysum"]).abs() + K * E
    assert whole(want["dU"], 1 / 16) and whole(want["dT"], 1 / 16) and whole(want["dp"], 1 / 32)
    sums["dU"], sums["dT"] = float(du.max()) * 16, float(dt.max()) * 16
    sums["dp"] = float((dt @ Wp.abs()).max()) * 16
    sums["longest list"] = float(rows["cnt"].max())
    for name, s in sums.items():
        assert s < 2 ** 24, (case.name, name, s)
    return sums


# ---- float32 forms ------------------------------------------------------------------------------------------------------

def _fma(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def positions_f32(U, p, Wp, idx, r):
    """y (B,N,32,H) float32, every step as the kernel's header states it: (p[idx] - p[q]) / r, then
    fma(rz, Wz, fma(ry, Wy, rx * Wx)), then U[idx] + that."""
    j = idx.long()
    rel = (_take(p.float(), j) - p.float().unsqueeze(2)) / torch.tensor(r, dtype=F32)
    rx, ry, rz = (rel[..., i:i + 1] for i in range(3))
    w = Wp.float()
    dot = _fma(rz, w[:, 2], _fma(ry, w[:, 1], rx * w[:, 0]))
    return _take(U.float(), j) + dot


def pool_fwd_f32(U, p, Wp, idx, gamma, r):
    """-> ext, sel, ysum in float32 with the kernel's order of operations."""
    H = U.shape[2]
    y = positions_f32(U, p, Wp, idx, r)
    ext, sel = _extremum(y, sign_of(gamma, H, F32))
    folded, c = ball_structure(idx)
    mult0 = torch.where(folded, (K + 1 - c), torch.ones((), dtype=torch.long)).float().unsqueeze(-1)
    rows = torch.where(folded, c, torch.full((), K))
    ysum = mult0 * y[:, :, 0]
    for k in range(1, K):
        ysum = torch.where((k < rows).unsqueeze(-1), ysum + y[:, :, k], ysum)
    return ext, sel, ysum


def du_eval_f32(gsel, sel, rows):
    """Eval-mode dU (B N, H) float32: every list added in ascending row id, one float32 add per entry from 0."""
    BN, H = gsel.shape[0] * gsel.shape[1], gsel.shape[2]
    g, s = gsel.float().reshape(BN, H), sel.reshape(BN, H)
    term = torch.where(s[rows["query"]] == rows["slot"].to(torch.uint8).unsqueeze(-1), g[rows["query"]], torch.zeros(()))
    start = torch.cumsum(rows["cnt"], 0) - rows["cnt"]
    rank = torch.arange(len(rows["point"])) - start[rows["point"]]
    acc = torch.zeros(BN, H)
    by_rank = torch.sort(rank, stable=True)[1]
    at = 0
    for n_r in torch.bincount(rank).tolist():                                  # the r-th entry of every list that has one
        e = by_rank[at:at + n_r]
        at += n_r
        acc[rows["point"][e]] = acc[rows["point"][e]] + term[e]
    return acc.view(gsel.shape)


# ---- float cases --------------------------------------------------------------------------------------------------------

Float = collections.namedtuple("Float", "name seed B N H kind r")
_FLOAT_PLAN = (((2, 65), "ball", 0.25), ((3, 77), "whole", 0.5), ((5, 13), "mixed", 2.0))       # r = 0.3 in every other case
FLOAT = [Float(f"H{H}-B{B}N{N}-{kind}-r{0.3 if (h + s) % 2 == 0 else r}", 11 * h + s, B, N, H, kind, 0.3 if (h + s) % 2 == 0 else r)
         for h, H in enumerate(WIDTHS) for s, ((B, N), kind, r) in enumerate(_FLOAT_PLAN)]
FLOAT_IDS = [c.name for c in FLOAT]
BN_EPS = 1e-5
SEL_DROP_CAP = 1e-3


def float_inputs(case):
    """Gaussian U, p, Wp and g; gamma Gaussian (mixed signs); gsel = g gamma invstd and de = {D, E} =
    {-gamma invstd^2 S2 / count, -gamma invstd S1 / count - D mean}, S1 = sum g, S2 = sum g (ext - mean) invstd:
    BatchNorm's backward with the problem's own float64 statistics (no ReLU gate).  wp has one NaN pad column."""
    B, N, H = case.B, case.N, case.H
    gen = torch.Generator().manual_seed(700 + case.seed)
    U, p = torch.randn(B, N, H, generator=gen), torch.randn(B, N, 3, generator=gen)
    Wp = torch.randn(H, 3, generator=gen)
    idx, _ = graph_of(case.kind, B, N, 0, gen)
    gamma, g = torch.randn(H, generator=gen), torch.randn(B, N, H, generator=gen)
    ref = pool_fwd(U, p, Wp, idx, gamma, torch.tensor(case.r, dtype=F32).item())
    count = float(B * N * K)
    mean = ref["sums"][:H] / count
    invstd = 1.0 / torch.sqrt(ref["sums"][H:2 * H] / count - mean * mean + BN_EPS)
    g64, gm = g.double(), gamma.double()
    S1, S2 = g64.sum((0, 1)), (g64 * (ref["ext"] - mean) * invstd).sum((0, 1))
    D = -gm * invstd * invstd * S2 / count
    E = -gm * invstd * S1 / count - D * mean
    wp = torch.full((H, 4), float("nan"))
    wp[:, :3] = Wp
    return dict(U=U, p=p, W=Wp, wp=wp, idx=idx, gamma=gamma, gsel=(g64 * gm * invstd).float(), de=torch.cat([D, E]).float(),
                r=torch.tensor(case.r, dtype=F32).item())


def y_bar(U, p, Wp, idx, r):
    """Bar on |y_float32 - y_float64| per position (B,N,32,H).  With A = |rx Wx| + |ry Wy| + |rz Wz|: each relative
    coordinate carries the subtraction's and the division's rounding (2 EPS A), the product one on its term, the two fma one
    each on their partial sums (<= 3 EPS A), the last add one on |U| + A:  EPS (6 A + |U|)."""
    j = idx.long()
    A = ((_take(p.double(), j) - p.double().unsqueeze(2)).abs() / float(r)) @ Wp.double().abs().t()
    return EPS * UP * (6 * A + _take(U.double(), j).abs())


def sel_margin(y, ybar, idx, sign):
    """The float64 extremum's lead over the best position that holds ANOTHER point, minus the two positions' bars:
    (B,N,H); <= 0 where float32 may pick another neighbour (a copy of the same point ties exactly in both precisions, and
    both take the first)."""
    t = y * sign
    best, at = t.max(2)
    winner = torch.gather(idx.long().unsqueeze(-1).expand_as(t), 2, at.unsqueeze(2))                # (B,N,1,H)
    other = idx.long().unsqueeze(-1).expand_as(t) != winner
    rival = torch.where(other, t + ybar, torch.full((), -float("inf"), dtype=F64)).max(2)[0]
    return best - torch.gather(ybar, 2, at.unsqueeze(2)).squeeze(2) - rival


def float_bars(inp, rows, ysum, sel, geo_cnt=None):
    """Element-wise bars on |kernel - float64|, each from the kernel's arithmetic on float32 inputs (EPS = 2^-24 per
    rounding, UP for the second-order terms), the float64 reference taking the SAME float32 inputs; ysum and sel are the
    forward kernel's outputs (the backward reads them).  H = 64 VEC channels, a lane per VEC of them.

    ext, sel, ysum   no bar at a power-of-two radius: the float32 restatement `pool_fwd_f32` must match bit for bit.  `ext`
                     below is y's bar at the selected position, for a radius whose division the device might round otherwise.
    part1            the float64 sum of the float32 ysum values of 64 queries: bar 2^-40 sum |ysum|.
    part2            per query sum_k y^2 in float32: y's own error enters as 2 |y| ybar, m y, the first product and the
                     fma of every further row one rounding each on the running sum: <= (32 + 2) EPS sum y^2; the float64 sums
                     across queries: 2^-40.
    sums             column sums of part in float64: 2^-40 sum |part|.
    geo              occ an integer below 2^24: exact; SP one fma per entry of the list (or per lane, then six butterfly
                     adds): <= (cnt + 6) EPS sum mult |p[query]|.
    dU               acc: one add per entry, <= cnt EPS G, G = sum |gsel [slot == sel]| over the list.  The gathered sum of y =
                     fma(occ, U, Wp . (occ p - SP) / r): SP's bar, the product occ p, the subtraction, 1 / r and the product
                     with it (cnt + 6 + 4 roundings on R = (occ |p| + sum mult |p[query]|) / r), the coordinate product and two fma
                     (3 on RW = R . |Wp|), the last fma one on occ |U| + RW: <= EPS ((cnt + 14) RW + occ |U|).  occ E: 1; the fma
                     with D: 1; the add to acc: 1.  Together <= (cnt + 16) EPS (G + |D| (occ |U| + RW) + occ |E|).
    dT               dU's bar + the fma D ysum + 32 E, the add of gsel, the subtraction: 3 EPS (|dU| + |gsel| + |D ysum| + 32 |E|).
    dp               sum_c dT_c Wp_c: dT's bar through |Wp|, VEC fma per lane + six butterfly adds + the product with 1 / r and
                     its own rounding: (H / 64 + 8) EPS sum |dT_c Wp_c|; all over r.
    -> dict of float64 bars (ybar, part1, part2, geo, dU, dT, dp; each shaped as its quantity)."""
    U, p, Wp, idx, r = inp["U"], inp["p"], inp["W"][:, :3], inp["idx"], float(inp["r"])
    B, N, H = U.shape
    y = positions(U, p, Wp, idx, r)
    ybar = y_bar(U, p, Wp, idx, r)
    bars = {"ybar": ybar}
    bars["part1"] = _by_workgroup(ysum.double().abs()) * 2.0 ** -40
    q2 = (y * y).sum(2) * (K + 2) * EPS * UP + 2 * (y.abs() * ybar).sum(2) * UP
    bars["part2"] = _by_workgroup(q2) + _by_workgroup((y * y).sum(2)) * 2.0 ** -40
    cnt, occ, spabs = rows["cnt"].double().view(-1, 1), rows["occ"].view(-1, 1), rows["spabs"]
    bars["geo"] = torch.cat([torch.zeros(B * N, 1, dtype=F64), (cnt + 6) * EPS * UP * spabs], 1)
    flat = lambda t: t.double().reshape(B * N, -1)
    D, E = inp["de"][:H].double().abs(), inp["de"][H:].double().abs()
    RW = ((occ * flat(p).abs() + spabs) / r) @ Wp.double().abs().t()
    g = flat(inp["gsel"]).abs()
    hit = sel.reshape(B * N, H)[rows["query"]] == rows["slot"].to(torch.uint8).unsqueeze(-1)
    G = torch.zeros(B * N, H, dtype=F64).index_add_(0, rows["point"], torch.where(hit, g[rows["query"]], torch.zeros((), dtype=F64)))
    mag = G + D * (occ * flat(U).abs() + RW) + occ * E
    bars["dU"] = ((cnt + 16) * EPS * UP * mag).view(B, N, H)
    own = g + D * flat(ysum).abs() + K * E
    bars["dT"] = bars["dU"] + (3 * EPS * UP * (mag + own)).view(B, N, H)
    bars["dp"] = ((flat(bars["dT"]) @ Wp.double().abs() + (H // 64 + 8) * EPS * UP * ((mag + own) @ Wp.double().abs())) / r).view(B, N, 3)
    return bars
