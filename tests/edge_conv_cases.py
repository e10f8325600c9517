"""The problems tests/test_gpu_edge_conv_cases.py gives the raw entries of csrc/edge_conv.hip (apn_ec_csr, apn_ec_pool_fwd,
apn_ec_out_res, apn_ec_bwd_prep_act, apn_ec_pool_bwd), in plain torch (no extension): the case table, the input
generators and a reference of every entry.  tests/test_edge_conv_cases_cpu.py checks the table and the reference on the
CPU.

REFERENCE -- each entry restated from the header comment of csrc/edge_conv.hip as gathers over (b, i, k) and one loop
over the K slots (`pool_fwd`, `out`, `bwd_prep`, `csr`, `pool_bwd`); nothing of the kernels' tiling, waves or rows in
flight.  It runs in float64, or in float32 where the kernels' own order of float32 additions is part of the statement
(`pool_fwd`: ysum in slot order; `pool_bwd`: each reverse list in ascending position).

EXACT cases -- one wrong, missing or doubled term anywhere shows, because every float32 step of every kernel is exact
whatever its order:
    x in [-4, 4]^4, Wa - Wb and Wb in [-8, 8]: u = (Wa - Wb) x and v = Wb x are integers in [-128, 128], |y| <= 256 and
        the sum over K <= 64 slots of y^2 is at most 2^22;
    g an integer in [-64, 64]; the residual an integer in [-16, 16];
    scale in +-{1/4, 1/2, 1, 2} with the sign of gamma (+-0.0 under a gamma of +-0.0: BatchNorm's own fold), every sign in
        every 64-channel tile of a mixed gamma; shift in [-8, 8] and mean in [-4, 4] integers; invstd in {1/2, 1, 2};
    D in +-{0, 1/8, 1/4}; E a multiple of 1/8 with |E| <= 4; slope in {0, 1/4}.
Every intermediate is then an integer multiple of 2^-4 (2^-3 in partS's second half) and `exact_range` proves per case,
from the case's own values, that every sum of magnitudes stays below 2^24 of that unit -- the longest reverse list
included.  Points come as x with an integer W (C = 4 input channels) so that the literal composed statement -- gather
x_j - x_i, multiply by W, affine, activation, max over K -- can be evaluated beside the reference.

Graph kinds:
    knn      random distinct neighbours (repeats only where K > N);
    ties     the cloud holds N // 3 distinct points, every one at least three times, the first of them at the origin
             (v = 0 in every channel); every slot's point occurs in the row once more under ANOTHER index, so with
             K >= 2 every (query, channel) extremum is attained by at least two different neighbours;
    ladder   chosen points are gathered exactly 0, 1, 2, 3, 5, 63, 64, 65, 127, 128, 129 times (as many of these as the
             cloud's N K positions hold, rotated from cloud to cloud and case to case), one sink point takes the rest;
             the positions of a list are scattered over the cloud;
    outside  a knn graph with -1, n, n + 5, INT32_MIN and INT32_MAX in an eighth of the positions.

FLOAT cases -- Gaussian uv and g, pack and de from BatchNorm's fold of the problem's own statistics.  What must equal a
float32 restatement bit for bit, and the element-wise bars against float64 of everything else, are derived at
`float_bars`.
"""
import collections

import torch

F64, F32 = torch.float64, torch.float32
EPS = 2.0 ** -24                 # the relative error of one float32 rounding
QPB = 64                         # queries per workgroup of ec_pool_fwd: one `part` row each
TILE = 64                        # points per tile of ec_out / ec_bwd_prep: one partS row per (cloud, tile)
K_MAX = 64
C_IN = 4
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1

WIDTHS = (64, 128, 256, 512)
KS = (1, 2, 3, 4, 5, 6, 7, 8, 20, 33, 63, 64)            # (6: the one class K mod 4 == 2, K >= 4)
SHAPES = ((1, 1), (1, 63), (2, 65), (3, 77), (2, 128))
KINDS = ("knn", "ties", "ladder", "outside")
LD_PADS = (0, 4, 64)
GAMMAS = ("null", "pos", "mixed", "zeros")
SLOPES = (0.0, 0.25)
RESIDUALS = ("none", "contiguous", "permuted", "expanded")
G_LAYOUTS = ("contiguous", "permuted", "scalar")
LADDER = (0, 1, 2, 3, 5, 63, 64, 65, 127, 128, 129)
CSR_ONLY = ((2, 1025, 3), (1, 2049, 2), (3, 1024, 1))    # csr_scan_kernel's `per` = 2, 3, 1

Case = collections.namedtuple("Case", "name seed B N H K kind ld_pad gamma slope res g")


def rows_in_flight(H):
    """G of ec_pool_fwd_kernel / ec_pool_bwd_kernel: neighbours (list entries) loaded per step."""
    return 2 if H // 64 >= 8 else 4


def tail_class(H, K):
    """(K mod G, K < G): how the loop over the neighbours ends."""
    G = rows_in_flight(H)
    return K % G, K < G


# one K per tail class runs with all four graph kinds, the others with one kind each
_ALL_KINDS = {4: (1, 2, 3, 6, 33, 63, 64), 2: (1, 2, 63, 64)}


def _table():
    cases = []
    for h, H in enumerate(WIDTHS):
        for kk, K in enumerate(KS):
            kinds = KINDS if K in _ALL_KINDS[rows_in_flight(H)] else (KINDS[(h + kk) % 4],)
            for kind in kinds:
                i = len(cases)
                if kind == "knn":
                    B, N = SHAPES[i % 5]
                elif kind == "ladder":
                    B, N = SHAPES[2 + i % 3]
                else:
                    B, N = SHAPES[1 + i % 4]
                ld_pad, gamma, slope = LD_PADS[i % 3], GAMMAS[(i + i // 4) % 4], SLOPES[(i // 3) % 2]
                res, g = RESIDUALS[(i // 2 + i // 8) % 4], G_LAYOUTS[(i + i // 3) % 3]
                name = f"H{H}-K{K}-{kind}-B{B}N{N}-ld+{ld_pad}-{gamma}-s{slope}-res:{res}-g:{g}"
                cases.append(Case(name, 100 + i, B, N, H, K, kind, ld_pad, gamma, slope, res, g))
    return cases


CASES = _table()
CASE_IDS = [c.name for c in CASES]


# ---- graphs -------------------------------------------------------------------------------------------------------------

def knn_graph(B, N, K, gen):
    """Random distinct neighbours per row (K > N: the N points in random order, then random repeats)."""
    idx = torch.rand(B, N, N, generator=gen).argsort(-1)[..., :K]
    if K > N:
        idx = torch.cat([idx, torch.randint(0, N, (B, N, K - N), generator=gen)], -1)
    return idx.int()


def outside_values(N):
    return (-1, N, N + 5, INT32_MIN, INT32_MAX)


def outside_graph(B, N, K, gen):
    idx = knn_graph(B, N, K, gen).long().reshape(-1)
    where = torch.randperm(idx.numel(), generator=gen)[:max(5, idx.numel() // 8)]
    vals = torch.tensor(outside_values(N))
    idx[where] = vals[torch.arange(len(where)) % 5]
    return idx.view(B, N, K).int()


def palette(N):
    """ties: point j is a copy of point j mod P, P = N // 3 distinct points (every one held by >= 3 indices)."""
    return max(1, N // 3)


def ties_graph(B, N, K, gen):
    """Every slot's point occurs once more in its row under another index: slot k holds copy number k // m (rotated by a
    random start per row) of the row's distinct point number k mod m, m = K // 2."""
    P = palette(N)
    m = max(1, K // 2)
    members = torch.tensor([(N - p + P - 1) // P for p in range(P)])              # copies of distinct point p: p, p + P, ...
    chosen = torch.randint(0, P, (B, N, m), generator=gen)
    k = torch.arange(K)
    pal = chosen[..., k % m]                                                     # (B, N, K)
    start = torch.randint(0, 3, (B, N, 1), generator=gen)
    copy = (k // m + start) % members[pal]
    return (pal + copy * P).int()


def ladder_graph(B, N, K, gen, rotate=0):
    """-> idx, and per cloud {point: times gathered} of the ladder's points (the sink is not listed)."""
    idx = torch.empty(B, N * K, dtype=torch.int64)
    made = []
    for b in range(B):
        pts = torch.randperm(N, generator=gen).tolist()
        sink = pts.pop()
        left, taken = N * K, {}
        r = (rotate + 4 * b) % len(LADDER)
        for cnt in LADDER[r:] + LADDER[:r]:
            if cnt <= left and pts:
                taken[pts.pop()] = cnt
                left -= cnt
        order = torch.randperm(N * K, generator=gen)
        tgt = torch.full((N * K,), sink)
        at = 0
        for p, cnt in taken.items():
            tgt[order[at:at + cnt]] = p
            at += cnt
        idx[b] = tgt
        made.append(taken)
    return idx.view(B, N, K).int(), made


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


def exact_inputs(case):
    """-> dict of CPU tensors: x (B,N,4), W (H,8) = [Wa | Wb], uv (B,N,ld) with NaN in the pad columns, idx (B,N,K) int32,
    gamma (H,) | None, pack (4H,) = {scale, shift, mean, invstd}, de (2H,) = {D, E}, g (B,H,N), res (B,H,N) | None (the
    LOGICAL values: the layouts of case.g / case.res are made where the buffers are placed), slope, and for a ladder
    graph `ladder`: per cloud {point: times gathered}."""
    B, N, H, K = case.B, case.N, case.H, case.K
    gen = torch.Generator().manual_seed(case.seed)
    inp = {"slope": case.slope}
    x = torch.randint(-4, 5, (B, N, C_IN), generator=gen).float()
    if case.kind == "ties":
        P = palette(N)
        x[:, 0] = 0.0                                                            # a point at the origin: v = 0 everywhere
        x = x[:, torch.arange(N) % P]
    Wd = torch.randint(-8, 9, (H, C_IN), generator=gen).float()                 # Wa - Wb
    Wb = torch.randint(-8, 9, (H, C_IN), generator=gen).float()
    inp["x"], inp["W"] = x, torch.cat([Wd + Wb, Wb], 1)
    ld = 2 * H + case.ld_pad
    uv = torch.full((B, N, ld), float("nan"))
    uv[..., :H], uv[..., H:2 * H] = x @ Wd.t(), x @ Wb.t()
    inp["uv"] = uv
    if case.kind == "knn":
        idx = knn_graph(B, N, K, gen)
    elif case.kind == "outside":
        idx = outside_graph(B, N, K, gen)
    elif case.kind == "ties":
        idx = ties_graph(B, N, K, gen)
    else:
        idx, inp["ladder"] = ladder_graph(B, N, K, gen, rotate=case.seed)
    inp["idx"] = idx
    gamma = gamma_of(case.gamma, H, gen)
    inp["gamma"] = gamma
    scale = _choice([0.25, 0.5, 1.0, 2.0], (H,), gen)
    if gamma is not None:
        scale = torch.where(gamma == 0, torch.zeros(H), scale)
        scale = torch.copysign(scale, gamma)
    shift = torch.randint(-8, 9, (H,), generator=gen).float()
    mean = torch.randint(-4, 5, (H,), generator=gen).float()
    invstd = _choice([0.5, 1.0, 2.0], (H,), gen)
    inp["pack"] = torch.cat([scale, shift, mean, invstd])
    D = _choice([0.0, 0.125, -0.125, 0.25, -0.25], (H,), gen)
    E = torch.randint(-32, 33, (H,), generator=gen).float() / 8.0
    inp["de"] = torch.cat([D, E])
    if case.g == "scalar":
        inp["g"] = torch.full((B, H, N), float(37 - 74 * (case.seed % 2)))
    else:
        inp["g"] = torch.randint(-64, 65, (B, H, N), generator=gen).float()
    if case.res == "none":
        inp["res"] = None
    elif case.res == "expanded":
        inp["res"] = torch.randint(-16, 17, (1, H, N), generator=gen).float().expand(B, -1, -1)
    else:
        inp["res"] = torch.randint(-16, 17, (B, H, N), generator=gen).float()
    return inp


def clamped(idx):
    """idx with every entry brought into its cloud, as both kernels that read idx do."""
    return idx.clamp(0, idx.shape[1] - 1)


# ---- reference ----------------------------------------------------------------------------------------------------------

def pool_fwd(uv, H, idx, gamma, dtype=F64):
    """uv (B,N,ld) rows [u | v | pad], idx (B,N,K), gamma (H,) | None ->
    ext (B,N,H) = the extremum over k of y[i,k] = u_i + v_j, j = idx[i,k] clamped to [0, N-1]: the maximum where
        gamma >= 0 or gamma is None, else the minimum;
    sel (B,N,H) uint8 = the first slot that holds it;
    ysum (B,N,H) = the sum of y over k, added in slot order in `dtype`;
    part1, part2 (rows, H) float64 = per 64 consecutive queries of the flattened (B N) the sums of ysum and of y^2 (y^2
        from float64 y)."""
    B, N, K = idx.shape
    u, v = uv[..., :H].to(dtype), uv[..., H:2 * H].to(dtype)
    j = clamped(idx.long())
    sign = torch.ones(H, dtype=dtype) if gamma is None else torch.where(gamma >= 0, 1.0, -1.0).to(dtype)
    best = sel = ysum = sq = None
    for k in range(K):
        vj = torch.gather(v, 1, j[:, :, k:k + 1].expand(-1, -1, H))
        y = u + vj
        t = y * sign
        y2 = (u.double() + vj.double()) ** 2
        if k == 0:
            best, sel, ysum, sq = t, torch.zeros(B, N, H, dtype=torch.uint8), y, y2
        else:
            better = t > best
            best = torch.where(better, t, best)
            sel = torch.where(better, torch.tensor(k, dtype=torch.uint8), sel)
            ysum = ysum + y
            sq = sq + y2
    rows = (B * N + QPB - 1) // QPB
    wg = torch.arange(B * N) // QPB
    part1 = torch.zeros(rows, H, dtype=F64).index_add_(0, wg, ysum.double().reshape(B * N, H))
    part2 = torch.zeros(rows, H, dtype=F64).index_add_(0, wg, sq.reshape(B * N, H))
    return best * sign, sel, ysum, part1, part2


def _affine(scale, ext, shift, dtype):
    """scale ext + shift with ONE rounding, as the kernels' fma: formed in float64 (the product of two float32 values is
    exact there), then rounded to `dtype`."""
    return (scale.double() * ext.double() + shift.double()).to(dtype)


def out(ext, pack, slope, res, dtype=F64):
    """-> (B,H,N): z = scale ext + shift; z > 0 ? z : slope z; + res."""
    H = ext.shape[2]
    z = _affine(pack[:H], ext, pack[H:2 * H], dtype)
    o = torch.where(z > 0, z, slope * z).transpose(1, 2)
    return o if res is None else o + res.to(dtype)


def bwd_prep(g, ext, pack, slope, dtype=F64):
    """g (B,H,N) -> gsel (B,N,H) = g act'(z) scale, act' = 1 where z > 0 else slope; partS (B * tiles, 2H) = per (cloud,
    64-point tile) {sum g act', sum g act' (ext - mean) invstd}."""
    B, N, H = ext.shape
    e = ext.to(dtype)
    scale, shift, mean, invstd = (pack[i * H:(i + 1) * H].to(dtype) for i in range(4))
    z = _affine(scale, e, shift, dtype)
    gv = g.to(dtype).transpose(1, 2) * torch.where(z > 0, 1.0, slope).to(dtype)
    tiles = (N + TILE - 1) // TILE
    row = (torch.arange(B).view(B, 1) * tiles + torch.arange(N).view(1, N) // TILE).reshape(-1)
    both = torch.cat([gv, gv * ((e - mean) * invstd)], -1).reshape(B * N, 2 * H)
    partS = torch.zeros(B * tiles, 2 * H, dtype=dtype).index_add_(0, row, both)
    return gv * scale, partS


def targets(idx):
    """(B N K,) int64: the point b N + clamp(idx) every position gathers."""
    B, N, K = idx.shape
    return (clamped(idx.long()) + torch.arange(B).view(B, 1, 1) * N).reshape(-1)


def csr(idx):
    """-> pcnt, poff (B N,), plist (B N K,) int32: the positions by the point they gather, ascending (a stable sort)."""
    B, N, K = idx.shape
    tgt = targets(idx)
    pcnt = torch.bincount(tgt, minlength=B * N)
    return pcnt.int(), (torch.cumsum(pcnt, 0) - pcnt).int(), torch.sort(tgt, stable=True)[1].int()


def pool_bwd(gsel, sel, idx, uv, H, ysum, de, dtype=F64):
    """-> duv (B,N,2H) = [du | dv],
        du_i = gsel_i + D ysum_i + K E
        dv_j = sum_L gsel_i [k == sel_i] + D (sum_L u_i + cnt_j v_j) + cnt_j E,   L = the positions (i, k) that gather j
    ysum None: the dense term is absent (de must be 0).  In float64 the sums over L are index_add_ (exact on these
    inputs in any order); in float32 each list is added in ascending position, one rounding per entry from 0."""
    B, N, K = idx.shape
    tgt = targets(idx)
    hit = sel.reshape(B * N, 1, H) == torch.arange(K, dtype=torch.uint8).view(1, K, 1)
    contrib = torch.where(hit, gsel.to(dtype).reshape(B * N, 1, H), torch.zeros((), dtype=dtype)).reshape(B * N * K, H)
    u, v = uv[..., :H].to(dtype).reshape(B * N, H), uv[..., H:2 * H].to(dtype).reshape(B * N, H)
    dense = ysum is not None
    cnt = torch.bincount(tgt, minlength=B * N)
    acc, us = torch.zeros(B * N, H, dtype=dtype), torch.zeros(B * N, H, dtype=dtype)
    query = torch.arange(B * N * K) // K
    if dtype == F64:
        acc.index_add_(0, tgt, contrib)
        if dense:
            us.index_add_(0, tgt, u[query])
    else:
        st, order = torch.sort(tgt, stable=True)
        rank = torch.arange(B * N * K) - (torch.cumsum(cnt, 0) - cnt)[st]      # place within its list
        by_rank = torch.sort(rank, stable=True)[1]
        at = 0
        for n_r in torch.bincount(rank).tolist():                               # the r-th entry of every list that has one
            pos = order[by_rank[at:at + n_r]]
            at += n_r
            acc[tgt[pos]] = acc[tgt[pos]] + contrib[pos]
            if dense:
                us[tgt[pos]] = us[tgt[pos]] + u[query[pos]]
    D, E = de[:H].to(dtype), de[H:].to(dtype)
    fc = cnt.to(dtype).view(-1, 1)
    du = gsel.to(dtype).reshape(B * N, H) + ((D * ysum.to(dtype).reshape(B * N, H) + K * E) if dense else 0.0)
    dv = acc + (D * (fc * v + us) + fc * E if dense else 0.0)
    return torch.cat([du, dv], -1).view(B, N, 2 * H)


def expected(case, inp):
    """Every entry's answer for a case, each stage from the previous stage's answer: dict of float64 / integer tensors.
    duv: training mode (ysum, de); duv_eval: ysum = None, de = 0."""
    H = case.H
    ext, sel, ysum, p1, p2 = pool_fwd(inp["uv"], H, inp["idx"], inp["gamma"])
    gsel, partS = bwd_prep(inp["g"], ext, inp["pack"], inp["slope"])
    pcnt, poff, plist = csr(inp["idx"])
    return dict(ext=ext, sel=sel, ysum=ysum, part=torch.cat([p1, p2], 1), out=out(ext, inp["pack"], inp["slope"], inp["res"]),
                gsel=gsel, partS=partS, pcnt=pcnt, poff=poff, plist=plist,
                duv=pool_bwd(gsel, sel, inp["idx"], inp["uv"], H, ysum, inp["de"]),
                duv_eval=pool_bwd(gsel, sel, inp["idx"], inp["uv"], H, None, torch.zeros(2 * H)))


def exact_range(case, inp, want):
    """The exactness argument checked on the case's own values: every input has the stated form, and every sum a kernel
    forms in float32 -- bounded by its sum of magnitudes, so in any order -- is below 2^24 of the unit all its terms are
    multiples of.  -> {accumulation: largest sum of magnitudes in its unit}; raises AssertionError otherwise."""
    B, N, H, K = case.B, case.N, case.H, case.K
    whole = lambda t, unit: bool((t / unit == torch.round(t / unit)).all())
    u, v = inp["uv"][..., :H].double(), inp["uv"][..., H:2 * H].double()
    scale, shift, mean, invstd = (inp["pack"][i * H:(i + 1) * H].double() for i in range(4))
    D, E = inp["de"][:H].double(), inp["de"][H:].double()
    g = inp["g"].double()
    assert whole(u, 1) and whole(v, 1) and float(u.abs().max()) <= 128 and float(v.abs().max()) <= 128
    assert bool(torch.isnan(inp["uv"][..., 2 * H:]).all())
    assert whole(g, 1) and float(g.abs().max()) <= 64
    assert set(scale.abs().tolist()) <= {0.0, 0.25, 0.5, 1.0, 2.0} and whole(shift, 1) and whole(mean, 1)
    assert set(invstd.tolist()) <= {0.5, 1.0, 2.0}
    assert set(D.abs().tolist()) <= {0.0, 0.125, 0.25} and whole(E, 0.125) and float(E.abs().max()) <= 4
    assert inp["slope"] in SLOPES
    if inp["gamma"] is not None:
        assert bool((torch.signbit(inp["gamma"]) == torch.signbit(inp["pack"][:H])).all())
    j = clamped(inp["idx"].long())
    tgt = targets(inp["idx"])
    cnt = torch.bincount(tgt, minlength=B * N).double().view(-1, 1)
    query = torch.arange(B * N * K) // K
    sums = {}
    # ec_pool_fwd: sum over k of |y| (unit 1) and of y^2 (unit 1)
    vabs = torch.stack([torch.gather(v, 1, j[:, :, k:k + 1].expand(-1, -1, H)) for k in range(K)], 2)     # (B,N,K,H)
    y = u.unsqueeze(2) + vabs
    sums["ysum"] = float(y.abs().sum(2).max())
    sums["y^2"] = float((y * y).sum(2).max())
    # ec_out: |scale ext| + |shift| in units of 1/4, the activation's product in 1/16, the residual
    ext = want["ext"]
    z = (scale * ext).abs() + shift.abs()
    sums["out"] = float((z + (0 if inp["res"] is None else inp["res"].double().abs().transpose(1, 2))).max()) * 16
    # ec_bwd_prep: gv = g act' a multiple of 1/4, gsel of 1/16; per tile sum |gv| (unit 1/4), sum |gv yhat| (unit 1/8)
    gv = g.transpose(1, 2).abs()
    yhat = ((ext - mean) * invstd).abs()
    assert whole(want["gsel"], 1 / 16) and whole(want["partS"][:, :H], 0.25) and whole(want["partS"][:, H:], 0.125)
    tiles = (N + TILE - 1) // TILE
    row = (torch.arange(B).view(B, 1) * tiles + torch.arange(N).view(1, N) // TILE).reshape(-1)
    both = torch.cat([gv * 4, gv * yhat * 8], -1).reshape(B * N, 2 * H)
    sums["partS"] = float(torch.zeros(B * tiles, 2 * H, dtype=F64).index_add_(0, row, both).max())
    # ec_pool_bwd: du (unit 1/16), the inner sum over the list of u + cnt v (unit 1), dv (unit 1/16)
    gsel = want["gsel"].abs().reshape(B * N, H)
    sums["du"] = float((gsel + D.abs() * want["ysum"].abs().reshape(B * N, H) + K * E.abs()).max()) * 16
    hit = want["sel"].reshape(B * N, 1, H) == torch.arange(K, dtype=torch.uint8).view(1, K, 1)
    contrib = torch.where(hit, gsel.reshape(B * N, 1, H), torch.zeros((), dtype=F64)).reshape(B * N * K, H)
    acc = torch.zeros(B * N, H, dtype=F64).index_add_(0, tgt, contrib)
    inner = torch.zeros(B * N, H, dtype=F64).index_add_(0, tgt, u.reshape(B * N, H).abs()[query]) + cnt * v.reshape(B * N, H).abs()
    sums["list u"] = float(inner.max())
    sums["dv"] = float((acc + D.abs() * inner + cnt * E.abs()).max()) * 16
    sums["longest list"] = float(cnt.max())
    for name, s in sums.items():
        assert s < 2 ** 24, (case.name, name, s)
    return sums


# ---- float cases --------------------------------------------------------------------------------------------------------

Float = collections.namedtuple("Float", "name seed B N H K")
FLOAT = [Float(f"H{H}-B{B}N{N}-K{K}", 7 * h + s, B, N, H, K)
         for h, H in enumerate(WIDTHS) for s, (B, N, K) in enumerate(((2, 65, 5), (3, 77, 20), (2, 65, 64)))]
FLOAT_IDS = [c.name for c in FLOAT]
BN_EPS = 1e-5


def float_inputs(case):
    """Gaussian uv (B,N,2H + 4: one quad of NaN pad) and g (B,H,N), a knn graph, a Gaussian gamma (mixed signs) and beta,
    slope 0.2 and a Gaussian residual.  pack is BatchNorm's fold of the problem's own statistics (float64 sums over all
    (i, k) of y and y^2); de -- {D, E}, BatchNorm's dense term dL/dy = D y + E -- is filled in by `float_dense` from the
    gradient's sums."""
    B, N, H, K = case.B, case.N, case.H, case.K
    gen = torch.Generator().manual_seed(500 + case.seed)
    uv = torch.full((B, N, 2 * H + 4), float("nan"))
    uv[..., :2 * H] = torch.randn(B, N, 2 * H, generator=gen)
    idx = knn_graph(B, N, K, gen)
    gamma, beta = torch.randn(H, generator=gen), torch.randn(H, generator=gen)
    _, _, ysum, _, p2 = pool_fwd(uv, H, idx, gamma)
    count = float(B * N * K)
    mean = ysum.sum((0, 1)) / count
    var = p2.sum(0) / count - mean * mean
    invstd = 1.0 / torch.sqrt(var + BN_EPS)
    scale = gamma.double() * invstd
    pack = torch.cat([scale, beta.double() - mean * scale, mean, invstd]).float()
    return dict(uv=uv, idx=idx, gamma=gamma, pack=pack, slope=0.2, g=torch.randn(B, H, N, generator=gen),
                res=torch.randn(B, H, N, generator=gen), count=count)


def float_dense(inp, partS):
    """de (2H,) float32 from partS (rows, 2H) = {sum g act', sum g act' yhat_sel} per tile:
    D = -gamma invstd^2 S2 / count,  E = -gamma invstd S1 / count - D mean   (BatchNorm's backward, dense part)."""
    H = inp["gamma"].shape[0]
    S = partS.double().sum(0)
    gamma, mean, invstd = inp["gamma"].double(), inp["pack"][2 * H:3 * H].double(), inp["pack"][3 * H:].double()
    D = -gamma * invstd * invstd * S[H:] / inp["count"]
    E = -gamma * invstd * S[:H] / inp["count"] - D * mean
    return torch.cat([D, E]).float()


def float_bars(H, K, idx, uv, pack, slope, res, g, ext, gsel, sel, ysum, de):
    """Element-wise bars on |kernel - float64|, each from the kernel's arithmetic on float32 inputs (EPS = 2^-24 per
    rounding, (1 + 2^-10) for the second-order terms), the float64 reference taking the SAME float32 inputs -- ext, gsel,
    sel and ysum are the previous kernels' outputs.  A gate z > 0 cannot differ between the two: z is one correctly
    rounded fma in the kernel, so it has the sign of the exact value.

    ext, sel, ysum     no bar: y = u + v is one IEEE add, t > best is exact, ysum is K - 1 adds in slot order: the float32
                       restatement `pool_fwd(dtype=float32)` must match bit for bit.
    part2 (y^2 sums)   per y: the add's rounding enters y^2 twice, then the K fma accumulations of the query, then the
                       float64 sums (negligible): <= (K + 2) EPS sum y^2.  The issue's bar (K + 64) EPS sum y^2 covers it.
    part1              the float64 sum of the float32 ysum values: exact to 2^-53: bar 2^-40 sum |ysum|.
    out                z = fma(scale, ext, shift): 1 rounding; z > 0: the activation multiplies by 1 (exact), else by the
                       slope: 1 more; a residual: 1 more on the sum.  Without a residual (`out_nores`, the entry called with
                       res = NULL) at most 2 roundings: <= EPS |z act| (1 + [z <= 0]); with one (`out`)
                       <= EPS (|z act| (1 + [z <= 0]) + |z act| + |res|).
    gsel               g act': exact where z > 0, else 1 rounding; times scale: 1: <= EPS |gsel| (1 + [z <= 0]).
    partS              per term 1 rounding in gv (first half), 3 more in yhat = (ext - mean) invstd and the fma (second
                       half: gv's, the subtraction's, the product's), then 16 adds in a wave and 2 levels across the four
                       waves: <= (64 + 3) EPS sum of the tile's |terms|, the subtraction's rounding counted on
                       |gv| (|ext| + |mean|) invstd.
    du                 K E: 1 rounding, the fma: 1, the add: 1: <= 4 EPS (|gsel| + |D ysum| + |K E|).
    dv                 cnt adds into acc, cnt into the list's sum of u, then fma(cnt, v, .), cnt E, fma(D, ., .) and the
                       last add: <= (cnt + 4) EPS (sum |gsel [sel]| + |D| (sum |u| + cnt |v|) + cnt |E|).
    -> dict of float64 bars: part2, part1, out, out_nores, gsel, partS, duv."""
    B, N, _ = idx.shape
    up = 1.0 + 2.0 ** -10
    u, v = uv[..., :H].double(), uv[..., H:2 * H].double()
    j = clamped(idx.long())
    sq = sum((u + torch.gather(v, 1, j[:, :, k:k + 1].expand(-1, -1, H))) ** 2 for k in range(K))
    rows = (B * N + QPB - 1) // QPB
    wg = torch.arange(B * N) // QPB
    bars = {"part2": torch.zeros(rows, H, dtype=F64).index_add_(0, wg, sq.reshape(B * N, H)) * (K + 64) * EPS,
            "part1": torch.zeros(rows, H, dtype=F64).index_add_(0, wg, ysum.double().abs().reshape(B * N, H)) * 2.0 ** -40}
    scale, shift, mean, invstd = (pack[i * H:(i + 1) * H].double() for i in range(4))
    e = ext.double()
    z = scale * e + shift
    za = torch.where(z > 0, z, slope * z).abs().transpose(1, 2)
    roundings = torch.where(z > 0, 1.0, 2.0)
    bars["out_nores"] = roundings.transpose(1, 2) * za * EPS * up
    bars["out"] = bars["out_nores"] + (0 if res is None else (za + res.double().abs()) * EPS * up)
    bars["gsel"] = roundings * gsel.double().abs() * EPS * up
    gv = (g.double().transpose(1, 2) * torch.where(z > 0, 1.0, slope)).abs()
    tiles = (N + TILE - 1) // TILE
    row = (torch.arange(B).view(B, 1) * tiles + torch.arange(N).view(1, N) // TILE).reshape(-1)
    both = torch.cat([gv, gv * (e.abs() + mean.abs()) * invstd], -1).reshape(B * N, 2 * H)
    bars["partS"] = torch.zeros(B * tiles, 2 * H, dtype=F64).index_add_(0, row, both) * (64 + 3) * EPS * up
    D, E = de[:H].double().abs(), de[H:].double().abs()
    tgt = targets(idx)
    cnt = torch.bincount(tgt, minlength=B * N).double().view(-1, 1)
    query = torch.arange(B * N * K) // K
    ga = gsel.double().abs().reshape(B * N, H)
    hit = sel.reshape(B * N, 1, H) == torch.arange(K, dtype=torch.uint8).view(1, K, 1)
    contrib = torch.where(hit, ga.reshape(B * N, 1, H), torch.zeros((), dtype=F64)).reshape(B * N * K, H)
    acc = torch.zeros(B * N, H, dtype=F64).index_add_(0, tgt, contrib)
    inner = torch.zeros(B * N, H, dtype=F64).index_add_(0, tgt, u.reshape(B * N, H).abs()[query]) + cnt * v.reshape(B * N, H).abs()
    du = 4 * (ga + D * ysum.double().abs().reshape(B * N, H) + K * E) * EPS * up
    dv = (cnt + 4) * (acc + D * inner + cnt * E) * EPS * up
    bars["duv"] = torch.cat([du, dv], -1).view(B, N, 2 * H)
    return bars
