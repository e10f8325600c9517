"""The stacked-cloud operator contract of csrc/pointops.hip (include/adaptpoint_amd.h) stated in numpy
(tests/test_pointops_cpu.py, tests/test_gpu_pointops.py, tests/golden/make_golden_pointops.py).

Every statement takes the precision `f` (np.float64 or np.float32).  In float32 every operation is rounded to float32
in the contract's order -- sums are sequential from their first term (np.cumsum), products are rounded before they are
added, the squared distance is fma(tz, tz, fma(ty, ty, tx * tx)) -- so a kernel can be compared bit for bit.  (The fma
is emulated through float64, exact on lattices and wherever no double rounding occurs.)

Layout: xyz (n,3), features (n,c), offset (b) int32 cumulative ends; queries (m,..) with new_offset (b)."""
import numpy as np

TAU = 6 * 2.0 ** -24            # relative error bar of an fp32 squared distance at C = 3 (tests/chamfer_reference.py)
FAR = 1e10                      # the reference's initial heap distance and `tmp` fill
SIZES = (70, 5, 200, 1, 129, 300)


def offsets(sizes):
    return np.cumsum(np.asarray(sizes, dtype=np.int64)).astype(np.int32)


def quarter(sizes):
    return tuple(s // 4 for s in sizes)


def ranges(offset):
    ends = [int(e) for e in offset]
    return list(zip([0] + ends[:-1], ends))


def cloud_of(q, new_offset):
    """The first cloud i with q < new_offset[i]; rows at or past the last end belong to the last cloud."""
    i = 0
    while i < len(new_offset) - 1 and q >= int(new_offset[i]):
        i += 1
    return i


def query_ranges(m, n, offset, new_offset):
    """(m,2): the support rows [start, end) of every query row, clamped into [0, n]."""
    rg = ranges(offset)
    out = np.empty((m, 2), dtype=np.int64)
    for q in range(m):
        s, e = rg[cloud_of(q, new_offset)]
        s = min(max(s, 0), n)
        out[q] = s, min(max(e, s), n)
    return out


def dist2(q, s, f):
    """(m,n): |q_i - s_j|^2 in precision f; float32: fma(tz, tz, fma(ty, ty, tx * tx)), t = q - s."""
    t = q.astype(f)[:, None, :] - s.astype(f)[None, :, :]
    if f is np.float64:
        return (t * t).sum(-1)
    t = t.astype(np.float64)                                # products of two floats are exact in float64
    inner = (t[..., 1] * t[..., 1] + (t[..., 0] * t[..., 0]).astype(np.float32)).astype(np.float32)
    return (t[..., 2] * t[..., 2] + inner).astype(np.float32)


def knn(k, xyz, new_xyz, offset, new_offset, f):
    """idx (m,k) int32, dist2 (m,k) f: the k smallest (d2, row) keys of the query's own cloud, ascending; the slots a
    short cloud leaves hold (start of the cloud clamped into [0, n), 1e10)."""
    n, m = len(xyz), len(new_xyz)
    idx = np.empty((m, k), dtype=np.int32)
    d2 = np.full((m, k), FAR, dtype=f)
    for q, (s, e) in enumerate(query_ranges(m, n, offset, new_offset)):
        idx[q] = min(s, n - 1)
        d = dist2(new_xyz[q:q + 1], xyz[s:e], f)[0]
        order = np.argsort(d, kind="stable")                # ties: ascending row
        order = order[d[order] < f(FAR)][:k]
        idx[q, :len(order)] = s + order
        d2[q, :len(order)] = d[order]
    return idx, d2


def ball(radius, nsample, xyz, new_xyz, offset, new_offset, f):
    """idx (m,nsample) int32: the first nsample rows of the cloud with d2 < r^2, ascending; the rest repeat the first
    hit; no hit: zeros.  r^2 is the product of the float32 radius with itself, rounded to f."""
    n, m = len(xyz), len(new_xyz)
    r2 = f(np.float32(radius)) * f(np.float32(radius))
    idx = np.zeros((m, nsample), dtype=np.int32)
    for q, (s, e) in enumerate(query_ranges(m, n, offset, new_offset)):
        hits = s + np.nonzero(dist2(new_xyz[q:q + 1], xyz[s:e], f)[0] < r2)[0][:nsample]
        if len(hits):
            idx[q] = hits[0]
            idx[q, :len(hits)] = hits
    return idx


def fps_threads(n_max):
    """T = min(1024, 2^floor(log2 n_max)), the reference's block size."""
    return min(1024, 1 << (int(n_max).bit_length() - 1))


def fps_tree(xyz, offset, new_offset, n_max, f, tmp=None):
    """idx (m) int32 and the final tmp (n): the reference's kernel emulated directly -- T threads, row k on thread
    (k - start) mod T keeping its first maximum, then the block tree (the lower slot wins unless the upper one is strictly
    greater).  Also returned: the smallest gap (best - second best running minimum) / best over all steps."""
    n = len(xyz)
    T = fps_threads(n_max)
    tmp = np.full(n, FAR, dtype=f) if tmp is None else tmp.astype(f).copy()
    idx = np.zeros(int(new_offset[-1]), dtype=np.int32)
    written = np.zeros(len(idx), dtype=bool)
    gap = np.inf
    for (s, e), (sm, em) in zip(ranges(offset), ranges(new_offset)):
        if em <= sm:
            continue                                        # an empty output range writes nothing
        idx[sm], written[sm] = s, True
        old = s
        for j in range(sm + 1, em):
            written[j] = True
            if e <= s:
                idx[j] = s
                continue
            d = np.minimum(dist2(xyz[old:old + 1], xyz[s:e], f)[0], tmp[s:e])
            tmp[s:e] = d
            best = np.full(T, -1.0, dtype=f)
            besti = np.full(T, s, dtype=np.int64)
            for t in range(min(T, e - s)):
                own = d[t::T]
                a = int(np.argmax(own))                     # the first maximum
                best[t], besti[t] = own[a], s + t + a * T
            w = T // 2
            while w >= 1:
                up = best[w:2 * w] > best[:w]               # strict: the lower slot keeps a tie
                besti[:w] = np.where(up, besti[w:2 * w], besti[:w])
                best[:w] = np.maximum(best[:w], best[w:2 * w])
                w //= 2
            old = int(besti[0])
            idx[j] = old
            top = np.sort(d)[::-1][:2]
            if len(top) == 2 and top[0] > 0:
                gap = min(gap, float((top[0] - top[1]) / top[0]))
    return idx, tmp, written, gap


def clamp(idx, n):
    return np.clip(idx.astype(np.int64), 0, n - 1)


def csr(idx, n):
    """pcnt (n), poff (n), plist (m k): row j's list = the positions i k + s with clamp(idx)[i,s] == j, ascending."""
    flat = clamp(idx, n).reshape(-1)
    plist = np.argsort(flat, kind="stable").astype(np.int32)
    pcnt = np.bincount(flat, minlength=n).astype(np.int32)
    poff = (np.cumsum(pcnt) - pcnt).astype(np.int32)
    return pcnt, poff, plist


def _seq(terms, axis):
    """The sequential sum along `axis`, from the first term, in the terms' own precision."""
    return np.take(np.cumsum(terms, axis=axis, dtype=terms.dtype), -1, axis=axis)


def _list_sum(terms, idx, n):
    """(n,c): per support row the sequential sum of terms (m k, c) over its list, in list order; empty: 0."""
    pcnt, poff, plist = csr(idx, n)
    out = np.zeros((n, terms.shape[1]), dtype=terms.dtype)
    for j in np.nonzero(pcnt)[0]:
        out[j] = _seq(terms[plist[poff[j]:poff[j] + pcnt[j]]], 0)
    return out


def grouping_fwd(inp, idx, f):
    return inp.astype(f)[clamp(idx, len(inp))]


def grouping_bwd(grad_out, idx, n, f):
    return _list_sum(grad_out.astype(f).reshape(-1, grad_out.shape[-1]), idx, n)


def interpolation_fwd(inp, idx, weight, f):
    return _seq(inp.astype(f)[clamp(idx, len(inp))] * weight.astype(f)[..., None], 1)


def interpolation_bwd(grad_out, idx, weight, n, f):
    k = idx.shape[1]
    terms = np.repeat(grad_out.astype(f), k, axis=0) * weight.astype(f).reshape(-1, 1)
    return _list_sum(terms, idx, n)


def subtraction_fwd(in1, in2, idx, f):
    return in1.astype(f)[:, None, :] - in2.astype(f)[clamp(idx, len(in2))]


def subtraction_bwd(grad_out, idx, n, f):
    g = grad_out.astype(f)
    return _seq(g, 1), _list_sum(-g.reshape(-1, g.shape[-1]), idx, n)


def _wexp(weight, c, f):
    """weight (m,k,w_c) -> (m,k,c) with channel ch reading ch % w_c."""
    return np.tile(weight.astype(f), (1, 1, c // weight.shape[-1]))


def aggregation_fwd(inp, position, weight, idx, f):
    c = inp.shape[1]
    return _seq((inp.astype(f)[clamp(idx, len(inp))] + position.astype(f)) * _wexp(weight, c, f), 1)


def aggregation_bwd(inp, position, weight, idx, grad_out, f):
    """-> grad_input (n,c), grad_position (m,k,c), grad_weight (m,k,w_c)."""
    n, c = inp.shape
    m, k, w_c = weight.shape
    g = grad_out.astype(f)[:, None, :]
    wexp = _wexp(weight, c, f)
    gpos = g * wexp
    prod = g * (inp.astype(f)[clamp(idx, n)] + position.astype(f))
    gw = _seq(prod.reshape(m, k, c // w_c, w_c), 2)
    return _list_sum(gpos.reshape(-1, c), idx, n), gpos, gw


def interpolation_weights(dist2_, f):
    """The reference's inverse-distance weights from squared kNN distances: sqrt, 1 / (d + 1e-8), normalised."""
    recip = f(1.0) / (np.sqrt(dist2_.astype(f)) + f(1e-8))
    return recip / recip.sum(1, keepdims=True, dtype=f)


# ------------------------------------------------------------------------------------------------ generators
def lattice_clouds(sizes, seed):
    """Stacked clouds of distinct integer lattice points (float32): distances are exact and ties plentiful."""
    rng = np.random.default_rng(seed)
    parts = []
    for s in sizes:
        g = 2
        while g ** 3 < s + s // 2 + 1:
            g += 1
        pick = rng.choice(g ** 3, size=s, replace=False)
        parts.append(np.stack(np.unravel_index(pick, (g, g, g)), -1).astype(np.float32))
    return np.concatenate(parts) if parts else np.zeros((0, 3), np.float32)


def seeded_clouds(sizes, seed):
    """Stacked clouds uniform in [-1, 1]^3 (float32)."""
    return np.random.default_rng(seed).uniform(-1, 1, (int(sum(sizes)), 3)).astype(np.float32)


def features(shape, seed, f=np.float32):
    return np.random.default_rng(seed).standard_normal(shape).astype(f)


def small_ints(shape, seed, hi=4):
    """Integer-valued float32 in [-hi, hi]: sums of their products stay exact in fp32 far below 2^24."""
    return np.random.default_rng(seed).integers(-hi, hi + 1, shape).astype(np.float32)


# The golden scene (tests/golden/pointops_golden.npz): `fine` = seeded SIZES clouds, `coarse` = their furthest samples
# at a quarter of each size ((17, 1, 50, 0, 32, 75): an empty cloud in the middle).  The generator walks seeds from
# GOLDEN_FIRST_SEED until its gap assertions hold and records the seed it kept.
GOLDEN_FIRST_SEED = 0
GOLDEN_CASES = {
    # name: (what, k or nsample, feature width, extra)
    "fps": ("furthestsampling", None, None, None),
    "knn3": ("knnquery fine -> fine", 3, None, None),
    "knn16": ("knnquery coarse -> fine", 16, None, None),
    "knn33": ("knnquery coarse -> fine", 33, None, None),
    "ball": ("ballquery coarse -> fine", 16, None, 0.4),
    "qg_xyz": ("queryandgroup coarse <- fine, use_xyz", 16, 2, True),
    "qg_feat": ("queryandgroup coarse <- fine, features only", 16, 2, False),
    "interp": ("interpolation2 coarse -> fine", 3, 2, None),
    "sub": ("subtraction on the coarse self-graph", 3, 4, None),
    "agg": ("aggregation on the coarse self-graph", 3, 4, 2),
}


def golden_scene(seed):
    """fine xyz (705,3), offset, new_offset (quarter sizes) and the seeded features / loss weights of every case."""
    xyz = seeded_clouds(SIZES, seed)
    n, m = len(xyz), int(sum(quarter(SIZES)))
    r = lambda shape, salt: features(shape, 1000 * (seed + 1) + salt)
    return dict(xyz=xyz, offset=offsets(SIZES), new_offset=offsets(quarter(SIZES)),
                feat=r((n, 2), 1), w_qg_xyz=r((m, 16, 5), 2), w_qg_feat=r((m, 16, 2), 3),
                cfeat=r((m, 2), 4), w_interp=r((n, 2), 5),
                in1=r((m, 4), 6), in2=r((m, 4), 7), w_sub=r((m, 3, 4), 8),
                ainp=r((m, 4), 9), apos=r((m, 3, 4), 10), aw=r((m, 3, 2), 11), w_agg=r((m, 4), 12))


# ------------------------------------------------------------------------------------------- derived error bars
U = 2.0 ** -24                  # unit roundoff of float32
W_ULPS = 16                     # relative error of an interpolation weight in units of U, derived in golden_bounds


def _bar(nterms, roundings, abs_sum):
    """A sequential fp32 sum of `nterms` terms, each the product of `roundings` rounded operations on exact inputs: every
    term carries a relative error of roundings U, and each of the nterms - 1 additions one more U on a partial sum that
    is at most the sum of magnitudes: (nterms + roundings) U sum|term| covers both to first order, with one U to spare for
    the second order."""
    return (np.asarray(nterms, dtype=np.float64) + roundings) * U * abs_sum


def _list_abs(terms, idx, n):
    """Per support row: the length of its list and the sum of |terms| over it."""
    flat = clamp(idx, n).reshape(-1)
    s = np.zeros((n, terms.shape[1]))
    np.add.at(s, flat, np.abs(terms.astype(np.float64)))
    return np.bincount(flat, minlength=n)[:, None], s


def golden_bounds(sc, gold):
    """name -> the bar on |fp32 evaluation - golden| for every value the golden records, from operation counts:
    (terms per sum + roundings per term) x 2^-24 x the sum of the terms' magnitudes (`_bar`).

      knn3_dist    d2 is within TAU = 6 U relative, sqrt halves that and rounds once: TAU dist covers it.
      qg_*         the gathered coordinates take one subtraction (U |value|), gathered features none; the loss is summed
                   in float64 by the tests, so its bar is sum |w| x the element bars (+ 1e-12 relative for that sum).
                   A gradient is the list sum of the loss weights: (list length) U sum|w|; d/d new_xyz sums k of them.
      interp_*     a weight (1 / (dist + 1e-8)) / sum: dist within 4 U, the add and the reciprocal 2 U, the sum of three
                   such terms 2 U more on top of their 6 U, the division 1 U -- 15 U, W_ULPS = 16.  Output: k products
                   of one rounding each, weights off by W_ULPS: (k + 1 + W_ULPS) U sum|input w|; likewise the gradient
                   over a list.
      sub_*        one subtraction per element; grad1 sums k loss weights, grad2 a list of them.
      agg_*        a term (input + position) * weight is two roundings: (k + 2) U sum|term|; grad_position one product;
                   grad_weight c / w_c terms of two roundings; grad_input a list of one-rounding products."""
    xyz, off, noff = sc["xyz"], sc["offset"], sc["new_offset"]
    n, m = len(xyz), int(noff[-1])
    coarse = xyz[gold["fps_idx"].astype(np.int64)]
    f = np.float64
    out = {"knn3_dist": TAU * gold["knn3_dist"]}
    idx16 = gold["knn16_idx"].astype(np.int32)
    gx = grouping_fwd(xyz, idx16, f) - coarse.astype(f)[:, None, :]
    w = sc["w_qg_xyz"].astype(f)
    out["qg_xyz_loss"] = U * np.abs(w[..., :3] * gx).sum() + 1e-12 * np.abs(gold["qg_xyz_loss"])
    out["qg_feat_loss"] = 1e-12 * np.abs(gold["qg_feat_loss"])
    cnt, s = _list_abs(w.reshape(-1, 5), idx16, n)
    out["qg_xyz_gxyz"], out["qg_xyz_gfeat"] = _bar(cnt, 0, s[:, :3]), _bar(cnt, 0, s[:, 3:])
    out["qg_xyz_gnew"] = _bar(16, 0, np.abs(w[..., :3]).sum(1))
    cnt, s = _list_abs(sc["w_qg_feat"].reshape(-1, 2), idx16, n)
    out["qg_feat_gfeat"] = _bar(cnt, 0, s)
    iidx, id2 = knn(3, coarse, xyz, noff, off, f)
    iw = interpolation_weights(id2, f)
    out["interp_out"] = _bar(3, 1 + W_ULPS, np.abs(sc["cfeat"].astype(f)[iidx] * iw[..., None]).sum(1))
    cnt, s = _list_abs(np.repeat(sc["w_interp"].astype(f), 3, axis=0) * iw.reshape(-1, 1), iidx, m)
    out["interp_gfeat"] = _bar(cnt, 1 + W_ULPS, s)
    cidx = gold["cknn3_idx"].astype(np.int32)
    ws = sc["w_sub"].astype(f)
    out["sub_loss"] = U * np.abs(ws * subtraction_fwd(sc["in1"], sc["in2"], cidx, f)).sum() + 1e-12 * np.abs(gold["sub_loss"])
    out["sub_g1"] = _bar(3, 0, np.abs(ws).sum(1))
    cnt, s = _list_abs(ws.reshape(-1, 4), cidx, m)
    out["sub_g2"] = _bar(cnt, 0, s)
    inp, pos, aw, g = (sc[k].astype(f) for k in ("ainp", "apos", "aw", "w_agg"))
    wexp = _wexp(aw, 4, f)
    out["agg_out"] = _bar(3, 2, np.abs((inp[cidx] + pos) * wexp).sum(1))
    out["agg_gpos"] = U * np.abs(g[:, None, :] * wexp)
    out["agg_gw"] = _bar(2, 2, np.abs(g[:, None, :] * (inp[cidx] + pos)).reshape(m, 3, 2, 2).sum(2))
    cnt, s = _list_abs((g[:, None, :] * wexp).reshape(-1, 4), cidx, m)
    out["agg_ginp"] = _bar(cnt, 1, s)
    return out


def golden_eval32(sc, gold):
    """name -> the float32 statements' value of everything `golden_bounds` bars, on the golden's own indices."""
    f = np.float32
    xyz, off, noff = sc["xyz"], sc["offset"], sc["new_offset"]
    n, m = len(xyz), int(noff[-1])
    coarse = xyz[gold["fps_idx"].astype(np.int64)]
    out = {"knn3_dist": np.sqrt(knn(3, xyz, xyz, off, off, f)[1])}
    idx16 = gold["knn16_idx"].astype(np.int32)
    dot = lambda a, b: (a.astype(np.float64) * b.astype(np.float64)).sum()
    gx, gf = grouping_fwd(xyz, idx16, f) - coarse[:, None, :], grouping_fwd(sc["feat"], idx16, f)
    out["qg_xyz_loss"] = dot(np.concatenate((gx, gf), -1), sc["w_qg_xyz"])
    out["qg_feat_loss"] = dot(gf, sc["w_qg_feat"])
    out["qg_xyz_gxyz"] = grouping_bwd(sc["w_qg_xyz"][..., :3], idx16, n, f)
    out["qg_xyz_gfeat"] = grouping_bwd(sc["w_qg_xyz"][..., 3:], idx16, n, f)
    out["qg_xyz_gnew"] = -_seq(sc["w_qg_xyz"][..., :3].astype(f), 1)
    out["qg_feat_gfeat"] = grouping_bwd(sc["w_qg_feat"], idx16, n, f)
    iidx, id2 = knn(3, coarse, xyz, noff, off, f)
    iw = interpolation_weights(id2, f)
    out["interp_out"] = interpolation_fwd(sc["cfeat"], iidx, iw, f)
    out["interp_gfeat"] = interpolation_bwd(sc["w_interp"], iidx, iw, m, f)
    cidx = gold["cknn3_idx"].astype(np.int32)
    out["sub_loss"] = dot(subtraction_fwd(sc["in1"], sc["in2"], cidx, f), sc["w_sub"])
    out["sub_g1"], out["sub_g2"] = subtraction_bwd(sc["w_sub"], cidx, m, f)
    out["agg_out"] = aggregation_fwd(sc["ainp"], sc["apos"], sc["aw"], cidx, f)
    out["agg_ginp"], out["agg_gpos"], out["agg_gw"] = aggregation_bwd(sc["ainp"], sc["apos"], sc["aw"], cidx, sc["w_agg"], f)
    return out
