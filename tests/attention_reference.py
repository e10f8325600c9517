"""Two references for the attention kernels of csrc/attention.hip, in plain torch on any device; no code is shared with
the kernels.

`float64(...)`  softmax(q k^T / 4) v, lse in log2 units, the three gradients -- the arithmetic of oracle.attention /
                oracle.attention_grad (numpy), cloud by cloud so that M = 4096 and B = 32 fit, plus the magnitudes the
                element-wise bars of tests/test_gpu_attention_cases.py are made of.  tests/test_attention_cases_cpu.py
                holds it against the numpy oracle.
`model(...)`    the kernels' INTENDED arithmetic: every operand split into hi + lo bf16 (round to nearest even, the
                remainder formed in float32), a product = lo*hi + hi*lo + hi*hi accumulated in float32, log2(e)/4 folded
                into q, keys in tiles of 32 with the running maximum and sum, P and dS split again, the backward's P
                recomputed from the saved lse, delta = rowsum(dO * O).  Sums inside a product are torch's float32 ones
                (another order than the MFMA's), exp2 / log2 are torch's.
"""
import math

import torch

TILE = 32
LOG2E = 1.4426950408889634
C2 = 3 * 2.0 ** -16          # two bf16 planes: truncation <= 2^-16 of either operand, lo * lo (<= 2^-16) dropped
EPS = 2.0 ** -24


def _heads(t, H):
    B, M, _ = t.shape
    return t.reshape(B, M, H, 16).permute(0, 2, 1, 3)


def _merge(t):
    B, H, M, _ = t.shape
    return t.permute(0, 2, 1, 3).reshape(B, M, H * 16)


# ---- float64 ---------------------------------------------------------------------------------------------------------------

def float64(q, k, v, H, g=None, C2=C2):
    """-> dict: out (B,M,C), lse (B,H,M) in log2 units, with g also dq, dk, dv; and the bars' magnitudes
    delta (B,H,M): max_j [(C2 + 22 eps) |q_i|.|k_j| / 4 + 4 eps |s_ij|]  (nats), lse_nat,
    pv = sum_j p_ij |v_jd|, and the element-wise bars bar_out, bar_lse, bar_dv, bar_dq, bar_dk.  C2: the constant of one
    product -- 3 * 2^-16 for the two-plane MFMA products; the float32 kernel of few points passes its own."""
    B, M, C = q.shape
    res = {n: [] for n in ("out", "lse", "delta", "pv", "dq", "dk", "dv", "bar_out", "bar_lse", "bar_dv", "bar_dq", "bar_dk")}
    tail = (M / 32 + 40) * EPS
    for b in range(B):
        qh, kh, vh = (_heads(t[b:b + 1].double(), H)[0] for t in (q, k, v))               # (H, M, 16)
        s = qh @ kh.transpose(1, 2) / 4.0
        lse = torch.logsumexp(s, dim=-1)
        p = torch.exp(s - lse.unsqueeze(-1))
        out = p @ vh
        # score error in nats: both operands split (C2) and 16 products + the log2(e)/4 fold + the roundings of the
        # sum (22 eps) against |q|.|k| / 4; the subtraction of the maximum and the exp2 argument against |s| (4 eps)
        delta = ((C2 + 22 * EPS) * (qh.abs() @ kh.abs().transpose(1, 2)) / 4.0 + 4 * EPS * s.abs()).amax(-1)
        w = torch.expm1(2 * delta) + C2 + tail                                           # relative bar of sum_j p_ij x_j
        pv = p @ vh.abs()
        res["out"].append(out), res["lse"].append(lse / math.log(2.0)), res["delta"].append(delta), res["pv"].append(pv)
        res["bar_out"].append(w.unsqueeze(-1) * pv)
        res["bar_lse"].append((delta + 4 * EPS * (1 + lse.abs())) / math.log(2.0))
        if g is not None:
            gh = _heads(g[b:b + 1].double(), H)[0]
            dp = gh @ vh.transpose(1, 2)
            Dl = (gh * out).sum(-1, keepdim=True)
            ds = p * (dp - Dl)
            res["dv"].append(p.transpose(1, 2) @ gh)
            res["dq"].append(ds @ kh / 4.0)
            res["dk"].append(ds.transpose(1, 2) @ qh / 4.0)
            res["bar_dv"].append((p * w.unsqueeze(-1)).transpose(1, 2) @ gh.abs())
            # The bar on dS_ij = p_ij (dP_ij - D_i), term by term (each from the arithmetic of attn_bwd_kv / attn_bwd_q):
            #   2 delta_i |dP_ij - D_i|   P is recomputed as exp2(s' - lse'): s' and lse' are each within delta_i (nats)
            #                             of the true score / log-sum-exp, so P' = P (1 +- 2 delta_i) to first order;
            #   C2 |dO_i|.|v_j|           dP = dO . v is a two-plane product: 16 bits of either operand, lo * lo dropped;
            #   errD_i                    D_i = rowsum(dO * O) inherits the forward's bar on O: sum_d |dO_id| bar_out_id;
            # all three times p_ij.  Then the last product, dQ = dS' K / 4 (dK = dS'^T Q / 4), is two-plane again:
            #   C2 sum_j |dS_ij| |k_jd| / 4
            # on top of the error of dS carried through |k| / 4 (|q| / 4).
            errD = (gh.abs() * res["bar_out"][-1]).sum(-1, keepdim=True)
            eds = p * (2 * delta.unsqueeze(-1) * (dp - Dl).abs() + C2 * (gh.abs() @ vh.abs().transpose(1, 2)) + errD)
            res["bar_dq"].append((eds + C2 * ds.abs()) @ kh.abs() / 4.0)
            res["bar_dk"].append((eds + C2 * ds.abs()).transpose(1, 2) @ qh.abs() / 4.0)
    done = {}
    for n, parts in res.items():
        if not parts:
            continue
        t = torch.stack(parts)                                                           # (B, H, M[, 16])
        done[n] = _merge(t) if t.dim() == 4 else t
    return done


# ---- the model of the kernels' arithmetic -----------------------------------------------------------------------------------

def split(x):
    hi = x.to(torch.bfloat16).float()
    return hi, (x - hi).to(torch.bfloat16).float()


def prod3(a, b):
    """a = (hi, lo) (..., R, K), b = (hi, lo) (..., Q, K) -> a b^T (..., R, Q): small terms first, hi * hi last."""
    bt = [t.transpose(-1, -2) for t in b]
    return (a[1] @ bt[0] + a[0] @ bt[1]) + a[0] @ bt[0]


def model(q, k, v, H, g=None):
    """-> dict out, lse (log2 units) [, dq, dk, dv], float32."""
    f32 = torch.float32
    res = {n: [] for n in ("out", "lse", "dq", "dk", "dv")}
    scale = torch.tensor(0.25, dtype=f32) * torch.tensor(LOG2E, dtype=f32)               # 0.25f * AT_LOG2E, in float32
    B, M, C = q.shape
    for b in range(B):
        qh, kh, vh = (_heads(t[b:b + 1].float(), H)[0] for t in (q, k, v))               # (H, M, 16)
        Qs, Ks, Vs = split(qh * scale.to(q.device)), split(kh), split(vh)
        mx = torch.full((H, M), -math.inf, dtype=f32, device=q.device)
        lsum = torch.zeros(H, M, dtype=f32, device=q.device)
        o = torch.zeros(H, M, 16, dtype=f32, device=q.device)
        for t0 in range(0, M, TILE):
            kt = tuple(x[:, t0:t0 + TILE] for x in Ks)
            vt = tuple(x[:, t0:t0 + TILE].transpose(1, 2) for x in Vs)                    # (H, 16, 32)
            s = prod3(Qs, kt)                                                            # (H, M, 32), log2 units
            mnew = torch.maximum(mx, s.amax(-1))
            alpha = torch.exp2(mx - mnew)
            p = torch.exp2(s - mnew.unsqueeze(-1))
            lsum = lsum * alpha + p.sum(-1)
            o = o * alpha.unsqueeze(-1) + prod3(split(p), vt)
            mx = mnew
        out = o * (1.0 / lsum).unsqueeze(-1)
        lse = mx + torch.log2(lsum)
        res["out"].append(out), res["lse"].append(lse)
        if g is None:
            continue
        gh = _heads(g[b:b + 1].float(), H)[0]
        Gs = split(gh)
        Dl = (gh * out).sum(-1)
        p = torch.exp2(prod3(Qs, Ks) - lse.unsqueeze(-1))                                 # (H, M, M): queries x keys
        ds = p * (prod3(Gs, Vs) - Dl.unsqueeze(-1))
        Pt, St = (tuple(x.transpose(1, 2) for x in split(y)) for y in (p, ds))
        gt, qt, k4 = (tuple(x.transpose(1, 2) for x in y) for y in (Gs, split(qh * 0.25), split(kh * 0.25)))
        res["dv"].append(prod3(Pt, gt))
        res["dk"].append(prod3(St, qt))
        res["dq"].append(prod3(split(ds), k4))
    done = {}
    for n, parts in res.items():
        if parts:
            t = torch.stack(parts)
            done[n] = _merge(t) if t.dim() == 4 else t
    return done


# ---- the operand images (apn_attention_prep / the image kernel of the backward) ----------------------------------------------

def acc_row(reg, h):
    return (reg & 3) + 8 * (reg >> 2) + 4 * h


def tile_permutation():
    """position p = 16 s + 8 h + j of a 32-tile holds the point acc_row(8 s + j, h) of the tile (the MFMA accumulator's
    row order: adaptpoint_amd/csrc/apn_mfma.h)."""
    return [acc_row(8 * (p >> 4) + (p & 7), (p >> 3) & 1) for p in range(32)]


def rows_image(img, B, H, M):
    """(B*H*M*32,) bf16 -> hi, lo (B, H, M, 16) float32"""
    t = img.view(B, H, M, 2, 16).float()
    return t[:, :, :, 0], t[:, :, :, 1]


def trans_image(img, B, H, M):
    """(B*H*M*32,) bf16, (B, H, [hi|lo], 16, M) with every 32-tile permuted -> hi, lo (B, H, M, 16) float32 in point order"""
    t = img.view(B, H, 2, 16, M // 32, 32).float()
    perm = torch.tensor(tile_permutation(), device=img.device)
    un = torch.empty_like(t)
    un[..., perm] = t                                            # position p holds point perm[p]
    un = un.reshape(B, H, 2, 16, M).permute(0, 1, 2, 4, 3)
    return un[:, :, 0], un[:, :, 1]
