"""Two references for the head-dim-64 kernels of csrc/token_attention.hip, in plain torch on any device; no code is shared
with the kernels.  The counterpart of tests/attention_reference.py on the packed qkv (B, T, [3][H][64]).

`float64(...)`  softmax(q k^T / 8) v, lse in log2 units, the packed gradient, cloud by cloud, plus the magnitudes the
                element-wise bars of tests/test_gpu_token_attention.py are made of.
`model(...)`    the kernels' INTENDED arithmetic: every operand split into hi + lo bf16, a product = lo*hi + hi*lo + hi*hi
                accumulated in float32, the finished score times 0.125 * log2e_f32 (one rounding; 0.125 is exact), keys in
                tiles of 32 -- the last one as short as it is: the model has no pads -- with the running maximum and sum,
                P and dS split again, the backward's P recomputed from the saved lse, delta = rowsum(dO * O), dQ and dK
                scaled by 0.125 at the end.  Sums inside a product are torch's float32 ones (another order than the
                MFMA's), exp2 / log2 are torch's.

The constants of the bars, derived from that arithmetic (C2 as in attention_reference: two planes per operand):
  a score   64 products of split operands (C2 each, relative to |q_d k_d|), summed in float32 in some order (at most
            64 + 3 additions: 64 terms, three planes chained) and scaled once (1 rounding):  (C2 + 70 eps) |q|.|k| / 8,
            then the subtraction of the maximum and the exp2 argument against |s|: 4 eps |s|.
  sum_j p x 32 keys per tile and T / 32 rescaled tiles, the division / the lse's log2, the split of P:  C2 + (T/32 + 40) eps
            on top of the scores' exp(2 delta) - 1.
  dP        64 products again: (C2 + 70 eps) |dO|.|v|.
  dQ, dK    the last product is two-plane with a float32 sum over T terms: (C2 + (T/32 + 40) eps) sum |dS| |k| / 8.
"""
import math

import torch

from attention_reference import C2, EPS, split, prod3

D = 64
TILE = 32
LOG2E_F32 = float(torch.tensor(1.4426950408889634, dtype=torch.float32))
SUM64 = 70 * EPS


def _heads(t, H):
    B, T, _ = t.shape
    return t.reshape(B, T, H, D).permute(0, 2, 1, 3)


def _merge(t):
    B, H, T, _ = t.shape
    return t.permute(0, 2, 1, 3).reshape(B, T, H * D)


def _finish(res):
    done = {}
    for n, parts in res.items():
        if parts:
            t = torch.stack(parts)
            done[n] = _merge(t) if t.dim() == 4 else t
    for pre in ("", "bar_"):
        if pre + "dq" in done:
            done[pre + "dqkv"] = torch.cat([done.pop(pre + "dq"), done.pop(pre + "dk"), done.pop(pre + "dv")], dim=-1)
    return done


def float64(qkv, H, g=None):
    """-> dict: out (B,T,C), lse (B,H,T) in log2 units, with g also dqkv (B,T,3C); bar_out, bar_lse, bar_dqkv."""
    B, T, _ = qkv.shape
    names = ("out", "lse", "dq", "dk", "dv", "bar_out", "bar_lse", "bar_dq", "bar_dk", "bar_dv")
    res = {n: [] for n in names}
    tail = (T / 32 + 40) * EPS
    for b in range(B):
        qh, kh, vh = (_heads(t.double(), H)[0] for t in qkv[b:b + 1].chunk(3, dim=-1))      # (H, T, 64)
        s = qh @ kh.transpose(1, 2) / 8.0
        lse = torch.logsumexp(s, dim=-1)
        p = torch.exp(s - lse.unsqueeze(-1))
        out = p @ vh
        delta = ((C2 + SUM64) * (qh.abs() @ kh.abs().transpose(1, 2)) / 8.0 + 4 * EPS * s.abs()).amax(-1)
        w = torch.expm1(2 * delta) + C2 + tail
        res["out"].append(out), res["lse"].append(lse / math.log(2.0))
        res["bar_out"].append(w.unsqueeze(-1) * (p @ vh.abs()))
        res["bar_lse"].append((delta + 4 * EPS * (1 + lse.abs())) / math.log(2.0))
        if g is not None:
            gh = _heads(g[b:b + 1].double(), H)[0]
            dp = gh @ vh.transpose(1, 2)
            Dl = (gh * out).sum(-1, keepdim=True)
            ds = p * (dp - Dl)
            res["dv"].append(p.transpose(1, 2) @ gh)
            res["dq"].append(ds @ kh / 8.0)
            res["dk"].append(ds.transpose(1, 2) @ qh / 8.0)
            res["bar_dv"].append((p * w.unsqueeze(-1)).transpose(1, 2) @ gh.abs())
            # dS_ij = p_ij (dP_ij - D_i): P' = P (1 +- 2 delta_i) (score and lse each within delta_i); dP a 64-product
            # two-plane sum; D_i = rowsum(dO * O) inherits the forward's bar on O (and its own 64-term float32 sum)
            errD = (gh.abs() * res["bar_out"][-1]).sum(-1, keepdim=True) + SUM64 * (gh.abs() * out.abs()).sum(-1, keepdim=True)
            eds = p * (2 * delta.unsqueeze(-1) * (dp - Dl).abs() + (C2 + SUM64) * (gh.abs() @ vh.abs().transpose(1, 2)) + errD)
            last = eds + (C2 + tail) * ds.abs()
            res["bar_dq"].append(last @ kh.abs() / 8.0)
            res["bar_dk"].append(last.transpose(1, 2) @ qh.abs() / 8.0)
    return _finish(res)


def model(qkv, H, g=None, pad_keys=0):
    """-> dict out, lse (log2 units) [, dqkv], float32.  pad_keys > 0 appends that many ZERO keys / values to every
    (cloud, head) WITHOUT masking them -- what a kernel that relied on 'a pad scores low' would compute (forward only)."""
    f32 = torch.float32
    res = {n: [] for n in ("out", "lse", "dq", "dk", "dv")}
    B, T, _ = qkv.shape
    sc = torch.tensor(0.125 * LOG2E_F32, dtype=f32, device=qkv.device)
    for b in range(B):
        qh, kh, vh = (_heads(t.float(), H)[0] for t in qkv[b:b + 1].chunk(3, dim=-1))       # (H, T, 64)
        if pad_keys:
            kh, vh = (torch.cat([t, t.new_zeros(H, pad_keys, D)], dim=1) for t in (kh, vh))
        Qs, Ks, Vs = split(qh), split(kh), split(vh)
        mx = torch.full((H, T), -math.inf, dtype=f32, device=qkv.device)
        lsum = torch.zeros(H, T, dtype=f32, device=qkv.device)
        o = torch.zeros(H, T, D, dtype=f32, device=qkv.device)
        for t0 in range(0, kh.shape[1], TILE):
            kt = tuple(x[:, t0:t0 + TILE] for x in Ks)
            vt = tuple(x[:, t0:t0 + TILE].transpose(1, 2) for x in Vs)
            s = prod3(Qs, kt) * sc
            mnew = torch.maximum(mx, s.amax(-1))
            alpha = torch.exp2(mx - mnew)
            p = torch.exp2(s - mnew.unsqueeze(-1))
            lsum = lsum * alpha + p.sum(-1)
            o = o * alpha.unsqueeze(-1) + prod3(split(p), vt)
            mx = mnew
        out = o * (1.0 / lsum).unsqueeze(-1)
        lse = mx + torch.log2(lsum)
        res["out"].append(out), res["lse"].append(lse)
        if g is None or pad_keys:
            continue
        gh = _heads(g[b:b + 1].float(), H)[0]
        Gs = split(gh)
        Dl = (gh * out).sum(-1)
        p = torch.exp2(prod3(Qs, Ks) * sc - lse.unsqueeze(-1))                               # (H, T, T): queries x keys
        ds = p * (prod3(Gs, Vs) - Dl.unsqueeze(-1))
        tr = lambda pair: tuple(x.transpose(1, 2) for x in pair)
        res["dv"].append(prod3(tr(split(p)), tr(Gs)))
        res["dk"].append(prod3(tr(split(ds)), tr(Qs)) * 0.125)
        res["dq"].append(prod3(split(ds), tr(Ks)) * 0.125)
    return _finish(res)


def planes(x):
    """How many bf16 planes the float32 tensor x needs to be represented exactly: 1, 2, or 3 (= more than two)."""
    hi, lo = split(x)
    if bool((hi == x).all()):
        return 1
    return 2 if bool((hi + lo == x).all()) else 3
