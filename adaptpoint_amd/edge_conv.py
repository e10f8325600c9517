"""DGCNN's EdgeConv block, fused (csrc/edge_conv.hip).

    out (B,H,N) = act(bn(max_k W [x_i ; x_j(i,k) - x_i])),   W = [Wa | Wb] (H x 2C), act = LeakyReLU(slope)
    (openpoints/models/layers/graph_conv.py:38-51 over create_convblock2d)

The convolution is linear in [x_i ; x_j - x_i], so it is hoisted to the points -- u = (Wa - Wb) x, v = Wb x, one
contraction with the stacked weight [Wa - Wb ; Wb] -- and y[i,k] = u_i + v_j(i,k).  BatchNorm + LeakyReLU is monotone
per channel with the sign of gamma, so the max over K commutes with them, exactly as in `adaptpoint_amd.local_aggr`:

    out[b,c,i] = act(scale_c ext_k y[i,k][c] + shift_c),   ext = max (gamma_c >= 0) | min

Neither the (B,2C,N,K) nor the (B,H,N,K) tensor of the composed path exists, forward or backward.  A block is

    index     the reverse-neighbour lists of idx (a function of idx alone, built once per graph)   apn_ec_csr
    forward   [u | v] = x^T [Wa - Wb ; Wb]^T                              the contraction kernel (apn_pw_contract)
              ext, sel, ysum, BatchNorm's partial sums                    apn_ec_pool_fwd
              pack = BatchNorm's fold (running buffers updated)           batchnorm.pooled_stats_pack
              out = act(scale ext + shift) [+ residual], channels first   apn_ec_out_res
    backward  gsel = g act' scale, {sum g act', sum g act' yhat}          apn_ec_bwd_prep_act, batchnorm.dense_terms
              [du | dv] per point through the reverse lists               apn_ec_pool_bwd   (no float atomics)
              dL/dx = [Wa - Wb ; Wb]^T [du | dv]^T, dL/dW from [du | dv]^T x^T    the contraction kernel

DeepGCN's blocks (adaptpoint_amd.deepgcn) use ReLU and a residual: `edge_conv(..., slope=0, residual=x)` adds it in the
output kernel (the block's `body(x) + x` without another pass); ReLU is still non-decreasing, so the max over K
commutes with it as above.  Every block goes through these two entries, DGCNN's (slope > 0, no residual) included; the
C interface keeps apn_ec_out and apn_ec_bwd_prep, the same launches behind a slope > 0 guard.

Gradients are bit-identical from run to run.  The data-parallel BatchNorm exchange is not built here: with sync_bn at
world size > 1 `dgcnn.EdgeConv` raises instead of normalising rank-locally.
"""
from typing import NamedTuple

import torch

from . import _lib, batchnorm, pointwise
from . import fused as _fz
from .fused import _call

WIDTHS = (64, 128, 256, 512)
K_MAX = 64
C_IN = (3, 4, 64, 128, 256)


def covers(B, N, K, C, H, biased=False, momentum=0.1):
    """Whether the kernels cover an EdgeConv block, on plain values: B clouds of N points, K neighbours, C input
    channels (the convolution reads 2C), H output channels, whether the convolution has a bias, BatchNorm's momentum."""
    return (H in WIDTHS and C in C_IN and 1 <= K <= K_MAX and not biased and momentum is not None
            and 0 < B <= 65535 and N > 0 and B * N < 2 ** 24)


class EdgeIndex(NamedTuple):
    """A neighbour graph and its reverse lists: what the backward pass walks."""
    idx: torch.Tensor          # (B,N,K) int32
    pcnt_poff: torch.Tensor    # (2,B*N) int32: how many positions gather each point, where its list starts
    plist: torch.Tensor        # (B*N*K,) int32: positions (b N + i) K + slot, ascending per list


@torch.no_grad()
def edge_index(idx):
    """The `EdgeIndex` of idx (B,N,K): part of the index step -- a function of idx alone, no gradient, built once
    per graph however many backward passes use it."""
    idx = idx.int().contiguous()
    if not idx.is_cuda:
        raise RuntimeError("adaptpoint_amd.edge_conv needs CUDA/HIP tensors: the product path has no CPU fallback")
    B, N, K = idx.shape
    i32 = dict(dtype=torch.int32, device=idx.device)
    pcnt_poff = torch.empty(2, B * N, **i32)
    plist = torch.empty(B * N * K, **i32)
    scratch = torch.empty(B * N * (K + 1), **i32)
    _call("apn_ec_csr", idx.device, B, N, K, idx.data_ptr(), pcnt_poff.data_ptr(), plist.data_ptr(), scratch.data_ptr())
    return EdgeIndex(idx, pcnt_poff, plist)


class _Block(NamedTuple):
    """What `_EdgeConv` needs beside its tensors."""
    bn: torch.nn.Module        # the BatchNorm2d (its running buffers are updated)
    slope: float               # LeakyReLU's, 0 for ReLU
    graph: EdgeIndex
    res_is_x: bool             # the residual is the block's own input (C == H): `res` is None, dL/dx takes g


class _EdgeConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, gamma, beta, res, blk):
        bn, slope, graph, res_is_x = blk
        x = x.contiguous()
        dev = x.device
        B, C, N = x.shape
        H = w.shape[0]
        K = graph.idx.shape[2]
        training = batchnorm.mode(bn)[0]
        f32 = dict(dtype=torch.float32, device=dev)
        lib = _lib.load()
        with torch.no_grad():
            W = w.detach().reshape(H, 2 * C)
            Wc = torch.cat([W[:, :C] - W[:, C:], W[:, C:]], 0).contiguous()           # (2H, C): [Wa - Wb ; Wb]
            # the convolution at the points: UV[b] (N x 2H) = x[b]^T Wc^T, operands read where they lie
            UV = torch.empty(B, N, 2 * H, **f32)
            pointwise.contract(B, N, 2 * H, C, x, C * N, N, False, Wc, 0, C, True, UV, d_batch=N * 2 * H, ldd=2 * H)
            ext = torch.empty(B, N, H, **f32)
            sel = torch.empty(B, N, H, dtype=torch.uint8, device=dev)
            count = float(B * N * K)
            rows = lib.apn_ec_pool_rows(B, N) if training else 0
            ysum = torch.empty(B, N, H, **f32) if training else None
            part = torch.empty(rows, 2 * H, dtype=torch.float64, device=dev) if training else None
            _call("apn_ec_pool_fwd", dev, B, N, H, K, UV.data_ptr(), 2 * H, graph.idx.data_ptr(), _fz._ptr(gamma),
                  ext.data_ptr(), sel.data_ptr(), _fz._ptr(ysum), _fz._ptr(part))
            pack = batchnorm.pooled_stats_pack(part, rows, H, count, bn, training, sync=False)
            out = torch.empty(B, H, N, **f32)
            r = x if res_is_x else res
            if r is not None and (r.shape != out.shape or r.dtype != torch.float32 or r.device != dev):
                raise RuntimeError(f"edge_conv: residual {tuple(r.shape)} {r.dtype} does not match the output "
                                   f"{tuple(out.shape)} float32")
            rs = r.stride() if r is not None else (0, 0, 0)
            _call("apn_ec_out_res", dev, B, N, H, ext.data_ptr(), pack.data_ptr(), slope, _fz._ptr(r), rs[0], rs[1],
                  rs[2], out.data_ptr())
        ctx.save_for_backward(x, UV, ext, sel, ysum, pack, Wc)
        ctx.graph = graph
        ctx.cfg = (slope, training, count, gamma is not None, beta is not None, w.shape)
        ctx.res_is_x = res_is_x
        return out

    @staticmethod
    def backward(ctx, g):
        x, UV, ext, sel, ysum, pack, Wc = ctx.saved_tensors
        graph = ctx.graph
        slope, training, count, has_gamma, has_beta, wshape = ctx.cfg
        need_x, need_w, need_res = ctx.needs_input_grad[0], any(ctx.needs_input_grad[1:4]), ctx.needs_input_grad[4]
        dev = x.device
        B, C, N = x.shape
        H = ext.shape[2]
        K = graph.idx.shape[2]
        lib = _lib.load()
        if g.dtype != torch.float32:
            g = g.float()
        f32 = dict(dtype=torch.float32, device=dev)
        prow = lib.apn_ec_bwd_prep_rows(B, N)
        gsel = torch.empty(B, N, H, **f32)
        partS = torch.empty(prow, 2 * H, **f32)
        gs = g.stride()
        _call("apn_ec_bwd_prep_act", dev, B, N, H, g.data_ptr(), gs[0], gs[1], gs[2], ext.data_ptr(), pack.data_ptr(),
              slope, gsel.data_ptr(), partS.data_ptr())
        de, g_gamma, g_beta = batchnorm.dense_terms(partS, prow, H, pack, count, training)
        g_x = g_w = None
        if need_x or need_w:
            dUV = torch.empty(B, N, 2 * H, **f32)
            _call("apn_ec_pool_bwd", dev, B, N, H, K, gsel.data_ptr(), sel.data_ptr(), graph.pcnt_poff.data_ptr(),
                  graph.plist.data_ptr(), UV.data_ptr(), 2 * H, _fz._ptr(ysum), de.data_ptr(), dUV.data_ptr())
        if need_x:
            # dL/dx[b] (C x N) = Wc^T dUV[b]^T, channels first without a transposed copy
            g_x = torch.empty(B, C, N, **f32)
            pointwise.contract(B, C, N, 2 * H, Wc, 0, C, False, dUV, N * 2 * H, 2 * H, True, g_x, d_batch=C * N, ldd=N)
            if ctx.res_is_x:
                g_x += g                                     # the residual's gradient is g itself
        if need_w:
            # dL/dWc = sum_b dUV[b]^T x[b]^T in fixed-order shares; dWa = its u rows, dWb = its v rows minus them
            g_wc = torch.empty(2 * H, C, **f32)
            pointwise.contract(B, 2 * H, C, N, dUV, N * 2 * H, 2 * H, False, x, C * N, N, True, g_wc, reduce=True)
            g_w = torch.cat([g_wc[:H], g_wc[H:] - g_wc[:H]], 1).view(wshape)
        g_res = g if need_res else None                      # (needs_input_grad is False for res = None)
        if not need_w:
            return g_x, None, None, None, g_res, None
        return g_x, g_w, g_gamma if has_gamma else None, g_beta if has_beta else None, g_res, None


def edge_conv(x, graph, conv, bn, slope, residual=None):
    """act(bn(max_k conv([x_i ; x_j - x_i]))) [+ residual] on the kernels.  x (B,C,N); graph: the `EdgeIndex` of the
    neighbours (`edge_index(idx)`); conv: the bias-free Conv2d(2C, H, 1); bn: its BatchNorm2d; slope: LeakyReLU's, 0 for
    ReLU; residual (B,H,N), any strides: added behind the activation in the output kernel (`residual is x`, a
    ResDynBlock: its gradient joins dL/dx with one add)."""
    if not slope >= 0:
        raise ValueError(f"edge_conv: slope {slope} (the max over K commutes with a non-decreasing activation only)")
    res_is_x = residual is x
    return _EdgeConv.apply(x, conv.weight, bn.weight, bn.bias, None if res_is_x else residual,
                           _Block(bn, float(slope), graph, res_is_x))
