"""PointNeXt's LocalAggregation with one grouped convolution, fused (csrc/local_aggr.hip).

    out (B,H,N) = [relu](bn(max_K conv(cat[(p[idx] - p) / r, f[idx]]))),   idx (B,N,32): a ball query of p around p
    (openpoints/models/backbone/pointnext.py:27-78 as InvResMLP builds it, :246)

The feature part of the convolution is hoisted to the points as in `adaptpoint_amd.fused_wide` -- U = Wf f (B,N,H),
y[q,k] = U[idx[q,k]] + Wp (p[idx[q,k]] - p[q]) / r, the coordinate columns applied to the relative position as the
composed path forms it -- and because BatchNorm + ReLU is monotone per channel with the sign of gamma, the max over K
commutes with them:

    out[b,c,q] = relu(scale_c ext_k y[q,k][c] + shift_c),   ext = max (gamma_c >= 0) | min

The pass over the B*N*K positions is one gather-extremum over every query's distinct neighbours; no (B,C,N,K) tensor
exists, forward or backward.  A block is

    forward   U = f^T Wf^T                                              the contraction kernel (apn_pw_contract)
              ext, sel, ysum, BatchNorm's partial sums                  apn_la_pool_fwd
              pack = BatchNorm's fold (running buffers updated)         batchnorm.pooled_stats_pack
              out = relu(scale ext + shift), channels first             apn_sa_wide_out
    backward  g' = g [out > 0] scale, {sum g, sum g yhat}               apn_sa_wide_bwd_prep, batchnorm.dense_terms
              dU, dT (, dL/dp) per point through the inverse map        apn_la_pool_bwd   (no float atomics)
              dL/df = Wf^T dU, dL/dW = [dT^T p / r, dU^T f^T]           the contraction kernel

Gradients are bit-identical from run to run.  With sync_bn the float64 sums are all-reduced over ranks where they
leave the kernels (`fused_wide._reduced`'s exchange in the backward pass).
"""
import torch

from . import _lib, batchnorm, fused_wide, pointwise
from . import fused as _fz
from .fused import _call

K_NS = 32
WIDTHS = (64, 128, 256, 512)


def covers(B, N, K, C, w, biased=False, momentum=0.1):
    """Whether the kernels cover a LocalAggregation, on plain values: B clouds of N points, K neighbours, C input
    channels, w the (out, in) channels of its convolution."""
    return (K == K_NS and w[0] in WIDTHS and w[1] == C + 3 and not biased and momentum is not None
            and 0 < B <= 65535 and N > 0 and B * N < 2 ** 24)


class _LocalAggregation(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p, f, w, gamma, beta, mods):
        scale, bn, sync_bn, nbr, relu = mods
        p, f = p.contiguous(), f.contiguous()
        dev = f.device
        B, C, N = f.shape
        H = w.shape[0]
        training = batchnorm.mode(bn)[0]
        sync = sync_bn and (_fz._world(True) > 1 or _fz.FORCE_PHASED)
        f32 = dict(dtype=torch.float32, device=dev)
        lib = _lib.load()
        with torch.no_grad():
            W = w.detach().reshape(H, C + 3).contiguous()
            # the feature columns at the points: U[b] (N x H) = f[b]^T Wf^T, operands read where they lie
            U = torch.empty(B, N, H, **f32)
            pointwise.contract(B, N, H, C, f, C * N, N, False, W[:, 3:], 0, C + 3, True, U, d_batch=N * H, ldd=H)
            ext = torch.empty(B, N, H, **f32)
            sel = torch.empty(B, N, H, dtype=torch.uint8, device=dev)
            count = float(B * N * K_NS)
            rows = lib.apn_la_pool_rows(B, N) if training else 0
            ysum = torch.empty(B, N, H, **f32) if training else None
            part = torch.empty(rows, 2 * H, dtype=torch.float64, device=dev) if training else None
            _call("apn_la_pool_fwd", dev, B, N, H, K_NS, float(scale), U.data_ptr(), p.data_ptr(), W.data_ptr(), C + 3,
                  nbr.idx.data_ptr(), _fz._ptr(gamma), ext.data_ptr(), sel.data_ptr(), _fz._ptr(ysum), _fz._ptr(part))
            pack = batchnorm.pooled_stats_pack(part, rows, H, count, bn, training, sync)
            out = torch.empty(B, H, N, **f32)
            _call("apn_sa_wide_out", dev, B, N, H, ext.data_ptr(), pack.data_ptr(), C, None, None, None,
                  1 if relu else 0, out.data_ptr())
        ctx.save_for_backward(p, f, U, ext, sel, ysum, pack, W, out if relu else None)
        ctx.nbr = nbr
        ctx.cfg = (scale, training, sync, count, gamma is not None, beta is not None, w.shape)
        return out

    @staticmethod
    def backward(ctx, g):
        p, f, U, ext, sel, ysum, pack, W, out_act = ctx.saved_tensors
        nbr = ctx.nbr
        scale, training, sync, count, has_gamma, has_beta, wshape = ctx.cfg
        need_p, need_f = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        need_w = any(ctx.needs_input_grad[2:5])
        dev = U.device
        B, N, H = U.shape
        C = W.shape[1] - 3
        lib = _lib.load()
        if g.dtype != torch.float32:
            g = g.float()
        f32 = dict(dtype=torch.float32, device=dev)
        prow = lib.apn_sa_wide_bwd_prep_rows(B, N)
        gsel = torch.empty(B, N, H, **f32)
        partS = torch.empty(prow, 2 * H, **f32)
        gs = g.stride()
        _call("apn_sa_wide_bwd_prep", dev, B, N, H, g.data_ptr(), gs[0], gs[1], gs[2], ext.data_ptr(), pack.data_ptr(),
              _fz._ptr(out_act), None, gsel.data_ptr(), partS.data_ptr())
        de, g_gamma, g_beta = batchnorm.dense_terms(partS, prow, H, pack, count, training,
                                                    fused_wide._reduced(partS, count) if sync else None)
        dU = torch.empty(B, N, H, **f32)
        dT = torch.empty(B, N, H, **f32)
        g_p = torch.empty(B, N, 3, **f32) if need_p else None
        _call("apn_la_pool_bwd", dev, B, N, H, K_NS, float(scale), gsel.data_ptr(), sel.data_ptr(), nbr.tmap.data_ptr(),
              nbr.pcnt_poff.data_ptr(), nbr.plist.data_ptr(), nbr.geo.data_ptr(), U.data_ptr(), p.data_ptr(),
              _fz._ptr(ysum), de.data_ptr(), W.data_ptr(), C + 3, dU.data_ptr(), dT.data_ptr(), _fz._ptr(g_p))
        g_f = g_w = None
        if need_f:
            # dL/df[b] (C x N) = Wf^T dU[b]^T, channels first without a transposed copy
            g_f = torch.empty(B, C, N, **f32)
            pointwise.contract(B, C, N, H, W[:, 3:], 0, C + 3, False, dU, N * H, H, True, g_f, d_batch=C * N, ldd=N)
        if need_w:
            # dL/dWf = sum_b dU[b]^T f[b]^T, dL/dWp = sum_b dT[b]^T p[b] / r: fixed-order shares
            g_wf = torch.empty(H, C, **f32)
            pointwise.contract(B, H, C, N, dU, N * H, H, False, f, C * N, N, True, g_wf, reduce=True)
            g_wp = torch.empty(H, 3, **f32)
            pointwise.contract(B, H, 3, N, dT, N * H, H, False, p, N * 3, 3, False, g_wp, reduce=True)
            g_w = torch.cat([g_wp * (1.0 / scale), g_wf], 1).view(wshape)
        if not need_w:
            return g_p, g_f, None, None, None, None
        return g_p, g_f, g_w, g_gamma if has_gamma else None, g_beta if has_beta else None, None


def aggregate(p, f, index, scale, conv, bn, relu=True, sync_bn=False):
    """[relu](bn(max_K conv(cat[(p[idx] - p) / scale, f[idx]]))) on the kernels.  index: the `NeighbourIndex` of the
    ball query of p around p (`fused_wide.neighbour_index(idx, p, N)`); scale: the radius when the grouper
    normalises relative positions, else 1."""
    return _LocalAggregation.apply(p, f, conv.weight, bn.weight, bn.bias, (float(scale), bn, sync_bn, index, bool(relu)))
