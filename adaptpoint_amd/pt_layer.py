"""Point Transformer's vector-attention layer, fused (csrc/point_transformer.hip).

    [q | k | v] (n,3C) = x [Wq ; Wk ; Wv]^T + [bq | bk | bv]            one torch matmul (plumbing; `_Project`)
    h (n,k,3) = ReLU(BN3(Linear(3,3)(d)))                              composed, on the stage's shared d (three wide)
    pr = W2 h + b2,  r = k_j - q_i + pr,  y = relu(bn1 r),  t = W3 y + b3,  z = relu(bn2 t),  l = W4 z + b4,
    a = softmax over the k slots,  out_i[c] = sum_s (v_j[c] + pr[c]) a_is[c mod C/8]       the kernels

No (n,k,C) tensor exists in forward: the per-pair tensors are t and a, both (n,k,C/8), and they are what backward
saves.  Backward materialises ONE grouped tensor, dr (n,k,C), between the kernel that makes it per query and the
reverse-list walk that sums it per neighbour; dq | dk | dv land in one (n,3C) tensor for the matmul's backward.

A launch list (training; eval skips rel_stats and the two folds):
    forward   apn_pt_rel_stats + fold -> bn1's scale / shift;  apn_pt_mid + fold -> bn2's;  apn_pt_attend
    backward  apn_pt_attend_bwd + fold -> dW4, db4, bn2's sums;  apn_pt_mid_bwd + fold -> dW3, db3, bn1's sums;
              apn_pt_rel_bwd + fold -> dr, dq, dh, dW2, db2;  apn_pt_scatter_bwd -> dk, dv;
              apn_pt_colsum + fold -> the projection's bias gradient
The BatchNorm algebra between them (mean, variance, scale / shift, the dense term D x + E, dgamma, dbeta, the running
buffers) is torch arithmetic on C-long float64 vectors on the device: no host read, capturable into a graph.  Every
sum has a fixed order: two runs give the same bits.
"""
import torch

from . import _lib, batchnorm
from .fused import _call, _ptr


def _fold(part, rows, width, dev):
    sums = torch.empty(width, dtype=torch.float64, device=dev)
    _call("apn_pt_fold", dev, part.data_ptr(), rows, width, sums.data_ptr())
    return sums


def _bn_forward(bn, sums, count):
    """(scale, shift, mean, rstd) in float64 from the folded {sum x, sum x^2} -- or, in eval mode, from the running
    statistics; in training mode the running buffers are updated as nn.BatchNorm1d does (unbiased variance)."""
    C = bn.num_features
    gamma, beta = bn.weight.detach().double(), bn.bias.detach().double()
    if sums is not None:
        mean = sums[:C] / count
        var = (sums[C:] / count - mean * mean).clamp_min(0.0)
        if batchnorm.mode(bn)[1] and bn.training:
            m = bn.momentum
            bn.running_mean.mul_(1.0 - m).add_((m * mean).to(bn.running_mean.dtype))
            bn.running_var.mul_(1.0 - m).add_((m * var * (count / max(count - 1.0, 1.0))).to(bn.running_var.dtype))
            bn.num_batches_tracked.add_(1)
    else:
        mean, var = bn.running_mean.double(), bn.running_var.double()
    rstd = torch.rsqrt(var + bn.eps)
    scale = gamma * rstd
    return scale, beta - mean * scale, mean, rstd


def _bn_backward(sum_g, sum_gx, scale, mean, rstd, count, training):
    """(dgamma, dbeta, D, E) in float64: dL/dx = scale g + D x + E (D = E = 0 on running statistics)."""
    dbeta = sum_g
    dgamma = rstd * (sum_gx - mean * sum_g)
    if not training:
        return dgamma, dbeta, torch.zeros_like(dgamma), torch.zeros_like(dgamma)
    D = -scale * rstd * dgamma / count
    return dgamma, dbeta, D, -scale * dbeta / count - D * mean


class _Project(torch.autograd.Function):
    """[q | k | v] = x W^T + b with torch's matmuls and the bias gradient as fixed-order column sums (apn_pt_colsum +
    fold): torch's own reduction over the rows holds a memset node once captured at a few thousand rows."""

    @staticmethod
    def forward(ctx, x, W, b):
        ctx.save_for_backward(x, W)
        return torch.addmm(b, x, W.t())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        x, W = ctx.saved_tensors
        g = g.contiguous()
        n, width = g.shape
        rows = _lib.load().apn_pt_colsum_rows(n)
        part = torch.empty(rows, width, dtype=torch.float64, device=g.device)
        _call("apn_pt_colsum", g.device, n, width, g.data_ptr(), width, part.data_ptr())
        return g @ W, g.t() @ x, _fold(part, rows, width, g.device).to(g.dtype)


class _PtAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, h, W2, b2, gamma1, beta1, W3, b3, gamma2, beta2, W4, b4, bn1, bn2, graph):
        dev = qkv.device
        n, C = qkv.shape[0], qkv.shape[1] // 3
        Cp, k = C // 8, graph.idx.shape[1]
        idx = graph.idx
        f32 = dict(dtype=torch.float32, device=dev)
        lib = _lib.load()
        training = batchnorm.mode(bn1)[0]
        with torch.no_grad():
            qkv, h = qkv.contiguous(), h.contiguous()
            wts = torch.cat([W2.reshape(-1), b2, W3.t().reshape(-1), b3, W4.reshape(-1), b4]).float().contiguous()
            bn = torch.empty(2 * C + 2 * Cp, **f32)
            rows = lib.apn_pt_rows(n, k, C)
            count = float(n * k)
            sums1 = sums2 = part2 = None
            if training:
                part1 = torch.empty(rows, 2 * C, dtype=torch.float64, device=dev)
                _call("apn_pt_rel_stats", dev, n, k, C, qkv.data_ptr(), 3 * C, h.data_ptr(), idx.data_ptr(),
                      wts.data_ptr(), part1.data_ptr())
                sums1 = _fold(part1, rows, 2 * C, dev)
                mid_rows = lib.apn_pt_mid_rows(n, k, C)
                part2 = torch.empty(mid_rows, 2 * Cp, dtype=torch.float64, device=dev)
            sc1, sh1, mean1, rstd1 = _bn_forward(bn1, sums1, count)
            bn[:C], bn[C:2 * C] = sc1, sh1
            t = torch.empty(n, k, Cp, **f32)
            _call("apn_pt_mid", dev, n, k, C, qkv.data_ptr(), 3 * C, h.data_ptr(), idx.data_ptr(), wts.data_ptr(),
                  bn.data_ptr(), t.data_ptr(), _ptr(part2))
            if training:
                sums2 = _fold(part2, mid_rows, 2 * Cp, dev)
            sc2, sh2, mean2, rstd2 = _bn_forward(bn2, sums2, count)
            bn[2 * C:2 * C + Cp], bn[2 * C + Cp:] = sc2, sh2
            a = torch.empty(n, k, Cp, **f32)
            out = torch.empty(n, C, **f32)
            _call("apn_pt_attend", dev, n, k, C, qkv.data_ptr(), 3 * C, h.data_ptr(), idx.data_ptr(), wts.data_ptr(),
                  bn.data_ptr(), t.data_ptr(), a.data_ptr(), out.data_ptr())
        ctx.save_for_backward(qkv, h, t, a, wts, bn, sc1, mean1, rstd1, sc2, mean2, rstd2)
        ctx.graph = graph
        ctx.cfg = (n, k, C, rows, count, training, W2.dtype)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, go):
        qkv, h, t, a, wts, bn, sc1, mean1, rstd1, sc2, mean2, rstd2 = ctx.saved_tensors
        n, k, C, rows, count, training, wdtype = ctx.cfg
        Cp = C // 8
        dev = qkv.device
        idx = ctx.graph.idx
        f32 = dict(dtype=torch.float32, device=dev)
        f64 = dict(dtype=torch.float64, device=dev)
        go = go.float().contiguous()
        csr = ctx.graph.csr()
        common = (n, k, C, qkv.data_ptr(), 3 * C, h.data_ptr(), idx.data_ptr(), wts.data_ptr(), bn.data_ptr())

        wa = Cp * Cp + 3 * Cp
        g1 = torch.empty(n, k, Cp, **f32)
        part = torch.empty(rows, wa, **f64)
        _call("apn_pt_attend_bwd", dev, *common, t.data_ptr(), a.data_ptr(), go.data_ptr(), g1.data_ptr(),
              part.data_ptr())
        sa = _fold(part, rows, wa, dev)
        dW4, db4 = sa[:Cp * Cp].view(Cp, Cp), sa[Cp * Cp:Cp * Cp + Cp]
        dgamma2, dbeta2, D2, E2 = _bn_backward(sa[Cp * Cp + Cp:Cp * Cp + 2 * Cp], sa[Cp * Cp + 2 * Cp:], sc2, mean2,
                                               rstd2, count, training)
        de = torch.empty(2 * C + 2 * Cp, **f32)
        de[2 * C:2 * C + Cp], de[2 * C + Cp:] = D2, E2                 # (mid_bwd reads D2, E2 only; D1, E1 follow)
        wm = Cp * C + Cp + 2 * C
        part = torch.empty(rows, wm, **f64)
        _call("apn_pt_mid_bwd", dev, *common, de.data_ptr(), t.data_ptr(), g1.data_ptr(), part.data_ptr())
        sm = _fold(part, rows, wm, dev)
        dW3, db3 = sm[:Cp * C].view(Cp, C), sm[Cp * C:Cp * C + Cp]
        dgamma1, dbeta1, D1, E1 = _bn_backward(sm[Cp * C + Cp:Cp * C + Cp + C], sm[Cp * C + Cp + C:], sc1, mean1, rstd1,
                                               count, training)
        de[:C], de[C:2 * C] = D1, E1

        dr = torch.empty(n, k, C, **f32)
        dh = torch.empty(n, k, 3, **f32)
        dqkv = torch.empty(n, 3 * C, **f32)
        part = torch.empty(rows, 4 * C, **f64)
        _call("apn_pt_rel_bwd", dev, *common, de.data_ptr(), t.data_ptr(), g1.data_ptr(), a.data_ptr(), go.data_ptr(),
              dr.data_ptr(), dh.data_ptr(), dqkv.data_ptr(), 3 * C, part.data_ptr())
        sr = _fold(part, rows, 4 * C, dev)
        dW2, db2 = sr[:3 * C].view(C, 3), sr[3 * C:]
        _call("apn_pt_scatter_bwd", dev, n, k, C, dr.data_ptr(), go.data_ptr(), a.data_ptr(),
              csr.pcnt_poff.data_ptr(), csr.plist.data_ptr(), dqkv.data_ptr(), 3 * C)
        c = lambda v: v.to(wdtype)
        return (dqkv, dh, c(dW2), c(db2), c(dgamma1), c(dbeta1), c(dW3), c(db3), c(dgamma2), c(dbeta2), c(dW4), c(db4),
                None, None, None)


def point_transformer_layer(layer, x, graph):
    """`PointTransformerLayer.forward` on the kernels: x (n,C) float32 CUDA, graph: the level's `StageGraph`."""
    from .point_transformer import _channel_bn
    lq, lk, lv = layer.linear_q, layer.linear_k, layer.linear_v
    qkv = _Project.apply(x, torch.cat([lq.weight, lk.weight, lv.weight], 0), torch.cat([lq.bias, lk.bias, lv.bias], 0))
    lp, lw = layer.linear_p, layer.linear_w
    h = lp[2](_channel_bn(lp[1], lp[0](graph.d)))
    return _PtAttention.apply(qkv, h, lp[3].weight, lp[3].bias, lw[0].weight, lw[0].bias, lw[2].weight, lw[2].bias,
                              lw[3].weight, lw[3].bias, lw[5].weight, lw[5].bias, lw[0], lw[3], graph)
