"""PointMLP's geometric-affine grouping stage with its first convolution hoisted to the points (csrc/affine_group.hip).

`LocalGrouper(normalize="anchor", use_xyz=False)` followed by `PreExtraction.transfer`'s bias-free convolution
(openpoints/models/backbone/pointmlp.py:150-263) is, per cloud, with j = idx[s,k] and a = fps_idx[s],

    d[s,k,:] = x[j,:] - x[a,:]                      sigma = unbiased std of all S K C entries of d,  r = 1 / (sigma + 1e-5)
    y[s,k,:] = W [alpha d r + beta ; x[a,:]]        W = [W1 | W2]

y is linear in the grouped tensor, so with Wa = W1 alpha (columns scaled), [P | Q] = x [Wa ; W2]^T over the N points
(one contraction, `pointwise.contract`: S K / N times fewer multiply-adds) and c0 = W1 beta

    y[s,k,:] = r (P[j,:] - P[a,:]) + Q[a,:] + c0

Neither the grouped (B,S,K,C) tensor, nor its difference, its normalised and affine copies, the repeated anchor, the
(B,S,K,2C) concatenation or its permuted copy exist.  A call is

    index     fps_idx, new_xyz, idx and the reverse lists of idx and of fps_idx      FPS, apn_knn_query, apn_po_csr (x2)
    forward   {sum d, sum d^2} per cloud, float64                                     apn_ag_moments, apn_ag_fold
              r from the moments                                                      a few torch operations on (B,2)
              [P | Q]                                                                 apn_pw_contract
              y (B,O,S K) + BatchNorm's partial rows                                  apn_ag_combine_fwd
    backward  dL/dy as rows                                                           apn_pw_transpose
              [dP | dQ] per point, shares of dr and dc0                               apn_ag_combine_bwd, apn_ag_fold (x2)
              the gradient through sigma                                              apn_ag_sigma_bwd
              dL/dx += [dP | dQ] [Wa ; W2],  d[Wa ; W2] = sum [dP | dQ]^T x           apn_pw_contract (x2)

The chain from Wa and c0 to W, alpha and beta is three small elementwise products and two column sums in the backward
pass.  `affine_group_bn_act` adds the layer's BatchNorm (+ ReLU): `batchnorm.bn_act` on the partial rows in training mode, the
combine launch's own eval form (running statistics, one launch, no y) otherwise.  Also here: `bn_act` and `res_relu_max` (the tail of a PreExtraction: add + ReLU + max over K).
Gradients are bit-identical from run to run: no float atomics anywhere.  There is no CPU fallback.
"""
from typing import NamedTuple, Optional

import torch

from . import _lib, batchnorm
from .fused import _call, _ptr

K_MAX = 64


def covers(B, N, S, K, C, O, groups=1, bias=False, use_xyz=False, normalize="anchor", activation="relu"):
    """Whether the kernels cover a LocalGrouper + PreExtraction stage, on plain values: B clouds of N points, S queries
    of K neighbours, C input channels, O output channels, and the block's configuration."""
    return (groups == 1 and not bias and not use_xyz and normalize == "anchor" and str(activation).lower() == "relu"
            and 1 <= K <= K_MAX and K <= N and S >= 1 and C >= 1 and O >= 1 and S * K * C >= 2
            and 0 < B <= 65535 and B * N < 2 ** 24 and B * S < 2 ** 24 and S * K < 2 ** 24)


class GroupIndex(NamedTuple):
    """A stage's sample and neighbour graph with their reverse lists: a function of the coordinates alone."""
    fps_idx: torch.Tensor                 # (B,S) int32
    new_xyz: torch.Tensor                 # (B,S,3)
    idx: torch.Tensor                     # (B,S,K) int32
    nbr_cnt_off: Optional[torch.Tensor]   # (2,B*N) int32: how many positions gather each point, where its list starts
    nbr_list: Optional[torch.Tensor]      # (B*S*K,) int32: flat positions (b S + s) K + k, ascending per list
    anc_cnt_off: Optional[torch.Tensor]   # (2,B*N) int32: the same for the anchors
    anc_list: Optional[torch.Tensor]      # (B*S,) int32: flat queries b S + s


def _flat_csr(idx2d, n_rows):
    m, k = idx2d.shape
    dev = idx2d.device
    cnt_off = torch.empty(2, n_rows, dtype=torch.int32, device=dev)
    plist = torch.empty(m * k, dtype=torch.int32, device=dev)
    scratch = torch.empty(n_rows + m * k, dtype=torch.int32, device=dev)
    _call("apn_po_csr", dev, n_rows, m, k, idx2d.data_ptr(), cnt_off.data_ptr(), plist.data_ptr(), scratch.data_ptr())
    return cnt_off, plist


@torch.no_grad()
def group_index(fps_idx, new_xyz, idx, n_points):
    """The `GroupIndex` of a sample fps_idx (B,S) and its neighbours idx (B,S,K) among n_points points per cloud.  On
    the GPU with the reverse lists (apn_po_csr on flat rows, indices clamped into their cloud first, as every kernel
    clamps them); CPU tensors give the bare indices (the composed path needs no lists)."""
    fps_idx = fps_idx.int().contiguous()
    idx = idx.int().contiguous()
    if not idx.is_cuda:
        return GroupIndex(fps_idx, new_xyz, idx, None, None, None, None)
    B, S, K = idx.shape
    base = (torch.arange(B, dtype=torch.int32, device=idx.device) * n_points).view(B, 1, 1)
    flat_i = (idx.clamp(0, n_points - 1) + base).view(B * S, K).contiguous()
    flat_a = (fps_idx.clamp(0, n_points - 1) + base.view(B, 1)).view(B * S, 1).contiguous()
    nbr = _flat_csr(flat_i, B * n_points)
    anc = _flat_csr(flat_a, B * n_points)
    return GroupIndex(fps_idx, new_xyz, idx, nbr[0], nbr[1], anc[0], anc[1])


def _fold(part, rows, ncol):
    out = torch.empty(ncol, dtype=torch.float64, device=part.device)
    _call("apn_ag_fold", part.device, rows, ncol, part.data_ptr(), out.data_ptr())
    return out


def moments(x, graph):
    """(B,2) float64 {sum d, sum d^2} of d = x[idx] - x[fps_idx] over each cloud's S K C entries."""
    B, N, C = x.shape
    S, K = graph.idx.shape[1:]
    rows = _lib.load().apn_ag_moment_rows(S)
    part = torch.empty(rows, B, 2, dtype=torch.float64, device=x.device)
    _call("apn_ag_moments", x.device, B, N, S, K, C, x.data_ptr(), graph.idx.data_ptr(), graph.fps_idx.data_ptr(),
          part.data_ptr())
    return _fold(part, rows, 2 * B).view(B, 2)


class _AffineGroupLinear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, alpha, beta, graph, bn=None, relu=False, gamma=None, bias=None):
        """bn None: -> (y, BatchNorm's partial rows).  bn given (a BatchNorm in eval mode; gamma, bias its parameters):
        -> ([relu](bn(y)), stat) from the running statistics in the combine launch itself."""
        from .pointwise import contract
        x = x.contiguous()
        dev = x.device
        B, N, C = x.shape
        S, K = graph.idx.shape[1:]
        O = weight.shape[0]
        w = weight.detach().reshape(O, 2 * C)
        al, be = alpha.detach().reshape(1, C), beta.detach().reshape(1, C)
        ws = torch.cat([w[:, :C] * al, w[:, C:]], 0)             # (2O, C): [Wa ; W2]
        c0 = w[:, :C] @ be.reshape(C)                             # W1 beta
        lib = _lib.load()
        n = S * K * C
        mom = moments(x, graph)
        mean = mom[:, 0] / n
        sigma = ((mom[:, 1] - mom[:, 0] * mean) / (n - 1)).clamp_min(0.0).sqrt()
        r = (1.0 / (sigma + 1e-5)).float()
        pq = torch.empty(B, N, 2 * O, device=dev)
        contract(B, N, 2 * O, C, x, N * C, C, True, ws, 0, C, True, pq, d_batch=N * 2 * O, ldd=2 * O)
        ctx.graph = graph
        ctx.shapes = (weight.shape, alpha.shape, beta.shape)
        if bn is None:
            y = torch.empty(B, O, S * K, device=dev)
            part = torch.empty(lib.apn_pw_conv_tiles(B, S * K), 2, O, device=dev)
            _call("apn_ag_combine_fwd", dev, B, N, S, K, O, pq.data_ptr(), graph.idx.data_ptr(), graph.fps_idx.data_ptr(),
                  r.data_ptr(), c0.data_ptr(), y.data_ptr(), part.data_ptr(), 1, None, None, None, None, 0.0, 0, None, None)
            ctx.save_for_backward(x, ws, pq, r, sigma, mean, w, al, be)
            ctx.eval_cfg = None
            ctx.mark_non_differentiable(part)
            return y, part
        # eval mode: scale, shift and ReLU in the combine launch; y (what apn_pw_bn_act_grad reads) only for a backward pass
        y = torch.empty(B, O, S * K, device=dev) if any(ctx.needs_input_grad) else None
        out = torch.empty(B, O, S * K, device=dev)
        stat = torch.empty(4, O, device=dev)
        _call("apn_ag_combine_fwd", dev, B, N, S, K, O, pq.data_ptr(), graph.idx.data_ptr(), graph.fps_idx.data_ptr(),
              r.data_ptr(), c0.data_ptr(), _ptr(y), None, 0, _ptr(gamma), _ptr(bias), bn.running_mean.data_ptr(),
              bn.running_var.data_ptr(), float(bn.eps), int(relu), stat.data_ptr(), out.data_ptr())
        ctx.save_for_backward(x, ws, pq, r, sigma, mean, w, al, be, y, stat)
        ctx.eval_cfg = (bool(relu), gamma is not None, bias is not None)
        ctx.mark_non_differentiable(stat)
        return out, stat

    @staticmethod
    def backward(ctx, gy, _):
        from .pointwise import contract
        x, ws, pq, r, sigma, mean, w, al, be = ctx.saved_tensors[:9]
        graph = ctx.graph
        dev = x.device
        B, N, C = x.shape
        S, K = graph.idx.shape[1:]
        O = ws.shape[0] // 2
        lib = _lib.load()
        gy = gy.contiguous()
        g_gamma = g_bias = None
        if ctx.eval_cfg is not None:
            # gy arrived as dL/d out: through the eval-mode BatchNorm (+ ReLU) first
            gy, g_gamma, g_bias = batchnorm.bn_act_grad(gy, *ctx.saved_tensors[9:], False, *ctx.eval_cfg)
        gyt = torch.empty(B, S * K, O, device=dev)
        _call("apn_pw_transpose", dev, B, O, S * K, gy.data_ptr(), gyt.data_ptr())
        rows = lib.apn_ag_point_rows(N)
        dpq = torch.empty(B, N, 2 * O, device=dev)
        part_dr = torch.empty(rows, B, dtype=torch.float64, device=dev)
        part_c0 = torch.empty(B * rows, O, dtype=torch.float64, device=dev)
        _call("apn_ag_combine_bwd", dev, B, N, S, K, O, gyt.data_ptr(), r.data_ptr(), pq.data_ptr(),
              graph.nbr_cnt_off.data_ptr(), graph.nbr_list.data_ptr(), graph.anc_cnt_off.data_ptr(),
              graph.anc_list.data_ptr(), dpq.data_ptr(), part_dr.data_ptr(), part_c0.data_ptr())
        g_x = g_w = g_alpha = g_beta = None
        need_w, need_alpha, need_beta = ctx.needs_input_grad[1:4]
        if ctx.needs_input_grad[0]:
            dr = _fold(part_dr, rows, B)
            n = S * K * C
            r64 = 1.0 / (sigma + 1e-5)
            # (sigma == 0: every d is equal, the reference's gradient is undefined there; the path is dropped.  No
            # zeros_like: under capture it would be a memset node)
            kappa = (-r64 * r64 * dr / ((n - 1) * sigma.clamp_min(1e-30))) * (sigma > 0).double()
            kappa, mu = kappa.float(), mean.float()
            g_x = torch.empty(B, N, C, device=dev)
            _call("apn_ag_sigma_bwd", dev, B, N, S, K, C, x.data_ptr(), graph.idx.data_ptr(), graph.fps_idx.data_ptr(),
                  kappa.data_ptr(), mu.data_ptr(), graph.nbr_cnt_off.data_ptr(), graph.nbr_list.data_ptr(),
                  graph.anc_cnt_off.data_ptr(), graph.anc_list.data_ptr(), g_x.data_ptr())
            # dL/dx[b] (N x C) += [dP | dQ][b] (N x 2O) [Wa ; W2] (2O x C)
            lin = torch.empty(B, N, C, device=dev)
            contract(B, N, C, 2 * O, dpq, N * 2 * O, 2 * O, True, ws, 0, C, False, lin, d_batch=N * C, ldd=C)
            g_x += lin
        if need_w or need_alpha or need_beta:
            # d[Wa ; W2] (2O x C) = sum_b [dP | dQ][b]^T x[b] in fixed-order shares, then the chain to W, alpha and beta by
            # hand: Wa = W1 alpha, c0 = W1 beta.  (Autograd would do it through slices of W, whose backward pass zero-fills
            # a tensor: a memset node in a captured step from O = 512 on.)  The column sums go through apn_ag_fold.
            g_ws = torch.empty(2 * O, C, device=dev)
            contract(B, 2 * O, C, N, dpq, N * 2 * O, 2 * O, False, x, N * C, C, False, g_ws, reduce=True)
            dc0 = _fold(part_c0, B * rows, O).float().view(O, 1)
            w1 = w[:, :C]
            if need_w:
                g_w = torch.cat([g_ws[:O] * al + dc0 * be, g_ws[O:]], 1).view(ctx.shapes[0])
            if need_alpha:
                g_alpha = _fold((g_ws[:O] * w1).double().contiguous(), O, C).float().view(ctx.shapes[1])
            if need_beta:
                g_beta = _fold((w1 * dc0).double().contiguous(), O, C).float().view(ctx.shapes[2])
        return g_x, g_w, g_alpha, g_beta, None, None, None, g_gamma, g_bias


def _need_cuda(what, *tensors):
    if not all(t.is_cuda for t in tensors):
        raise RuntimeError(f"adaptpoint_amd.affine_group.{what} needs CUDA/HIP tensors: the product path has no CPU "
                           "fallback")


def _check_inputs(x, graph, alpha, beta, weight):
    _need_cuda("affine_group_linear", x, graph.idx)
    if graph.nbr_list is None:
        raise RuntimeError("affine_group_linear: the GroupIndex carries no reverse lists (build it from CUDA tensors)")
    C = x.shape[2]
    if weight.shape[0] * 2 * C != weight.numel() or alpha.numel() != C or beta.numel() != C:
        raise RuntimeError(f"affine_group_linear: weight {tuple(weight.shape)}, alpha {tuple(alpha.shape)}, beta "
                           f"{tuple(beta.shape)} for {C} channels")


def affine_group_linear(x, graph, alpha, beta, weight):
    """y (B,O,S K) = W [alpha (x[idx] - x[fps_idx]) r + beta ; x[fps_idx]] in the hoisted form, and BatchNorm's partial
    rows of y (what `bn_act` folds).  x (B,N,C) rows; graph: the stage's `GroupIndex`; alpha, beta: the grouper's
    affine parameters (C elements); weight: the bias-free 1x1 convolution's (O, 2C[, 1])."""
    _check_inputs(x, graph, alpha, beta, weight)
    return _AffineGroupLinear.apply(x.float(), weight, alpha, beta, graph)


def affine_group_bn_act(x, graph, alpha, beta, weight, bn, relu=True):
    """[relu](bn(y)) for y = `affine_group_linear(x, graph, alpha, beta, weight)` and the BatchNorm module `bn`.  In
    training mode the combine launch leaves BatchNorm's partial rows and apn_pw_bn_act follows (running buffers
    updated); in eval mode the combine launch applies the running statistics itself: one launch, y not written unless a
    gradient is wanted."""
    if batchnorm.mode(bn)[0]:
        y, part = affine_group_linear(x, graph, alpha, beta, weight)
        return bn_act(y, part, bn, relu)
    _check_inputs(x, graph, alpha, beta, weight)
    return _AffineGroupLinear.apply(x.float(), weight, alpha, beta, graph, bn, relu, bn.weight, bn.bias)[0]


def bn_act(y, part, bn, relu=True):
    """[relu](bn(y)) for y (B,C,N) and its partial rows `part` as `affine_group_linear` returns them."""
    return batchnorm.BNAct.apply(y, part, bn.weight, bn.bias, bn, relu)


class _ResReluMax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, h, K):
        z, h = z.contiguous(), h.contiguous()
        B, O, SK = z.shape
        S = SK // K
        out = torch.empty(B, O, S, device=z.device)
        sel = torch.empty(B, O, S, dtype=torch.uint8, device=z.device)
        _call("apn_ag_res_relu_max", z.device, B, O, S, K, z.data_ptr(), h.data_ptr(), out.data_ptr(), sel.data_ptr())
        ctx.save_for_backward(out, sel)
        ctx.K = K
        return out

    @staticmethod
    def backward(ctx, g):
        out, sel = ctx.saved_tensors
        B, O, S = out.shape
        g = g.contiguous()
        gz = torch.empty(B, O, S * ctx.K, device=g.device)
        _call("apn_ag_res_relu_max_grad", g.device, B, O, S, ctx.K, g.data_ptr(), out.data_ptr(), sel.data_ptr(),
              gz.data_ptr(), None)
        return gz, gz, None                                   # (the same values for both: one tensor)


def res_relu_max(z, h, K):
    """out (B,O,S) = max_k relu(z + h) for z, h (B,O,S K) with position s K + k: the tail of the last
    `ConvBNReLURes1D` of a PreExtraction fused with its adaptive_max_pool1d.  The first maximum takes the gradient."""
    _need_cuda("res_relu_max", z, h)
    if z.shape != h.shape or z.dim() != 3 or z.shape[2] % K or not 1 <= K <= K_MAX:
        raise RuntimeError(f"res_relu_max: z {tuple(z.shape)}, h {tuple(h.shape)}, K = {K}")
    return _ResReluMax.apply(z.float(), h.float(), K)
