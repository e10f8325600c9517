"""Feature propagation with its convolution hoisted to the coarse points (csrc/feature_prop.hip).

The decoder block of the imitator (`PointNetFeaturePropagation`, generator_component4_15.py:330-366), of PointNeXt
(`FeaturePropogation`, pointnext.py:173-226) and of PointNet++ (pointnetv2.py:108-150) is

    y = relu(bn(W [f1 ; blend(f2)]))      f1 (B,C1,n) dense skip features, f2 (B,C2,m) coarse features, m < n
    blend(u)[b,o,i] = sum_j weight[b,i,j] u[b,o,idx[b,i,j]],  j < 3                     (three_interpolate)

The convolution and the interpolation are both linear, so the convolution can run BEFORE the interpolation:

    W [f1 ; blend(f2)] = W[:, :C1] f1 + blend(W[:, C1:] f2)

-- the coarse product on m points instead of n, the interpolation (and its gradient) on O channels instead of C2, and
neither the interpolated (B,C2,n) tensor nor the (B,C1+C2,n) concatenation exist.  On the device a block is

    forward   a = W[:, :C1] f1 | u = W[:, C1:] f2      ONE launch of the contraction kernel (apn_pw_contract2), the
                                                        weight's column blocks addressed in place
              y = a + blend(u) (+ BatchNorm partials)   apn_fp_blend_stats
              out = relu(bn(y))                         batchnorm.bn_act (training); in eval mode the previous launch does it
    backward  gy = dL/dy                                batchnorm.bn_act_grad
              gu = blend^T(gy)                          apn_three_interpolate_grad on O channels into a zeroed (B,O,m)
              g_f1 = W[:, :C1]^T gy | g_f2 = W[:, C1:]^T gu            one two-problem launch
              gW[:, :C1] = sum gy f1^T | gW[:, C1:] = sum gu f2^T      one two-problem launch + one fold

Every sum runs in a fixed order while `apn_three_interpolate_grad` takes its sorted-gather form, i.e. while
28 n + 8 m bytes of map fit its 96 KB budget and m <= 8192 (every imitator shape up to N = 2048): results and gradients
are then bit-identical from run to run.  Beyond that the gradient of the blend falls back to LDS / global float atomics:
still correct, no longer bit-reproducible.

With `cond` (B,Cc) -- a per-cloud vector that the composed block repeats over the n points and concatenates in FRONT of
f1 (the class conditioning of `PointNextPartDecoder`, pointnext.py:626-663) -- the convolution has Cc + C1 + C2 input
channels and

    W [cond 1^T ; f1 ; blend(f2)] = (W[:, :Cc] cond_b) 1^T + W[:, Cc:Cc+C1] f1 + blend(W[:, Cc+C1:] f2)

so the vector's share is a bias c (B,O) per (cloud, channel) in front of the BatchNorm: neither the (B,Cc,n) repeat nor
the (B,Cc+C1+C2,n) concatenation exist.  c = cond W[:, :Cc]^T, g_cond = gc W[:, :Cc] and gW[:, :Cc] = gc^T cond are
products with B rows, each ONE launch of `pointwise.contract` (the project's contraction kernel: fixed-order sums, no
split-K, so no scratch and no memset node); y = (a + blend(u)) + c in this association order (apn_fp_blend_stats_cond,
the same kernel); gc = the row sums of gy (apn_fp_cond_grad, fixed order).

`propagate` takes the torch modules (their parameters are used, their buffers updated in place), so `state_dict`s stay
the reference's: the block still owns ONE Conv1d(C1 + C2, O, 1).  On CPU tensors, or where `supported` says no, the
same hoisted algebra runs as plain torch operations under autograd.
"""
import ctypes

import torch
import torch.nn.functional as F

from . import _lib, batchnorm
from .batchnorm import ptr


def supported(f1, f2, conv, bn, cond=None):
    """What the kernels serve: float32 CUDA contiguous f1 (B,C1,n) (or None) and f2 (B,C2,m), a plain bias-free 1x1
    convolution over C1 + C2 channels, a BatchNorm with a numeric momentum (`pointwise.supported`'s conditions); with
    `cond`: a float32 CUDA contiguous (B,Cc) tensor, Cc > 0, and Cc + C1 + C2 input channels."""
    feats = [f2] if f1 is None else [f1, f2]
    cc = 0
    if cond is not None:
        if not (isinstance(cond, torch.Tensor) and cond.is_cuda and cond.dtype == torch.float32 and cond.dim() == 2
                and cond.is_contiguous() and cond.shape[0] == f2.shape[0] and cond.shape[1] > 0):
            return False
        cc = cond.shape[1]
    if not all(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 3 and t.is_contiguous()
               and t.shape[2] > 0 for t in feats):
        return False
    if not isinstance(conv, (torch.nn.Conv1d, torch.nn.Conv2d)) or not isinstance(bn, torch.nn.modules.batchnorm._BatchNorm):
        return False
    one = lambda t, v: all(k == v for k in t)
    c1 = 0 if f1 is None else f1.shape[1]
    return (0 < f2.shape[0] <= 65535 and (f1 is None or f1.shape[0] == f2.shape[0])
            and one(conv.kernel_size, 1) and one(conv.stride, 1) and one(conv.padding, 0) and one(conv.dilation, 1)
            and conv.groups == 1 and conv.weight.dtype == torch.float32 and conv.weight.is_cuda and conv.bias is None
            and conv.in_channels == cc + c1 + f2.shape[1] and c1 + f2.shape[1] > c1
            and (bn.momentum is not None or not bn.training) and (bn.training or bn.track_running_stats))


def blend(u, nearest, weights):
    """three_interpolate as plain torch operations: u (B,O,m), nearest (B,n,3) integer, weights (B,n,3) -> (B,O,n)."""
    B, O, _ = u.shape
    n = nearest.shape[1]
    idx = nearest.long()
    out = None
    for j in range(3):
        term = torch.gather(u, 2, idx[:, :, j].unsqueeze(1).expand(B, O, n)) * weights[:, :, j].unsqueeze(1).to(u.dtype)
        out = term if out is None else out + term
    return out


def _propagate_torch(f1, f2, nearest, weights, conv, bn, relu, cond=None):
    cc = 0 if cond is None else cond.shape[1]
    c1 = cc + (0 if f1 is None else f1.shape[1])
    w = conv.weight.reshape(conv.out_channels, conv.in_channels, 1)
    y = blend(F.conv1d(f2, w[:, c1:]), nearest, weights)
    if f1 is not None:
        y = F.conv1d(f1, w[:, cc:c1]) + y
    if cond is not None:
        y = y + (cond.to(w.dtype) @ w[:, :cc, 0].t()).unsqueeze(-1)          # (a + blend(u)) + c, the kernel's order
    if conv.bias is not None:
        y = y + conv.bias.view(1, -1, 1)
    y = batchnorm.module_forward(y, bn)
    return torch.relu(y) if relu else y


def _pair(ctype, v0, v1):
    return (ctype * 2)(v0, v1)


def _contract2(dev, a_kcont, b_kcont, probs, splits=None, scratch=None):
    """apn_pw_contract2 on two problems (nbatch, r, q, k, a_ptr, a_batch, lda, b_ptr, b_batch, ldb, d_ptr, d_batch, ldd)."""
    from .fused import _call
    from .pointwise import PRECISION
    cols = list(zip(*probs))
    I, L, P = ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p
    kinds = (I, I, I, I, P, L, I, P, L, I, P, L, I)
    arr = [_pair(k, *c) for k, c in zip(kinds, cols)]
    sp = _pair(I, *(splits or (0, 0)))
    sc = _pair(P, *(scratch or (None, None)))
    # (the arrays are read during the call only: the launch's arguments are copied by the runtime)
    _call("apn_pw_contract2", dev, int(a_kcont), int(b_kcont), PRECISION, arr[0], arr[1], arr[2], arr[3], arr[4], arr[5],
          arr[6], arr[7], arr[8], arr[9], arr[10], arr[11], arr[12], sp, sc)


class _HoistedPropagation(torch.autograd.Function):
    @staticmethod
    def forward(ctx, f1, f2, weight, gamma, beta, nearest, weights, bn, relu, cond=None):
        from .fused import _call
        from .pointwise import contract
        dev = f2.device
        B, C2, m = f2.shape
        n = nearest.shape[1]
        C1 = 0 if f1 is None else f1.shape[1]
        Cc = 0 if cond is None else cond.shape[1]
        C = Cc + C1 + C2
        O = weight.shape[0]
        w = weight.detach().reshape(O, C).contiguous()
        wf = w.data_ptr() + 4 * Cc                          # the feature columns W[:, Cc:], addressed in place
        training = batchnorm.mode(bn)[0]
        u = torch.empty(B, O, m, device=dev)
        a = None
        if f1 is not None:
            a = torch.empty(B, O, n, device=dev)
            _contract2(dev, True, False, [
                (B, O, n, C1, wf, 0, C, f1.data_ptr(), C1 * n, n, a.data_ptr(), O * n, n),
                (B, O, m, C2, wf + 4 * C1, 0, C, f2.data_ptr(), C2 * m, m, u.data_ptr(), O * m, m)])
        else:
            contract(B, O, m, C2, w[:, Cc:], 0, C, True, f2, C2 * m, m, False, u, d_batch=O * m, ldd=m)
        cvec = None
        if cond is not None:
            # c (B,O) = cond (B x Cc) W[:, :Cc]^T: W's element (o, k) at o * C + k
            cvec = torch.empty(B, O, device=dev)
            contract(1, B, O, Cc, cond, 0, Cc, True, w, 0, C, True, cvec)
        blend_entry = ("apn_fp_blend_stats",) if cvec is None else ("apn_fp_blend_stats_cond",)
        cargs = () if cvec is None else (cvec.data_ptr(),)
        needs_grad = any(ctx.needs_input_grad[:5]) or (cond is not None and ctx.needs_input_grad[9])
        if training:
            y = a if a is not None else torch.empty(B, O, n, device=dev)       # (the blend adds into the skip product)
            tiles = _lib.load().apn_pw_conv_tiles(B, n)
            part = torch.empty(tiles, 2, O, device=dev)
            _call(*blend_entry, dev, B, O, m, n, ptr(a), u.data_ptr(), nearest.data_ptr(), weights.data_ptr(), *cargs,
                  y.data_ptr(), part.data_ptr(), 1, None, None, None, None, float(bn.eps), int(relu), None, None)
            out, stat = batchnorm.bn_act(y, part, tiles, gamma, beta, bn, relu)
        else:
            y = (a if a is not None else torch.empty(B, O, n, device=dev)) if needs_grad else None
            out = torch.empty(B, O, n, device=dev)
            stat = torch.empty(4, O, device=dev)
            _call(*blend_entry, dev, B, O, m, n, ptr(a), u.data_ptr(), nearest.data_ptr(), weights.data_ptr(), *cargs,
                  ptr(y), None, 0, ptr(gamma), ptr(beta), bn.running_mean.data_ptr(), bn.running_var.data_ptr(),
                  float(bn.eps), int(relu), stat.data_ptr(), out.data_ptr())
        ctx.save_for_backward(f1, f2, w, y, stat, nearest, weights, cond)
        ctx.cfg = (training, relu, gamma is not None, beta is not None, weight.shape)
        return out

    @staticmethod
    def backward(ctx, g):
        from .fused import _call
        from .ops import zeros
        from .pointwise import contract
        f1, f2, w, y, stat, nearest, weights, cond = ctx.saved_tensors
        training, relu, has_gamma, has_beta, wshape = ctx.cfg
        dev = f2.device
        B, C2, m = f2.shape
        n = nearest.shape[1]
        C1 = 0 if f1 is None else f1.shape[1]
        Cc = 0 if cond is None else cond.shape[1]
        C = Cc + C1 + C2
        O = w.shape[0]
        wf = w.data_ptr() + 4 * Cc
        lib = _lib.load()
        need_cond = cond is not None and ctx.needs_input_grad[9]
        need_f1 = f1 is not None and ctx.needs_input_grad[0]
        need_f2, need_w = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        gy, g_gamma, g_beta = batchnorm.bn_act_grad(g, y, stat, training, relu, has_gamma, has_beta)
        g_f1 = g_f2 = gw = g_cond = gc = None
        if cond is not None and (need_cond or need_w):
            gc = torch.empty(B, O, device=dev)
            _call("apn_fp_cond_grad", dev, B, O, n, gy.data_ptr(), gc.data_ptr())
        if need_cond:
            # g_cond (B,Cc) = gc (B x O) W[:, :Cc]: W's element (k = o, c) at k * C + c
            g_cond = torch.empty(B, Cc, device=dev)
            contract(1, B, Cc, O, gc, 0, O, True, w, 0, C, False, g_cond)
        if need_f2 or need_w:
            gu = zeros(B, O, m, device=dev)                  # a kernel fill: capturable (no memset node)
            _call("apn_three_interpolate_grad", dev, B, O, n, m, gy.data_ptr(), nearest.data_ptr(), weights.data_ptr(),
                  gu.data_ptr())
        # the input gradients: W^T read in place (element (c, o) at w[o * C + c]), the two column blocks side by side
        if need_f1:
            g_f1 = torch.empty(B, C1, n, device=dev)
        if need_f2:
            g_f2 = torch.empty(B, C2, m, device=dev)
        if need_f1 and need_f2:
            _contract2(dev, False, False, [
                (B, C1, n, O, wf, 0, C, gy.data_ptr(), O * n, n, g_f1.data_ptr(), C1 * n, n),
                (B, C2, m, O, wf + 4 * C1, 0, C, gu.data_ptr(), O * m, m, g_f2.data_ptr(), C2 * m, m)])
        elif need_f1:
            contract(B, C1, n, O, w[:, Cc:], 0, C, False, gy, O * n, n, False, g_f1, d_batch=C1 * n, ldd=n)
        elif need_f2:
            contract(B, C2, m, O, w[:, Cc + C1:], 0, C, False, gu, O * m, m, False, g_f2, d_batch=C2 * m, ldd=m)
        if need_w:
            gw = torch.empty(O, C, device=dev)
            if f1 is not None:
                s0 = lib.apn_pw_contract2_splits(0, B, O, C1, n, B, O, C2, m)
                s1 = lib.apn_pw_contract2_splits(1, B, O, C1, n, B, O, C2, m)
                sc0 = torch.empty(s0, O, C1, device=dev)
                sc1 = torch.empty(s1, O, C2, device=dev)
                _contract2(dev, True, True, [
                    (B, O, C1, n, gy.data_ptr(), O * n, n, f1.data_ptr(), C1 * n, n, gw.data_ptr() + 4 * Cc, 0, C),
                    (B, O, C2, m, gu.data_ptr(), O * m, m, f2.data_ptr(), C2 * m, m, gw.data_ptr() + 4 * (Cc + C1), 0, C)],
                    splits=(s0, s1), scratch=(sc0.data_ptr(), sc1.data_ptr()))
            elif cond is None:
                contract(B, O, C2, m, gu, O * m, m, True, f2, C2 * m, m, True, gw, reduce=True)
            else:
                # (the reducing form writes rows of q floats: into a tight matrix, then the column block)
                gw2 = torch.empty(O, C2, device=dev)
                contract(B, O, C2, m, gu, O * m, m, True, f2, C2 * m, m, True, gw2, reduce=True)
                gw[:, Cc:] = gw2
            if cond is not None:
                # gW[:, :Cc] (O x Cc, leading dimension C) = gc^T cond: gc's element (o, k = b) at k * O + o
                contract(1, O, Cc, B, gc, 0, O, False, cond, 0, Cc, False, gw, ldd=C)
            gw = gw.view(wshape)
        return g_f1, g_f2, gw, g_gamma, g_beta, None, None, None, None, g_cond


def block_parts(block):
    """(conv, bn, relu) of a `convblock` -- Sequential(1x1 conv without bias, BatchNorm[, ReLU]) -- or None for any other
    structure (the callers then keep the composed path)."""
    mods = list(block)
    if len(mods) < 2 or not isinstance(mods[0], (torch.nn.Conv1d, torch.nn.Conv2d)):
        return None
    if not isinstance(mods[1], torch.nn.modules.batchnorm._BatchNorm):
        return None
    relu = isinstance(mods[-1], torch.nn.ReLU)
    conv = mods[0]
    if len(mods) != 2 + relu or conv.bias is not None or conv.groups != 1 or any(k != 1 for k in conv.kernel_size):
        return None
    return conv, mods[1], relu


def propagate(f1, f2, nearest, weights, conv, bn, relu=True, kernels=True, cond=None):
    """[relu](bn(conv([f1 ; three_interpolate(f2, nearest, weights)]))) in the hoisted form.

    f1 (B,C1,n) or None, f2 (B,C2,m); nearest (B,n,3) integer and weights (B,n,3) as `layers.three_nn_weights` returns
    them (they carry no gradient, as in the reference where three_nn is not differentiable); `conv` a 1x1 convolution
    over C1 + C2 channels whose first C1 input channels are f1's (the concatenation's order); `bn` its BatchNorm.
    cond (B,Cc) or None: a per-cloud vector that the composed block repeats over the n points in FRONT of f1 -- `conv`
    then has Cc + C1 + C2 input channels in that order (see the module's text); None: the call as it always was.
    kernels=False: the plain torch form also on the device."""
    if kernels and supported(f1, f2, conv, bn, cond):
        nearest = nearest.detach()
        weights = weights.detach()
        if nearest.dtype != torch.int32 or not nearest.is_contiguous():
            nearest = nearest.to(torch.int32).contiguous()
        if weights.dtype != torch.float32 or not weights.is_contiguous():
            weights = weights.float().contiguous()
        return _HoistedPropagation.apply(f1, f2, conv.weight, bn.weight, bn.bias, nearest, weights, bn, relu, cond)
    return _propagate_torch(f1, f2, nearest.detach(), weights.detach(), conv, bn, relu, cond)
