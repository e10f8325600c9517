"""The host side of every BatchNorm launch: what a `torch.nn.BatchNorm*` module means as kernel arguments.

The only caller of apn_pw_bn_act / apn_pw_bn_act_grad (the per-point pass, csrc/pointwise.hip), apn_sa_bn_fold (sums ->
pack, csrc/sa_glue.hip) and, for the pooled layers, apn_la_stats_fold / apn_sa_wide_consts2; the one place that says when a
module uses batch statistics, which of its buffers a kernel gets, and that momentum=None is refused.  Launches go through
`fused._call`, looked up per launch (fused.py imports this module), so instrumentation that rebinds that name sees them.
"""
from collections import namedtuple

import torch
import torch.nn.functional as F

from . import _lib

# a BatchNorm module as the kernels take it: five device pointers (None: absent), eps, momentum, training as 0 / 1
Args = namedtuple("Args", "gamma beta running_mean running_var num_batches_tracked eps momentum training")


def ptr(t):
    return None if t is None else t.data_ptr()


def mode(bn):
    """(training, track) of a BatchNorm module, or of anything with its attributes (`pointwise._NoNorm`)."""
    return (bn.training or not bn.track_running_stats,
            bool(bn.track_running_stats and bn.running_mean is not None))


def args(bn, no_momentum=None):
    """The `Args` of `bn`.  no_momentum: what stands in for momentum=None (the per-point layers pass 0.0: their
    predicate admits such a module in eval mode, where the kernels do not read it); None refuses it."""
    training, track = mode(bn)
    mom = bn.momentum if bn.momentum is not None else no_momentum
    if mom is None:
        raise RuntimeError("fused BatchNorm: BatchNorm(momentum=None) is not covered (the layer's supported() / "
                           "covers() routes it to the unfused path)")
    return Args(ptr(bn.weight), ptr(bn.bias), ptr(bn.running_mean) if track else None,
                ptr(bn.running_var) if track else None,
                ptr(bn.num_batches_tracked) if (track and bn.training) else None,
                float(bn.eps), float(mom), 1 if training else 0)


def bn_act(y, part, tiles, gamma, beta, bn, relu):
    """(out, stat) = [relu](bn(y)) for contiguous y (B,C,N): in training mode from the `tiles` partial rows `part` that
    y's producer left (running buffers updated), else from the running statistics.  gamma, beta: the parameters as the
    autograd node received them (None: absent).  stat (4,C) is what `bn_act_grad` reads."""
    from .fused import _call
    B, C, N = y.shape
    a = args(bn, no_momentum=0.0)
    out = torch.empty_like(y)
    stat = torch.empty(4, C, device=y.device)
    _call("apn_pw_bn_act", y.device, B, C, N, y.data_ptr(), ptr(part) if a.training else None, tiles, ptr(gamma),
          ptr(beta), a.eps, a.momentum, a.training, int(relu), a.running_mean, a.running_var, a.num_batches_tracked,
          stat.data_ptr(), out.data_ptr())
    return out, stat


def bn_act_grad(g, y, stat, training, relu, has_gamma, has_beta):
    """(dL/dy, dL/dgamma, dL/dbeta) of `bn_act` from g = dL/dout; the parameter gradients None where absent."""
    from .fused import _call
    B, C, N = y.shape
    dev = y.device
    g = g.contiguous()
    part_b = torch.empty(_lib.load().apn_pw_bn_act_grad_splits(B, C), 2, C, device=dev)
    gy = torch.empty_like(y)
    ggb = torch.empty(2, C, device=dev)
    _call("apn_pw_bn_act_grad", dev, B, C, N, g.data_ptr(), y.data_ptr(), stat.data_ptr(), int(training), int(relu),
          part_b.data_ptr(), gy.data_ptr(), ggb[0].data_ptr(), ggb[1].data_ptr())
    return gy, (ggb[0] if has_gamma else None), (ggb[1] if has_beta else None)


class BNAct(torch.autograd.Function):
    """[relu](bn(y)) for y (B,C,N) whose partial rows exist already (`affine_group.bn_act`)."""

    @staticmethod
    def forward(ctx, y, part, gamma, beta, bn, relu):
        y = y.contiguous()
        out, stat = bn_act(y, part, _lib.load().apn_pw_conv_tiles(y.shape[0], y.shape[2]), gamma, beta, bn, relu)
        ctx.save_for_backward(y, stat)
        ctx.cfg = (mode(bn)[0], relu, gamma is not None, beta is not None)
        return out

    @staticmethod
    def backward(ctx, g):
        y, stat = ctx.saved_tensors
        gy, g_gamma, g_beta = bn_act_grad(g, y, stat, *ctx.cfg)
        return gy, None, g_gamma, g_beta, None, None


def fold(src, rows, C, count, bn, training, dev, summed=False, sgn_from=None, sgn_c=0):
    """(pack, sgn): BatchNorm's fold -- {sum[C], sumsq[C]} over `count` positions -> pack {scale, shift, mean, invstd}[C]
    (float32, (4C,)), running buffers and num_batches_tracked updated as torch.nn.BatchNorm does.  src: the `rows`
    float32 partial rows, or (summed) the float64 sums with {count, world size} appended, as an exchange over ranks
    leaves them; not read in eval mode.  Rider: sgn (sgn_c,) = the sign of another BatchNorm's gamma `sgn_from`."""
    from .fused import _call
    a = args(bn)
    pack = torch.empty(4 * C, dtype=torch.float32, device=dev)
    sgn = torch.empty(sgn_c, dtype=torch.float32, device=dev) if sgn_c else None
    _call("apn_sa_bn_fold", dev, ptr(src) if (training and not summed) else None, rows, ptr(src) if summed else None, C,
          float(count), a.gamma, a.beta, a.eps, a.momentum, a.running_mean, a.running_var, a.num_batches_tracked,
          1 if training else 0, pack.data_ptr(), ptr(sgn_from), sgn_c, ptr(sgn))
    return pack, sgn


def pooled_stats_pack(part, rows, H, count, bn, training, sync):
    """The pack of a pooled layer (LocalAggregation, EdgeConv): its pool kernel's float64 partial rows `part` (None in
    eval mode) -> sums (all-reduced over ranks with `sync`) -> `fold`."""
    from .fused import _allreduce_sum_, _call
    dev = part.device if training else bn.running_mean.device
    sums = None
    if training:
        sums = torch.empty(2 * H + 2, dtype=torch.float64, device=dev)
        _call("apn_la_stats_fold", dev, part.data_ptr(), rows, H, count, sums.data_ptr())
        if sync:
            _allreduce_sum_(sums)
    return fold(sums, 0, H, count, bn, training, dev, summed=True)[0]


def dense_terms(partS, prow, H, pack, count, training, sums=None):
    """(de, g_gamma, g_beta) of a pooled layer's backward pass from the `prow` partial rows {sum g, sum g yhat} (or from
    their all-reduced `sums`): de (2H,) the dense terms of dL/dy, zero on running statistics."""
    from .fused import _call
    small = torch.empty(4 * H, dtype=torch.float32, device=partS.device)
    de, g_gamma, g_beta = small[:2 * H], small[2 * H:3 * H], small[3 * H:]
    _call("apn_sa_wide_consts2", partS.device, None if sums is not None else partS.data_ptr(), prow, ptr(sums), H,
          pack.data_ptr(), count, 1 if training else 0, de.data_ptr(), g_gamma.data_ptr(), g_beta.data_ptr())
    return de, g_gamma, g_beta


def module_forward(y, bn):
    """`bn(y)` for a BatchNorm module through F.batch_norm, whatever y's rank (buffers updated as the module's forward
    updates them): the layers' plain-torch paths."""
    factor = 0.0 if bn.momentum is None else bn.momentum
    if bn.training and bn.track_running_stats and bn.num_batches_tracked is not None:
        bn.num_batches_tracked.add_(1)
        if bn.momentum is None:
            factor = 1.0 / float(bn.num_batches_tracked)
    use_batch = bn.training or (bn.running_mean is None and bn.running_var is None)
    keep = not bn.training or bn.track_running_stats
    return F.batch_norm(y, bn.running_mean if keep else None, bn.running_var if keep else None, bn.weight, bn.bias,
                        use_batch, factor, bn.eps)
