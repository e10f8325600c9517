"""PointNeXt set-abstraction block over the gfx950 operators.

Host-side mirror of `SetAbstraction` in the reference
(openpoints/models/backbone/pointnext.py:82-170) restricted to what the configs
in scope instantiate (cfgs/scanobjectnn/pointnext-s.yaml:5-36): conv-norm-act
order, BatchNorm, ReLU, FPS sampler, ball-query or group-all grouping, max
pooling, optional residual.  Sub-module names and nesting match the reference
(`convs.<i>.0` conv, `convs.<i>.1` norm, `skipconv.0`), so a reference
state_dict loads unchanged.
"""
import logging
from typing import NamedTuple

import torch
import torch.nn as nn

from . import fused, fused_wide, layers, pointwise
from .layers import BallGrouper, make_grouper

_log = logging.getLogger("adaptpoint_amd")

# fused=True requests that fall back to the unfused operators, by reason (bench.py reports the
# total; each distinct reason is logged once).
FUSED_FALLBACKS = {}


# True: the width-generic kernels (csrc/sa_wide.hip) also take the 32 -> 32 -> 64 shape that the
# register-resident kernels of csrc/sa_fused.hip specialise in (A/B switch for benchmarks and tests).
PREFER_WIDE = False
# the fused index stage (apn_sa_sample_seq -> the resident samplers of csrc/fps.hip) keeps a cloud in registers / LDS:
# larger clouds take the unfused operators, whose FPS is the streaming sampler (csrc/fps.hip: fps_stream_kernel)
MAX_SAMPLE_SEQ_POINTS = 16384

# The paths of one call (`route`)
STEM = "stem"                # is_head: the 1x1 convolutions alone (csrc/pointwise.hip when fused)
GROUP_ALL = "group_all"      # all_aggr, fused: the per-point contraction kernels, then the pool
RESIDENT = "resident"        # the whole block on the register-resident kernels (fused.fused_set_abstraction)
WIDE = "wide"                # the block after its index stage on the width-generic kernels (fused_wide.block)
GROUPED = "grouped"          # unfused index stage, then the grouped MLP alone (fused / fused_wide.grouped_mlp_max)
COMPOSED = "composed"        # the unfused operators + PyTorch


class Plan(NamedTuple):
    """A block's structure as the kernels see it, from its modules alone (`SetAbstraction.plan`)."""
    kind: str                # "stem", "group_all" or "ball" (FPS + neighbourhoods)
    fused: bool
    mlp: tuple               # (conv1, bn1, conv2, bn2) when the MLP has the fused kernels' structure, else None
    relu_after: bool         # a ReLU after the last BatchNorm
    res: bool                # a residual branch (use_res)
    skip: nn.Module          # its 1x1 Conv1d (None: no branch, or one the kernels cannot take)
    stride: int
    K: int                   # neighbours per query
    widths: tuple            # the convolutions' output channels
    w1: tuple = None         # (out, in) channels of conv1 and of conv2; biased: either has a bias
    w2: tuple = None
    biased: bool = False


class Route(NamedTuple):
    """Where ONE call of a block runs (`route`)."""
    path: str
    wide: bool = False       # on the width-generic kernels (WIDE; GROUPED through fused_wide.grouped_mlp_max)
    fuse_skip: bool = False  # the residual branch runs inside the kernels
    reason: str = None       # why a fused=True call leaves the fused block (counted in FUSED_FALLBACKS)


def route(plan, c_in, B, N, cuda_f32=True, momenta=(), prefer_wide=False, sampling=False):
    """The path of one call, from the block's `Plan` and plain facts of the call: c_in input channels, B clouds of N
    points, float32 CUDA tensors or not, the BatchNorms' momenta, PREFER_WIDE, and whether the index stage is handed in
    (`sampling`).  Attribute and shape checks only: no tensor op, no device sync."""
    if plan.kind == "stem":
        return Route(STEM)
    if not plan.fused:
        return Route(COMPOSED)
    if plan.kind == "group_all":
        return Route(GROUP_ALL)
    M = N // plan.stride
    resident = wide = False
    if plan.mlp is not None and cuda_f32:
        shapes = (c_in, plan.w1, plan.w2, plan.biased, momenta)
        resident = fused.covers(B, N, M, plan.K, *shapes) and not prefer_wide
        wide = fused_wide.covers(B, M, plan.K, *shapes)
    whole = not plan.res or plan.skip is not None          # any residual branch is one the kernels can take
    if resident and whole and N <= MAX_SAMPLE_SEQ_POINTS:
        return Route(RESIDENT, fuse_skip=plan.res)
    reason = None
    if wide and not sampling and N > MAX_SAMPLE_SEQ_POINTS:
        reason = f"N={N} > {MAX_SAMPLE_SEQ_POINTS}: index stage beyond the resident samplers"
    elif wide and whole:
        return Route(WIDE, wide=True, fuse_skip=plan.res and fused_wide.lean(c_in, plan.w1[0]))
    if resident or wide:
        return Route(GROUPED, wide=not resident, reason=reason)
    return Route(COMPOSED, reason=f"C_in={c_in} -> {list(plan.widths)}, K={plan.K}: no fused kernel for this shape")


def _note_fallback(reason):
    if reason not in FUSED_FALLBACKS:
        _log.warning("SetAbstraction(fused=True) runs UNFUSED: %s", reason)
    FUSED_FALLBACKS[reason] = FUSED_FALLBACKS.get(reason, 0) + 1


def _ranks():
    import torch.distributed as dist
    return dist.get_world_size() if (dist.is_available() and dist.is_initialized()) else 1


def _norm(norm_args, channels, dim):
    if norm_args is None:
        return None
    name = norm_args.get('norm', None)
    if name is None:
        return None
    if name in ('bn', 'bn2d', 'bn1d'):
        # create_norm (layers/norm.py): 'bn' resolves by the block's dimension
        return nn.BatchNorm2d(channels) if dim == 2 else nn.BatchNorm1d(channels)
    raise NotImplementedError(f"norm '{name}' is outside the hot-path build")


def _act(act_args):
    if act_args is None:
        return None
    name = act_args.get('act', 'relu')
    if name == 'relu':
        return nn.ReLU(inplace=act_args.get('inplace', True))
    if name == 'leakyrelu':
        # create_act (layers/activation.py): nn.LeakyReLU(negative_slope, inplace)
        return nn.LeakyReLU(act_args.get('negative_slope', 0.01), inplace=act_args.get('inplace', True))
    raise NotImplementedError(f"activation '{name}' is outside the hot-path build")


def convblock(cin, cout, dim, norm_args=None, act_args=None, order='conv-norm-act', bias=True):
    """create_convblock1d/2d (layers/conv.py:24-104) for the conv-norm-act order:
    1x1 conv (bias dropped when a norm follows), norm, activation."""
    if order != 'conv-norm-act':
        raise NotImplementedError(f"conv order '{order}' is outside the hot-path build")
    norm = _norm(norm_args, cout, dim)
    conv_cls = nn.Conv2d if dim == 2 else nn.Conv1d
    layers = [conv_cls(cin, cout, 1, bias=bias and norm is None)]
    if norm is not None:
        layers.append(norm)
    act = _act(act_args)
    if act is not None:
        layers.append(act)
    return nn.Sequential(*layers)


class SetAbstraction(nn.Module):
    """pointnext.py:82-170."""

    def __init__(self, in_channels, out_channels, layers=1, stride=1,
                 group_args=None, norm_args=None, act_args=None, conv_args=None,
                 sampler='fps', feature_type='dp_fj', use_res=False, is_head=False, fused=False,
                 sync_bn=False, **kwargs):
        super().__init__()
        group_args = dict(group_args or {'NAME': 'ballquery', 'radius': 0.1, 'nsample': 16})
        norm_args = {'norm': 'bn1d'} if norm_args is None else norm_args
        act_args = {'act': 'relu'} if act_args is None else act_args
        conv_args = dict(conv_args or {})
        self.stride = stride
        self.is_head = is_head
        self.all_aggr = not is_head and stride == 1
        self.use_res = use_res and not self.all_aggr and not self.is_head
        self.feature_type = feature_type
        # fused=True routes group -> conv/BN/ReLU -> conv/BN -> max through csrc/sa_fused.hip
        # when the shapes allow; sync_bn=True all-reduces its BatchNorm statistics.
        self.fused = fused
        self.sync_bn = sync_bn

        mid_channel = out_channels // 2 if stride > 1 else out_channels
        channels = [in_channels] + [mid_channel] * (layers - 1) + [out_channels]
        if feature_type != 'dp_fj':
            raise NotImplementedError("only the 'dp_fj' aggregation (relative positions + neighbour "
                                      "features; the cfgs in scope) is on the hot path")
        channels[0] = in_channels if is_head else 3 + channels[0]

        if self.use_res:
            self.skipconv = (convblock(in_channels, channels[-1], 1)
                             if in_channels != channels[-1] else nn.Identity())
            self.act = _act(act_args)

        dim = 1 if is_head else 2
        convs = []
        for i in range(len(channels) - 1):
            last = i == len(channels) - 2
            convs.append(convblock(channels[i], channels[i + 1], dim,
                                   norm_args=norm_args if not is_head else None,
                                   act_args=None if last and (self.use_res or is_head) else act_args,
                                   **conv_args))
        self.convs = nn.Sequential(*convs)
        if not is_head:
            if self.all_aggr:
                group_args['nsample'] = None
                group_args['radius'] = None
            self.grouper = make_grouper(group_args)
            if sampler.lower() != 'fps':
                raise NotImplementedError("only the FPS sampler is on the hot path")

    def plan(self):
        """The block's `Plan` (read afresh on every call: modules can be swapped and momenta changed at run time)."""
        if self.is_head:
            return Plan("stem", self.fused, None, False, False, None, self.stride, None, ())
        blocks = [tuple(b) for b in self.convs]          # (unpacked once: indexing an nn.Sequential costs microseconds)
        widths, K = tuple(b[0].out_channels for b in blocks), getattr(self.grouper, 'nsample', None)
        if self.all_aggr:
            return Plan("group_all", self.fused, None, False, False, None, self.stride, K, widths)
        skip = tuple(self.skipconv) if self.use_res and isinstance(self.skipconv, nn.Sequential) else ()
        skip = skip[0] if len(skip) == 1 and isinstance(skip[0], nn.Conv1d) and isinstance(self.act, nn.ReLU) else None
        mlp, relu_after, w1, w2, biased = None, False, None, None, False
        blk1, blk2 = blocks if len(blocks) == 2 else ((), ())
        if (isinstance(self.grouper, BallGrouper) and self.grouper.normalize_dp
                and len(blk1) == 3 and isinstance(blk1[1], nn.BatchNorm2d) and isinstance(blk1[2], nn.ReLU)
                and len(blk2) in (2, 3) and isinstance(blk2[1], nn.BatchNorm2d)
                and (len(blk2) == 2 or isinstance(blk2[2], nn.ReLU))):
            mlp, relu_after = (blk1[0], blk1[1], blk2[0], blk2[1]), len(blk2) == 3
            w1, w2 = tuple(blk1[0].weight.shape[:2]), tuple(blk2[0].weight.shape[:2])
            biased = blk1[0].bias is not None or blk2[0].bias is not None
        return Plan("ball", self.fused, mlp, relu_after, self.use_res, skip, self.stride, K, widths, w1, w2, biased)

    def route(self, c_in, B, N, cuda_f32=True, sampling=False):
        """`route` of a call of this block as it stands (its modules, momenta and PREFER_WIDE read now); c_in None:
        the input channels its conv1 takes."""
        plan = self.plan()
        if c_in is None and plan.w1 is not None:
            c_in = plan.w1[1] - 3
        momenta = (plan.mlp[1].momentum, plan.mlp[3].momentum) if plan.mlp is not None else ()
        return plan, route(plan, c_in, B, N, cuda_f32, momenta, PREFER_WIDE, sampling)

    def sample(self, p, out=None, nested=False, ties=None):
        """The block's index stage alone (FPS + ball query; for the register-resident kernels also the neighbourhoods'
        occurrence statistics) -> adaptpoint_amd.fused.Sampling.  nested, ties: see `fused.sample_and_query`."""
        _, r = self.route(None, p.shape[0], p.shape[1], p.is_cuda and p.dtype == torch.float32, True)
        return fused.sample_and_query(p, p.shape[1] // self.stride, self.grouper.radius, self.grouper.nsample, out=out,
                                      geo=r.path == RESIDENT, nested=nested, ties=ties)

    def index_for(self, smp, n_points, c_in, out=None):
        """What the block's fused kernels derive from the neighbour indices of a Sampling, for c_in input channels
        (index-stage work, to be run where the Sampling is made).  The register-resident kernels take the tile map
        and, for their backward pass, its row map: smp.tmap, smp.rowmap.  The width-generic ones take the
        NeighbourIndex (tile map + inverse map; adaptpoint_amd.fused_wide), stored as smp.index and returned."""
        B, M = smp.idx.shape[0], smp.idx.shape[1]
        _, r = self.route(c_in, B, n_points, smp.idx.is_cuda, True)
        if r.path == RESIDENT:
            smp.tmap = fused_wide.tile_map(smp.idx, out=smp.tmap)
            smp.rowmap = fused_wide.row_map(smp.tmap, B, n_points, M, out=smp.rowmap, fidx=smp.fidx)
        elif r.path == WIDE:
            smp.index = fused_wide.neighbour_index(smp.idx, smp.new_p, n_points, fidx=smp.fidx if r.fuse_skip else None,
                                                   out=out)
            return smp.index
        return None

    def sample_many(self, ps, outs=None):
        """Index stages of several batches, FPS of one sharing its launch with the ball query of
        the previous one (adaptpoint_amd.fused.sample_and_query_many)."""
        return fused.sample_and_query_many(ps, ps[0].shape[1] // self.stride, self.grouper.radius,
                                           self.grouper.nsample, outs=outs)

    @staticmethod
    def pool(x):
        return torch.max(x, dim=-1, keepdim=False)[0]

    def forward(self, pf, sampling=None):
        p, f = pf
        plan, r = self.route(f.shape[1], p.shape[0], p.shape[1],
                             f.is_cuda and f.dtype == torch.float32 and p.dtype == torch.float32, sampling is not None)
        if r.path == STEM:
            for blk in self.convs:                      # a 1x1 convolution (csrc/pointwise.hip when fused)
                f = pointwise.run_block(f, blk, self.fused)
            return p, f
        g, M = self.grouper, p.shape[1] // self.stride
        if r.path == RESIDENT:
            return fused.fused_set_abstraction(p, f, M, g.radius, *plan.mlp, plan.skip, plan.res or plan.relu_after,
                                               sync_bn=self.sync_bn, sampling=sampling)
        if r.path == WIDE:
            return self._wide(p, f, plan, r, sampling)
        if r.path == COMPOSED and r.reason is not None and self.sync_bn and _ranks() > 1:
            # workloads.sync_batchnorm_ left this block's BatchNorms unconverted because the block exchanges its own
            # sums; the composed path below would normalise with RANK-LOCAL statistics -- silently not the reference's
            # SyncBatchNorm (train_autoaug.py:275-282).  Loud instead.
            raise RuntimeError("SetAbstraction(fused=True, sync_bn=True) cannot run its fused kernels (" + r.reason +
                               ") and its BatchNorm modules are plain ones: convert them "
                               "(adaptpoint_amd.dp.convert_sync_batchnorm) or build the block with fused=False")
        if r.reason is not None:
            _note_fallback(r.reason)
        idx = None
        if self.all_aggr:
            new_p = p
        elif sampling is not None:          # index stage computed ahead (adaptpoint_amd.fused.Sampling)
            picks, idx = sampling.fidx.long(), sampling.idx
            new_p = (torch.gather(p, 1, picks.unsqueeze(-1).expand(-1, -1, 3)) if p.requires_grad
                     else sampling.new_p)
        else:
            picks = layers.furthest_point_sample(p, M).long()
            new_p = torch.gather(p, 1, picks.unsqueeze(-1).expand(-1, -1, 3))
        identity = None
        if self.use_res:                 # the skip branch sees the sampled points' own features
            identity = self.skipconv(torch.gather(f, -1, picks.unsqueeze(1).expand(-1, f.shape[1], -1)))
        if r.path == GROUPED:
            if idx is None:
                idx = g.neighbours(new_p, p)
            pooled = (fused_wide if r.wide else fused).grouped_mlp_max(p, new_p, f, idx, g.radius, *plan.mlp,
                                                                       sync_bn=self.sync_bn)
            if plan.relu_after:          # activation after the last BN commutes with the max
                pooled = self.convs[1][2](pooled)
        else:
            dp, fj = self.grouper(new_p, p, f, idx) if idx is not None else self.grouper(new_p, p, f)
            x = torch.cat([dp, fj], 1)                                   # 'dp_fj' (group.py:325-326)
            if r.path == GROUP_ALL:
                # the "grouped" tensor is (B, C, 1, N) = the points themselves; its 1x1 layers run on the per-point
                # contraction kernels
                x = x.squeeze(2)
                for blk in self.convs:
                    x = pointwise.run_block(x, blk)
                pooled = self.pool(x).unsqueeze(-1)
            else:
                pooled = self.pool(self.convs(x))
        if identity is not None:
            pooled = self.act(pooled + identity)
        return new_p, pooled

    def _wide(self, p, f, plan, r, sampling):
        """The WIDE path: the block through the width-generic kernels (adaptpoint_amd.fused_wide), the residual branch
        and the final ReLU inside them when `r.fuse_skip`, else the branch composed through csrc/pointwise.hip."""
        g = self.grouper
        smp = sampling if sampling is not None else fused.sample_and_query(p.detach(), p.shape[1] // self.stride,
                                                                            g.radius, g.nsample)
        nbr = smp.index
        if nbr is None or (r.fuse_skip and nbr.fq is None):
            nbr = fused_wide.neighbour_index(smp.idx, smp.new_p, p.shape[1], fidx=smp.fidx if r.fuse_skip else None)
        new_p = smp.new_p
        if p.requires_grad:            # the sampled coordinates stay differentiable (the AdaptPoint feedback path)
            new_p = torch.gather(p, 1, smp.fidx.long().unsqueeze(-1).expand(-1, -1, 3))
        if r.fuse_skip or not plan.res:
            out = fused_wide.block(p, new_p, f, nbr, g.radius, *plan.mlp, skip_conv=plan.skip,
                                   relu=plan.res or plan.relu_after, sync_bn=self.sync_bn)
            return new_p, out
        pooled = fused_wide.block(p, new_p, f, nbr, g.radius, *plan.mlp, relu=False, sync_bn=self.sync_bn)
        identity = pointwise.run_block(torch.gather(f, -1, smp.fidx.long().unsqueeze(1).expand(-1, f.shape[1], -1)),
                                       self.skipconv)
        return new_p, self.act(pooled + identity)
