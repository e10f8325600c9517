"""PointNeXt-S classifier over the gfx950 set-abstraction blocks; InvResMLP and the general encoder (B / L / XL).

Host-side mirror of the model `cfgs/scanobjectnn/pointnext-s.yaml:5-36` builds in the reference:
`BaseCls` (openpoints/models/classification/cls_base.py:13-39) = `PointNextEncoder`
(openpoints/models/backbone/pointnext.py:312-441; blocks [1]*6, so every stage is one
SetAbstraction and no InvResMLP exists) + `ClsHead` (cls_base.py:78-136).  Module nesting and
names match the reference (`encoder.encoder.<stage>.0....`, `prediction.head.<i>....`), so a
reference state_dict loads unchanged.  Stage 1 (1024 -> 512 points, 32 -> 64 channels) has the
shape the fused kernels cover; the other stages run the unfused extension operators + PyTorch.

`LocalAggregation`, `InvResMLP` (pointnext.py:27-78, 229-276) and `PointNextEncoder` (pointnext.py:311-456, any
`blocks`) are the depth-scaled models' parts: an InvResMLP's aggregation runs on csrc/local_aggr.hip when fused
(adaptpoint_amd.local_aggr), its pointwise convolutions on csrc/pointwise.hip, and one ball query + NeighbourIndex
serves all the InvResMLP blocks of a stage that share radius and nsample.
"""
import torch
import torch.nn as nn

from .set_abstraction import MAX_SAMPLE_SEQ_POINTS, SetAbstraction

# forward_cls_feat without a pyramid handed in builds one itself (nested sampler: blocks 2-4 sample from the previous
# block's samples, which FPS returns as a prefix).  False: every block runs its own full sampler, as the reference does.
NESTED_PYRAMID = True


class PointNextEncoderS(nn.Module):
    """pointnext.py:338-441 for sa_layers=2, sa_use_res=True, one block per stage."""

    def __init__(self, in_channels=4, width=32, strides=(1, 2, 2, 2, 2, 1), radius=0.15,
                 radius_scaling=1.5, nsample=32, fused=False, sync_bn=False):
        super().__init__()
        self.strides = list(strides)
        # _to_full_list (pointnext.py:389-407): the radius grows after every down-sampling stage
        radii, r = [], radius
        for s in self.strides:
            radii.append(r)
            if s != 1:
                r *= radius_scaling
        channels = []
        for s in self.strides:
            if s != 1:
                width *= 2
            channels.append(width)
        stages, cin = [], in_channels
        for i, (s, c) in enumerate(zip(self.strides, channels)):
            is_head = i == 0 and s == 1
            sa = SetAbstraction(cin, c, layers=1 if is_head else 2, stride=s,
                                group_args={'NAME': 'ballquery', 'radius': radii[i], 'nsample': nsample,
                                            'normalize_dp': True},
                                norm_args={'norm': 'bn'}, act_args={'act': 'relu'},
                                conv_args={'order': 'conv-norm-act'}, sampler='fps',
                                feature_type='dp_fj', use_res=True, is_head=is_head,
                                fused=fused, sync_bn=sync_bn)
            stages.append(nn.Sequential(sa))
            cin = c
        self.encoder = nn.Sequential(*stages)
        self.out_channels = channels[-1]
        self.radii = radii

    @torch.no_grad()
    def index_pyramid(self, p0, out=None, events=False):
        """The index stages of ALL blocks -- FPS (+ sampled coordinates) and ball query per
        down-sampling block -- for a batch of coordinates p0 (B,N,3).  They depend on coordinates
        only (block k samples from block k-1's samples), so the whole pyramid can be computed ahead of
        the feature path: on another stream, for the next batch (scripts/bench_pointnext.py --pipeline).
        Returns one `adaptpoint_amd.fused.Sampling` (or None) per block; `out`: buffers to fill.  events: record an
        event behind every block's index stage (`Sampling.ready`); `forward_cls_feat` then waits block by block, so
        a pyramid running on a side stream is consumed level by level instead of as a whole."""
        res, p = [], p0.contiguous()
        ties = None          # block k + 1 samples from block k's samples: the nested sampler (csrc/fps.hip, NEST)
        for i, stage in enumerate(self.encoder):
            sa = stage[0]
            if sa.is_head or sa.all_aggr:
                res.append(None)
                continue
            smp = sa.sample(p, out=None if out is None else out[i], nested=True, ties=ties)
            ties = smp.ties
            # what the block's kernels derive from the neighbourhoods (tile map, row map or NeighbourIndex)
            sa.index_for(smp, p.shape[1], sa.convs[0][0].in_channels - 3, out=smp.index)
            if events:
                from . import graphs
                smp.ready = graphs.ready_event()
            res.append(smp)
            p = smp.new_p
        return res

    def forward_seg_feat(self, p0, f0=None):
        """Every level's (points, features): what the segmentation decoder consumes (pointnext.py:443-453)."""
        if hasattr(p0, 'keys'):
            p0, f0 = p0['pos'], p0.get('x', None)
        if f0 is None:
            f0 = p0.clone().transpose(1, 2).contiguous()
        p, f = [p0], [f0]
        for stage in self.encoder:
            _p, _f = stage[0]([p[-1], f[-1]])
            p.append(_p)
            f.append(_f)
        return p, f

    def forward_cls_feat(self, p0, f0=None, pyramid=None):
        if hasattr(p0, 'keys'):
            p0, f0 = p0['pos'], p0.get('x', None)
        if f0 is None:
            f0 = p0.clone().transpose(1, 2).contiguous()
        if pyramid is None and p0.is_cuda and NESTED_PYRAMID and p0.shape[1] <= MAX_SAMPLE_SEQ_POINTS:
            # (larger clouds: every block samples itself -- the unfused operators' streaming sampler; the nested copy only
            # pays off for N <= 4096 anyway)
            # the index stages of all blocks first (coordinates only; gradients reach p0 through the blocks' own
            # differentiable gathers): deeper levels then cost a copy instead of a sampler chain
            pyramid = self.index_pyramid(p0.detach())
        for i, stage in enumerate(self.encoder):
            smp = None if pyramid is None else pyramid[i]
            if smp is not None and smp.ready is not None:
                torch.cuda.current_stream(p0.device).wait_event(smp.ready)
            p0, f0 = stage[0]([p0, f0], sampling=smp) if smp is not None else stage[0]([p0, f0])
        return f0.squeeze(-1)


_BALL = {'NAME': 'ballquery', 'normalize_dp': True}


class LocalAggregation(nn.Module):
    """pointnext.py:27-78: p grouped around p itself, Conv2d-BN-ReLU blocks, a reduction over the neighbours.
    `forward(pf, index=None)`: index = the neighbours computed ahead -- an idx (B,N,K) tensor or, for the fused
    kernels, the `fused_wide.NeighbourIndex` of it (one per stage: `PointNextEncoder.stage_index`)."""

    def __init__(self, channels, norm_args=None, act_args=None, group_args=None, conv_args=None, feature_type='dp_fj',
                 reduction='max', last_act=True, fused=False, sync_bn=False):
        super().__init__()
        from .set_abstraction import convblock
        norm_args = {'norm': 'bn1d'} if norm_args is None else norm_args
        group_args = dict(group_args or {'NAME': 'ballquery', 'radius': 0.1, 'nsample': 16})
        if feature_type != 'dp_fj' or reduction.lower() != 'max' or group_args.get('NAME', 'ballquery') != 'ballquery':
            raise NotImplementedError("only the 'dp_fj' aggregation with a max over ball-query neighbours is on the "
                                      "hot path")
        channels = list(channels)
        channels[0] += 3
        self.convs = nn.Sequential(*[
            convblock(channels[i], channels[i + 1], 2, norm_args=norm_args,
                      act_args=None if i == len(channels) - 2 and not last_act else act_args, **dict(conv_args or {}))
            for i in range(len(channels) - 1)])
        from .layers import make_grouper
        self.grouper = make_grouper(group_args)
        self.reduction, self.feature_type = 'max', feature_type
        self.fused, self.sync_bn = fused, sync_bn

    def _uncovered(self, p, f):
        """None when csrc/local_aggr.hip covers this call, else the reason it does not."""
        from . import local_aggr
        blocks = [tuple(b) for b in self.convs]
        g = self.grouper
        ok = (len(blocks) == 1 and len(blocks[0]) in (2, 3) and isinstance(blocks[0][1], nn.BatchNorm2d)
              and (len(blocks[0]) == 2 or isinstance(blocks[0][2], nn.ReLU)))
        if ok:
            conv, bn = blocks[0][0], blocks[0][1]
            ok = (bn.training or bn.track_running_stats) and local_aggr.covers(
                p.shape[0], p.shape[1], g.nsample, f.shape[1], tuple(conv.weight.shape[:2]), conv.bias is not None,
                bn.momentum)
        if ok:
            return None
        return (f"LocalAggregation C_in={f.shape[1]} -> {[b[0].out_channels for b in blocks]}, K={g.nsample}: "
                "no fused kernel for this shape")

    def forward(self, pf, index=None):
        from . import fused_wide, local_aggr
        from .set_abstraction import _note_fallback, _ranks
        p, f = pf
        g = self.grouper
        if self.fused and f.is_cuda and f.dtype == torch.float32 and p.dtype == torch.float32:
            reason = self._uncovered(p, f)
            if reason is None:
                if not isinstance(index, fused_wide.NeighbourIndex):
                    pd = p.detach().contiguous()
                    idx = index if index is not None else g.neighbours(pd, pd)
                    index = fused_wide.neighbour_index(idx.contiguous(), pd, p.shape[1])
                blk = tuple(self.convs[0])
                return local_aggr.aggregate(p, f, index, g.radius if g.normalize_dp else 1.0, blk[0], blk[1],
                                            relu=len(blk) == 3, sync_bn=self.sync_bn)
            if self.sync_bn and _ranks() > 1:
                raise RuntimeError("LocalAggregation(fused=True, sync_bn=True) cannot run its fused kernels (" + reason +
                                   ") and its BatchNorm modules are plain ones: convert them "
                                   "(adaptpoint_amd.dp.convert_sync_batchnorm) or build the block with fused=False")
            _note_fallback(reason)
        idx = index.idx if isinstance(index, fused_wide.NeighbourIndex) else index
        dp, fj = g(p, p, f, idx) if idx is not None else g(p, p, f)
        return torch.max(self.convs(torch.cat([dp, fj], 1)), dim=-1, keepdim=False)[0]


class InvResMLP(nn.Module):
    """pointnext.py:229-276: LocalAggregation (one grouped convolution), pointwise convolutions with an expansion,
    the residual add and the activation.  Sub-module names are the reference's (`convs.convs.0.*`, `pwconv.<i>.*`)."""

    def __init__(self, in_channels, norm_args=None, act_args=None, aggr_args=None, group_args=None, conv_args=None,
                 expansion=1, use_res=True, num_posconvs=2, less_act=False, fused=False, sync_bn=False):
        super().__init__()
        from .set_abstraction import _act, convblock
        norm_args = {'norm': 'bn'} if norm_args is None else norm_args
        act_args = {'act': 'relu'} if act_args is None else act_args
        aggr_args = {'feature_type': 'dp_fj', 'reduction': 'max'} if aggr_args is None else aggr_args
        group_args = dict(_BALL, radius=0.1, nsample=32) if group_args is None else group_args
        self.use_res, self.fused = use_res, fused
        mid = int(in_channels * expansion)
        self.convs = LocalAggregation([in_channels, in_channels], norm_args=norm_args,
                                      act_args=act_args if num_posconvs > 0 else None, group_args=group_args,
                                      conv_args=conv_args, fused=fused, sync_bn=sync_bn, **aggr_args)
        channels = [] if num_posconvs < 1 else ([in_channels, in_channels] if num_posconvs == 1
                                                else [in_channels, mid, in_channels])
        self.pwconv = nn.Sequential(*[
            convblock(channels[i], channels[i + 1], 1, norm_args=norm_args,
                      act_args=act_args if i != len(channels) - 2 and not less_act else None, **dict(conv_args or {}))
            for i in range(len(channels) - 1)])
        self.act = _act(act_args)

    def forward(self, pf, index=None):
        from . import pointwise
        p, f = pf
        identity = f
        f = self.convs([p, f], index=index)
        for blk in self.pwconv:
            f = pointwise.run_block(f, blk, self.fused)
        if f.shape[-1] == identity.shape[-1] and self.use_res:
            f = f + identity
        return [p, self.act(f)]


class PointNextEncoder(nn.Module):
    """pointnext.py:311-456 for any `blocks`: stage i = one SetAbstraction (the stem when i == 0 and its stride is 1)
    followed by blocks[i] - 1 InvResMLP blocks; nesting `encoder.<stage>.<j>`, so a reference state_dict loads
    unchanged.  group_args: the grouper's settings besides radius and nsample (the cfgs set normalize_dp)."""

    def __init__(self, in_channels=4, width=32, blocks=(1, 4, 7, 4, 4), strides=(4, 4, 4, 4), block='InvResMLP',
                 nsample=32, radius=0.1, radius_scaling=2, nsample_scaling=1, sa_layers=1, sa_use_res=False,
                 expansion=4, use_res=True, aggr_args=None, group_args=None, norm_args=None, act_args=None,
                 conv_args=None, sampler='fps', fused=False, sync_bn=False):
        super().__init__()
        if block not in ('InvResMLP', InvResMLP):
            raise NotImplementedError(f"block '{block}' is outside the hot-path build")
        self.blocks, self.strides = list(blocks), list(strides)
        self.fused, self.sync_bn = fused, sync_bn
        aggr_args = {'feature_type': 'dp_fj', 'reduction': 'max'} if aggr_args is None else dict(aggr_args)
        base = dict(_BALL if group_args is None else group_args)
        norm_args = {'norm': 'bn'} if norm_args is None else norm_args
        act_args = {'act': 'relu'} if act_args is None else act_args
        self.radii = self._to_full_list(radius, radius_scaling)
        self.nsample = self._to_full_list(nsample, nsample_scaling)
        channels = []
        for s in self.strides:
            if s != 1:
                width *= 2
            channels.append(width)
        stages, cin = [], in_channels
        for i, nblk in enumerate(self.blocks):
            is_head = i == 0 and self.strides[i] == 1
            radii, ns = self.radii[i], self.nsample[i]
            layers = [SetAbstraction(cin, channels[i], layers=sa_layers if not is_head else 1, stride=self.strides[i],
                                     group_args=dict(base, radius=radii[0], nsample=ns[0]), sampler=sampler,
                                     norm_args=norm_args, act_args=act_args, conv_args=conv_args, is_head=is_head,
                                     use_res=sa_use_res, feature_type=aggr_args['feature_type'], fused=fused,
                                     sync_bn=sync_bn)]
            cin = channels[i]
            for j in range(1, nblk):
                layers.append(InvResMLP(cin, aggr_args=aggr_args, norm_args=norm_args, act_args=act_args,
                                        group_args=dict(base, radius=radii[j], nsample=ns[j]), conv_args=conv_args,
                                        expansion=expansion, use_res=use_res, fused=fused, sync_bn=sync_bn))
            stages.append(nn.Sequential(*layers))
        self.encoder = nn.Sequential(*stages)
        self.out_channels = channels[-1]
        self.channel_list = channels

    def _to_full_list(self, param, param_scaling=1):
        """pointnext.py:389-407: one value per block of every stage, from a scalar (grown after every down-sampling
        stage, its later blocks already at the grown value) or from a (nested) list padded with its last entry."""
        full = []
        if isinstance(param, (list, tuple)):
            for i, value in enumerate(param):
                value = list(value) if isinstance(value, (list, tuple)) else [value]
                full.append(value + [value[-1]] * (self.blocks[i] - len(value)))
        else:
            for i, s in enumerate(self.strides):
                if s == 1:
                    full.append([param] * self.blocks[i])
                else:
                    full.append([param] + [param * param_scaling] * (self.blocks[i] - 1))
                    param *= param_scaling
        return full

    @torch.no_grad()
    def stage_index(self, stage, p):
        """The index work of a stage's InvResMLP blocks for its points p (B,N,3) -- coordinates only, so it belongs
        with the index pyramid: ONE ball query of p around p per distinct (radius, nsample) among the blocks and,
        where the fused kernels will consume it, ONE NeighbourIndex.  -> a list, entry j - 1 for block j."""
        from . import fused_wide, layers
        made, res = {}, []
        p = p.detach().contiguous()
        for blk in list(stage)[1:]:
            la = blk.convs
            g = la.grouper
            key = (g.radius, g.nsample)
            if key not in made:
                idx = layers.ball_query(g.radius, g.nsample, p, p)
                if la.fused and p.is_cuda and p.dtype == torch.float32 and g.nsample == 32:
                    idx = fused_wide.neighbour_index(idx, p, p.shape[1])
                made[key] = idx
            res.append(made[key])
        return res

    def _stage(self, stage, p, f):
        p, f = stage[0]([p, f])
        if len(stage) > 1:
            for blk, index in zip(list(stage)[1:], self.stage_index(stage, p)):
                p, f = blk([p, f], index=index)
        return p, f

    def forward_cls_feat(self, p0, f0=None):
        if hasattr(p0, 'keys'):
            p0, f0 = p0['pos'], p0.get('x', None)
        if f0 is None:
            f0 = p0.clone().transpose(1, 2).contiguous()
        for stage in self.encoder:
            p0, f0 = self._stage(stage, p0, f0)
        return f0.squeeze(-1)

    def forward_seg_feat(self, p0, f0=None):
        if hasattr(p0, 'keys'):
            p0, f0 = p0['pos'], p0.get('x', None)
        if f0 is None:
            f0 = p0.clone().transpose(1, 2).contiguous()
        p, f = [p0], [f0]
        for stage in self.encoder:
            _p, _f = self._stage(stage, p[-1], f[-1])
            p.append(_p)
            f.append(_f)
        return p, f

    def forward(self, p0, f0=None):
        return self.forward_seg_feat(p0, f0)


class FeaturePropagation(nn.Module):
    """PointNet++ feature propagation (`FeaturePropogation`, pointnext.py:173-226):
    features known at the coarse points p2 are carried to the dense points p1 by inverse-distance
    weighting over the three nearest coarse points (`three_nn` + `three_interpolate`, the operators of
    section 8a), concatenated with the dense level's own features and passed through Conv1d-BN-ReLU
    blocks.  `upsample=False` is the global variant (mean-pooled feature broadcast back).  Sub-module
    names (`convs.<i>.0/1`, `linear1`, `linear2`) are the reference's."""

    def __init__(self, mlp, upsample=True, norm_args=None, act_args=None, hoisted=False, fused=False):
        super().__init__()
        from .set_abstraction import convblock
        self.hoisted = hoisted     # the first block of `convs` in adaptpoint_amd.propagation's form (upsample=True only)
        self.fused = fused         # hoisted: the later blocks of `convs` on the per-point layer kernels (fixed-order sums)
        norm_args = {'norm': 'bn1d'} if norm_args is None else norm_args
        act_args = {'act': 'relu'} if act_args is None else act_args
        mlp = list(mlp)
        self.upsample = upsample
        if not upsample:
            self.linear2 = nn.Sequential(nn.Linear(mlp[0], mlp[1]), nn.ReLU(inplace=True))
            mlp[1] *= 2
            self.linear1 = nn.Sequential(*[convblock(mlp[i], mlp[i + 1], 1, norm_args=norm_args, act_args=act_args)
                                           for i in range(1, len(mlp) - 1)])
        else:
            self.convs = nn.Sequential(*[convblock(mlp[i], mlp[i + 1], 1, norm_args=norm_args, act_args=act_args)
                                         for i in range(len(mlp) - 1)])

    def forward(self, pf1, pf2=None, cond=None):
        """cond (B,Cc) or None: a per-cloud vector repeated over the dense points in FRONT of f1 (the class
        conditioning of `partseg.PointNextPartDecoder`); hoisted, it never becomes a (B,Cc,n) tensor."""
        from . import pointwise, propagation
        from .layers import three_interpolation, three_nn_weights
        if pf2 is None:
            _, f = pf1
            g = self.linear2(f.mean(dim=-1))
            return self.linear1(torch.cat((f, g.unsqueeze(-1).expand(-1, -1, f.shape[-1])), dim=1))
        (p1, f1), (p2, f2) = pf1, pf2
        parts = propagation.block_parts(self.convs[0]) if self.hoisted else None
        if parts is not None:
            nearest, weights = three_nn_weights(p1.contiguous(), p2.contiguous())
            f = propagation.propagate(None if f1 is None else f1.contiguous(), f2.contiguous(), nearest, weights, *parts,
                                      cond=None if cond is None else cond.contiguous())
            for block in list(self.convs)[1:]:
                f = pointwise.run_block(f, block, True) if self.fused else block(f)
            return f
        if cond is not None:
            rep = cond.unsqueeze(-1).expand(-1, -1, p1.shape[1])
            f1 = rep if f1 is None else torch.cat((rep, f1), dim=1)
        up = three_interpolation(p1, p2, f2)
        return self.convs(up if f1 is None else torch.cat((f1, up), dim=1))


class PointNextDecoder(nn.Module):
    """`PointNextDecoder` (pointnext.py:461-500) for decoder_layers Conv1d blocks per level: walks the
    encoder's levels from coarse to dense, one FeaturePropagation per level (`decoder.<i>.0`)."""

    def __init__(self, encoder_channel_list, decoder_layers=2, decoder_stages=4, in_channels=3, hoisted=False):
        super().__init__()
        chans = list(encoder_channel_list)
        cur = chans[-1]
        skip = chans[:-1]
        if len(skip) < decoder_stages:
            skip.insert(0, in_channels)
        fp = chans[:decoder_stages]
        stages = [None] * len(fp)
        for i in range(-1, -len(fp) - 1, -1):
            stages[i] = nn.Sequential(FeaturePropagation([skip[i] + cur] + [fp[i]] * decoder_layers, hoisted=hoisted))
            cur = fp[i]
        self.decoder = nn.Sequential(*stages)
        self.out_channels = fp[-len(fp)]

    def forward(self, p, f):
        f = list(f)
        for i in range(-1, -len(self.decoder) - 1, -1):
            f[i - 1] = self.decoder[i][0]([p[i - 1], f[i - 1]], [p[i], f[i]])
        return f[-len(self.decoder) - 1]


class ClsHead(nn.Module):
    """cls_base.py:78-136 with mlps [512, 256], BatchNorm1d, ReLU, dropout 0.5.  `act`: a callable that makes the
    hidden layers' activation (None: ReLU)."""

    def __init__(self, num_classes=15, in_channels=512, mlps=(512, 256), dropout=0.5, act=None):
        super().__init__()
        act = (lambda: nn.ReLU(inplace=True)) if act is None else act
        dims = [in_channels] + list(mlps) + [num_classes]
        heads = []
        for i in range(len(dims) - 2):
            heads.append(nn.Sequential(nn.Linear(dims[i], dims[i + 1], bias=False),
                                       nn.BatchNorm1d(dims[i + 1]), act()))
            if dropout:
                heads.append(nn.Dropout(dropout))
        heads.append(nn.Sequential(nn.Linear(dims[-2], dims[-1])))
        self.head = nn.Sequential(*heads)

    def forward(self, x):
        return self.head(x)


class SmoothCrossEntropy(nn.Module):
    """openpoints/loss/build.py:12-66 (label_smoothing > 0 branch, no ignore_index/weight)."""

    def __init__(self, label_smoothing=0.3):
        super().__init__()
        self.label_smoothing = label_smoothing

    def forward(self, pred, gt):
        n_class = pred.size(1)
        one_hot = torch.zeros_like(pred).scatter(1, gt.view(-1, 1), 1)
        one_hot = one_hot * (1 - self.label_smoothing) + (1 - one_hot) * self.label_smoothing / (n_class - 1)
        return -(one_hot * torch.log_softmax(pred, dim=1)).sum(dim=1).mean()


class PointNextSClassifier(nn.Module):
    """BaseCls for cfgs/scanobjectnn/pointnext-s.yaml (+ criterion of cfgs/scanobjectnn/default.yaml:36-38)."""

    def __init__(self, num_classes=15, fused=False, sync_bn=False):
        super().__init__()
        self.encoder = PointNextEncoderS(fused=fused, sync_bn=sync_bn)
        self.prediction = ClsHead(num_classes, self.encoder.out_channels)
        self.criterion = SmoothCrossEntropy(0.3)

    def forward(self, data, pyramid=None):
        return self.prediction(self.encoder.forward_cls_feat(data, pyramid=pyramid))

    def get_logits_loss(self, data, gt, pyramid=None):
        logits = self.forward(data, pyramid=pyramid)
        return logits, self.criterion(logits, gt.long())


def fill_parameters_by_name(model, scale=0.08):
    """Deterministic, construction-order independent weights: every tensor of the state_dict is
    drawn from a generator seeded by its NAME.  Used so that the reference model (imported in the
    build container to make goldens) and this mirror hold identical weights without shipping a
    5 MB state_dict."""
    import zlib
    sd = model.state_dict()
    with torch.no_grad():
        for name, t in sd.items():
            g = torch.Generator().manual_seed(zlib.crc32(name.encode()) & 0x7FFFFFFF)
            if name.endswith('num_batches_tracked'):
                continue
            if name.endswith('running_var'):
                v = 0.5 + torch.rand(t.shape, generator=g)
            elif name.endswith('running_mean'):
                v = 0.1 * torch.randn(t.shape, generator=g)
            elif t.dim() == 1 and name.endswith('weight'):          # norm gamma
                v = 0.75 + 0.5 * torch.rand(t.shape, generator=g)
            elif t.dim() == 1:                                        # biases
                v = 0.05 * torch.randn(t.shape, generator=g)
            else:
                fan_in = t[0].numel()
                v = torch.randn(t.shape, generator=g) * (1.0 / fan_in) ** 0.5
            t.copy_(v.to(t.dtype))
    return model
