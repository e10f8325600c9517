"""Part segmentation (ShapeNetPart): the class-conditioned PointNeXt decoder, `BasePartSeg`, its head, losses and step.

Host-side mirror of what `examples/shapenetpart/train_adapt.py` trains in the reference:

  `PointNextPartDecoder`  openpoints/models/backbone/pointnext.py:500-663, all four `cls_map`s
  `SegHead`               openpoints/models/segmentation/base_seg.py:92-149
  `BasePartSeg`           base_seg.py:15-71 (encoder `pointnext.PointNextEncoder`)
  `Poly1FocalLoss`, `SmoothCrossEntropy`, `get_class_weights`
                          openpoints/loss/build.py:12-66, 179-254, openpoints/dataset/data_util.py:185-192
  `PartSegStep`           one iteration of `train_one_epoch` (train_adapt.py:497-523) for step_per_update = 1

Classes, parameters and buffers carry the reference's names (`encoder.encoder.<i>...`, `decoder.decoder.<i>.0.convs...`,
`decoder.global_conv1.0.0.weight`, `head.head.<i>...`): a reference `state_dict` loads with strict=True.

The class conditioning.  Every `cls_map` concatenates, in front of the skip features of the LAST propagation block, a
tensor that is one vector per cloud repeated over the N points:

  'pointnet2'             relu(Wc onehot + bc)                                              (B, 64)
  'curvenet'              [max_n act(conv1 f[-2]) ; max_n act(conv2 f[-1]) ; onehot]        (B, 64 + 128 + 16)
  'pointnext'             [max_n act(conv1 f[-2]) ; max_n act(conv2 f[-1]) ; part embedding]  (B, 64 + 128 + 50)
  'pointnext1'            act(convc(part embedding))                                        (B, 64)

With hoisted=True that vector is computed as a (B,Cc) tensor -- a Linear over the one-hot / embedding row for the two
`convc` maps (torch `F.linear` with B rows, bit-reproducible: no split-K atomics in a product of this size), conv + ReLU
+ max over the points for the global maps (`pointwise.conv_max` where it applies, `pointwise.run_block` + max otherwise)
-- and goes through `propagation.propagate(..., cond=)`: neither the (B,Cc,N) repeat, nor `convc` over N identical
columns, nor the (B,Cc+C1+C2,N) concatenation exist.  hoisted=False runs the reference's composition.

Outside this module's scope: `MultiSegHead` / `MultiShapeCrossEntropy`, `part_seg_refinement` (off by default in the
reference; its result depends on the in-place, label-by-label update order), the AdaptPoint generator on ShapeNetPart
(`Form_dataset_shapenet`) and the ShapeNetPart-C file readers.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import pointwise
from .pointnext import FeaturePropagation, InvResMLP, PointNextEncoder
from .set_abstraction import convblock

# cfgs/shapenetpart/pointnext-s.yaml of the PointNeXt release (the reference's tree trains this model through
# examples/shapenetpart/train_adapt.py): BasePartSeg = PointNextEncoder + PointNextPartDecoder('curvenet') + SegHead
POINTNEXT_S_ENCODER = dict(blocks=(1, 1, 1, 1, 1), strides=(1, 2, 2, 2, 2), width=32, in_channels=7, sa_layers=3,
                           sa_use_res=True, radius=0.1, radius_scaling=2.5, nsample=32, expansion=4,
                           aggr_args={'feature_type': 'dp_fj', 'reduction': 'max'},
                           group_args={'NAME': 'ballquery', 'normalize_dp': True}, conv_args={'order': 'conv-norm-act'},
                           act_args={'act': 'relu'}, norm_args={'norm': 'bn'})
POINTNEXT_S_DECODER = dict(cls_map='curvenet')
POINTNEXT_S_HEAD = dict(global_feat='max,avg', num_classes=50, norm_args={'norm': 'bn'})


class _MaxOverPoints(torch.autograd.Function):
    """x (B,C,N) -> (B,C), the max over the points.  torch.max's backward starts from a `torch.zeros` of x's size, which
    is a memset node in a captured step (ops.zeros); this one fills by a kernel."""

    @staticmethod
    def forward(ctx, x):
        val, idx = x.max(dim=-1)
        ctx.save_for_backward(idx)
        ctx.shape = x.shape
        return val

    @staticmethod
    def backward(ctx, g):
        from .ops import zeros
        (idx,) = ctx.saved_tensors
        gx = zeros(*ctx.shape, dtype=g.dtype, device=g.device)
        return gx.scatter_(-1, idx.unsqueeze(-1), g.unsqueeze(-1))


def max_over_points(x):
    return _MaxOverPoints.apply(x)


def _one_hot_like(logits, labels):
    """F.one_hot(labels, C) moved to the channel axis and cast to the logits' dtype (build.py:223-234), made directly:
    the int64 (..., C) tensor of F.one_hot is a memset node in a captured step."""
    from .ops import zeros
    return zeros(*logits.shape, dtype=logits.dtype, device=logits.device).scatter_(1, labels.unsqueeze(1), 1.0)


def _mean(x, rows=None):
    """x.mean().  On the GPU in two stages -- over the last axis (of x viewed as (rows, -1) when `rows` is given), then
    over the row sums: torch reduces ONE output over many thousands of inputs across workgroups that meet through a
    semaphore buffer it clears with a memset, and a memset node cannot stay in a captured step (graphs.py).  The two
    stages are block-level reductions with no such buffer.  CPU tensors keep the reference's single call."""
    if not x.is_cuda or x.numel() < 4096:
        return x.mean()
    if rows is not None:
        x = x.reshape(rows, -1)
    return x.sum(dim=-1).sum() / x.numel()


def _full_list(param, scaling, strides, blocks):
    """pointnext.py:606-624: one value per block of every decoder stage."""
    full = []
    if isinstance(param, (list, tuple)):
        for i, value in enumerate(param):
            value = list(value) if isinstance(value, (list, tuple)) else [value]
            full.append(value + [value[-1]] * (blocks[i] - len(value)))
    else:
        for i, s in enumerate(strides):
            if s == 1:
                full.append([param] * blocks[i])
            else:
                full.append([param] + [param * scaling] * (blocks[i] - 1))
                param *= scaling
    return full


class PointNextPartDecoder(nn.Module):
    """pointnext.py:500-663.  `decoder.<i>` = Sequential(FeaturePropagation, decoder_blocks[i] - 1 InvResMLP blocks);
    `forward(p, f, cls_label)` with the encoder's pyramid and cls_label (B,1) integer.  cls2partembed: the (num shape
    classes, 50) table of the 'pointnext' / 'pointnext1' maps (an attribute, not a buffer, as in the reference)."""

    def __init__(self, encoder_channel_list, decoder_layers=2, decoder_blocks=(1, 1, 1, 1), decoder_strides=(4, 4, 4, 4),
                 act_args=None, cls_map='pointnet2', num_classes=16, cls2partembed=None, hoisted=False, fused=False,
                 sync_bn=False, **kwargs):
        super().__init__()
        block = kwargs.get('block', 'InvResMLP')
        if block not in ('InvResMLP', InvResMLP):
            raise NotImplementedError(f"block '{block}' is outside the hot-path build")
        if cls_map not in ('curvenet', 'pointnet2', 'pointnext', 'pointnext1'):
            raise ValueError(f"PointNextPartDecoder: unknown cls_map '{cls_map}'")
        act_args = {'act': 'relu'} if act_args is None else act_args
        self.decoder_layers, self.hoisted, self.fused = decoder_layers, hoisted, fused
        chans = list(encoder_channel_list)
        self.in_channels = chans[-1]
        skip, fp = chans[:-1], chans[:-1]
        self.blocks, self.strides = list(decoder_blocks), list(decoder_strides)
        self.norm_args = kwargs.get('norm_args') or {'norm': 'bn'}
        self.act_args = act_args
        self.radii = _full_list(kwargs.get('radius', 0.1), kwargs.get('radius_scaling', 2), self.strides, self.blocks)
        self.nsample = _full_list(kwargs.get('nsample', 16), kwargs.get('nsample_scaling', 1), self.strides, self.blocks)
        self.cls_map, self.num_classes = cls_map, num_classes
        group_args = dict(kwargs.get('group_args') or {'NAME': 'ballquery'})
        aggr_args = kwargs.get('aggr_args') or {'feature_type': 'dp_fj', 'reduction': 'max'}
        wide = lambda cin, cout: nn.Sequential(convblock(cin, cout, 1, norm_args=None, act_args=act_args))
        if cls_map in ('curvenet', 'pointnext'):
            self.global_conv2 = wide(fp[-1] * 2, 128)
            self.global_conv1 = wide(fp[-2] * 2, 64)
            self.cond_channels = 64 + 128 + (16 if cls_map == 'curvenet' else 50)
        else:
            self.convc = wide(16 if cls_map == 'pointnet2' else 50, 64)
            self.cond_channels = 64
        if cls_map in ('pointnext', 'pointnext1'):
            self.cls2partembed = cls2partembed
        skip[0] += self.cond_channels
        n = len(fp)
        decoder = [None] * n
        cur = self.in_channels
        for i in range(-1, -n - 1, -1):
            layers = [FeaturePropagation([skip[i] + cur] + [fp[i]] * decoder_layers, act_args=act_args, hoisted=hoisted,
                                         fused=fused)]
            cur = fp[i]
            for j in range(1, self.blocks[i]):
                layers.append(InvResMLP(cur, aggr_args=aggr_args, norm_args=self.norm_args, act_args=act_args,
                                        group_args=dict(group_args, radius=self.radii[i][j], nsample=self.nsample[i][j]),
                                        conv_args=kwargs.get('conv_args'), expansion=kwargs.get('expansion', 4),
                                        use_res=kwargs.get('use_res', True), fused=fused, sync_bn=sync_bn))
            decoder[i] = nn.Sequential(*layers)
        self.decoder = nn.Sequential(*decoder)
        self.out_channels = fp[-n]

    # ------------------------------------------------------------------------------------- the conditioning vector
    def _one_hot(self, cls_label, like):
        B = cls_label.shape[0]
        return torch.zeros((B, self.num_classes), device=like.device, dtype=like.dtype).scatter_(1, cls_label, 1)

    def _embedding(self, cls_label, like):
        if self.cls2partembed is None:
            raise ValueError(f"PointNextPartDecoder(cls_map='{self.cls_map}') needs cls2partembed")
        self.cls2partembed = self.cls2partembed.to(like.device)
        return self.cls2partembed[cls_label.reshape(-1)]

    def _global_max(self, block, f):
        """(B, O) = max over the points of act(conv f): `block` = Sequential(Sequential(Conv1d with bias, ReLU))."""
        mods = list(block[0])
        conv = mods[0]
        relu = len(mods) == 2 and isinstance(mods[1], nn.ReLU)
        if self.fused and relu and pointwise.conv_max_supported(f, conv.in_channels):
            return pointwise.conv_max(f.contiguous(), conv.weight, conv.bias, relu=True)
        return max_over_points(pointwise.run_block(f, block[0], self.fused))

    def conditioning(self, f, cls_label):
        """The per-cloud vector (B, cond_channels) that the reference repeats over the N points."""
        if self.cls_map in ('curvenet', 'pointnext'):
            last = (self._one_hot(cls_label, f[-1]) if self.cls_map == 'curvenet'
                    else self._embedding(cls_label, f[-1]).to(f[-1].dtype))
            return torch.cat((self._global_max(self.global_conv1, f[-2]), self._global_max(self.global_conv2, f[-1]), last),
                             dim=1)
        row = (self._one_hot(cls_label, f[-1]) if self.cls_map == 'pointnet2'
               else self._embedding(cls_label, f[-1]).to(f[-1].dtype))
        mods = list(self.convc[0])
        conv = mods[0]
        out = F.linear(row, conv.weight.reshape(conv.out_channels, conv.in_channels), conv.bias)
        for act in mods[1:]:
            out = act(out)
        return out

    def _conditioning_composed(self, f, cls_label, N):
        """pointnext.py:628-653, statement for statement: the (B, cond_channels, N) tensor."""
        if self.cls_map in ('curvenet', 'pointnext'):
            emb1 = self.global_conv1(f[-2]).max(dim=-1, keepdim=True)[0]
            emb2 = self.global_conv2(f[-1]).max(dim=-1, keepdim=True)[0]
            last = (self._one_hot(cls_label, f[-1]) if self.cls_map == 'curvenet'
                    else self._embedding(cls_label, f[-1])).unsqueeze(-1)
            return torch.cat((emb1, emb2, last), dim=1).expand(-1, -1, N)
        if self.cls_map == 'pointnet2':
            return self.convc(self._one_hot(cls_label, f[-1]).unsqueeze(-1).repeat(1, 1, N))
        return self.convc(self._embedding(cls_label, f[-1]).unsqueeze(-1).expand(-1, -1, N))

    def _tail(self, stage, p, f):
        """The stage's InvResMLP blocks behind its propagation block, on one ball query per (radius, nsample)."""
        blocks = list(stage)[1:]
        if blocks:
            for blk, index in zip(blocks, PointNextEncoder.stage_index(None, stage, p)):
                p, f = blk([p, f], index=index)
        return f

    def forward(self, p, f, cls_label):
        f = list(f)
        N = p[0].shape[1]
        cls_label = cls_label.reshape(-1, 1).long()
        # (from the ENCODER's f[-2] and f[-1]: the loop below replaces f[-2])
        cond = self.conditioning(f, cls_label) if self.hoisted else self._conditioning_composed(f, cls_label, N)
        for i in range(-1, -len(self.decoder), -1):
            f[i - 1] = self._tail(self.decoder[i], p[i - 1], self.decoder[i][0]([p[i - 1], f[i - 1]], [p[i], f[i]]))
        first = self.decoder[0]
        if self.hoisted:
            out = first[0]([p[1], f[1]], [p[2], f[2]], cond=cond)
        else:
            out = first[0]([p[1], torch.cat([cond, f[1]], 1)], [p[2], f[2]])
        f[-len(self.decoder) - 1] = self._tail(first, p[1], out)
        return f[-len(self.decoder) - 1]


class SegHead(nn.Module):
    """base_seg.py:92-149: optional global max / avg features repeated over the points, Conv1d-BN-ReLU blocks with
    dropout, a final Conv1d with bias.  -> logits (B, num_classes, N)."""

    def __init__(self, num_classes, in_channels, mlps=None, norm_args=None, act_args=None, dropout=0.5, global_feat=None,
                 fused=False):
        super().__init__()
        norm_args = {'norm': 'bn1d'} if norm_args is None else norm_args
        act_args = {'act': 'relu'} if act_args is None else act_args
        self.global_feat = global_feat.split(',') if global_feat is not None else None
        self.fused = fused
        in_channels *= 1 if self.global_feat is None else len(self.global_feat) + 1
        if mlps is None:
            mlps = [in_channels, in_channels] + [num_classes]
        else:
            mlps = [in_channels] + (list(mlps) if isinstance(mlps, (list, tuple)) else [mlps]) + [num_classes]
        heads = []
        for i in range(len(mlps) - 2):
            heads.append(convblock(mlps[i], mlps[i + 1], 1, norm_args=norm_args, act_args=act_args))
            if dropout:
                heads.append(nn.Dropout(dropout))
        heads.append(convblock(mlps[-2], mlps[-1], 1, act_args=None))
        self.head = nn.Sequential(*heads)

    def forward(self, end_points):
        if self.global_feat is not None:
            feats = []
            for kind in self.global_feat:
                if 'max' in kind:
                    feats.append(max_over_points(end_points).unsqueeze(-1))
                elif kind in ('avg', 'mean'):
                    feats.append(torch.mean(end_points, dim=-1, keepdim=True))
            feats = torch.cat(feats, dim=1).expand(-1, -1, end_points.shape[-1])
            end_points = torch.cat((end_points, feats), dim=1)
        x = end_points
        for mod in self.head:
            x = pointwise.run_block(x.contiguous(), mod, self.fused) if isinstance(mod, nn.Sequential) else mod(x)
        return x


class BasePartSeg(nn.Module):
    """base_seg.py:54-71 over `PointNextEncoder`, `PointNextPartDecoder` and `SegHead`; the decoder's arguments are the
    encoder's updated by `decoder_args`, as `BaseSeg.__init__` merges them.  Defaults: PointNeXt-S for ShapeNetPart.
    fused: the encoder's and decoder's blocks on the fused kernels; hoisted: every propagation block in
    `adaptpoint_amd.propagation`'s form, the last one with the class conditioning as its `cond`."""

    def __init__(self, encoder_args=None, decoder_args=None, cls_args=None, fused=False, hoisted=False, sync_bn=False):
        super().__init__()
        encoder_args = dict(POINTNEXT_S_ENCODER if encoder_args is None else encoder_args)
        decoder_args = dict(POINTNEXT_S_DECODER if decoder_args is None else decoder_args)
        cls_args = dict(POINTNEXT_S_HEAD if cls_args is None else cls_args)
        for d in (encoder_args, decoder_args, cls_args):
            d.pop('NAME', None)
        self.encoder = PointNextEncoder(fused=fused, sync_bn=sync_bn, **encoder_args)
        merged = dict(encoder_args)
        merged.update(decoder_args)
        for k in ('in_channels', 'width', 'blocks', 'strides', 'sa_layers', 'sa_use_res', 'sampler'):
            merged.pop(k, None)
        self.decoder = PointNextPartDecoder(self.encoder.channel_list, hoisted=hoisted, fused=fused, sync_bn=sync_bn,
                                            **merged)
        cls_args['in_channels'] = self.decoder.out_channels
        self.head = SegHead(fused=fused, **cls_args)

    def forward(self, p0, f0=None, cls0=None):
        if hasattr(p0, 'keys'):
            p0, f0, cls0 = p0['pos'], p0['x'], p0['cls']
        elif f0 is None:
            f0 = p0.transpose(1, 2).contiguous()
        p, f = self.encoder.forward_seg_feat(p0, f0)
        return self.head(self.decoder(p, f, cls0))


# ------------------------------------------------------------------------------------------------------------ losses
class SmoothCrossEntropy(nn.Module):
    """openpoints/loss/build.py:12-66 without ignore_index: (B, C, N) logits are flattened to (B N, C) by
    transpose(1, 2).reshape, labels by view(-1); weight: per-class weights (C,), multiplied into the smoothed terms."""

    def __init__(self, label_smoothing=0.2, weight=None):
        super().__init__()
        self.label_smoothing = label_smoothing
        if weight is not None:
            weight = torch.as_tensor(np.asarray(weight) if not torch.is_tensor(weight) else weight).float().squeeze()
        self.register_buffer('weight', weight, persistent=False)

    def forward(self, pred, gt):
        rows = pred.shape[0] if pred.dim() > 2 else None
        if pred.dim() > 2:
            pred = pred.transpose(1, 2).reshape(-1, pred.shape[1])
        gt = gt.contiguous().view(-1)
        if self.label_smoothing > 0:
            n_class = pred.size(1)
            one_hot = torch.zeros_like(pred).scatter(1, gt.view(-1, 1), 1)
            one_hot = one_hot * (1 - self.label_smoothing) + (1 - one_hot) * self.label_smoothing / (n_class - 1)
            log_prb = F.log_softmax(pred, dim=1)
            if self.weight is not None:
                return _mean(-(one_hot * log_prb * self.weight).sum(dim=1), rows)
            return _mean(-(one_hot * log_prb).sum(dim=1), rows)
        return F.cross_entropy(pred, gt, weight=self.weight)


class Poly1FocalLoss(nn.Module):
    """openpoints/loss/build.py:179-254: sigmoid focal loss plus epsilon (1 - pt)^(gamma + 1), on logits (N, C) or
    (B, C, ...) with integer labels (N,) / (B, ...) (or one-hot ones with label_is_onehot)."""

    def __init__(self, epsilon=1.0, alpha=0.25, gamma=2.0, reduction="mean", weight=None, pos_weight=None,
                 label_is_onehot=False):
        super().__init__()
        self.epsilon, self.alpha, self.gamma, self.reduction = epsilon, alpha, gamma, reduction
        self.weight, self.pos_weight, self.label_is_onehot = weight, pos_weight, label_is_onehot

    def forward(self, logits, labels):
        p = torch.sigmoid(logits)
        if not self.label_is_onehot:
            labels = _one_hot_like(logits, labels.to(logits.device))
        labels = labels.to(device=logits.device, dtype=logits.dtype)
        ce_loss = F.binary_cross_entropy_with_logits(input=logits, target=labels, reduction="none", weight=self.weight,
                                                     pos_weight=self.pos_weight)
        pt = labels * p + (1 - labels) * (1 - p)
        FL = ce_loss * ((1 - pt) ** self.gamma)
        if self.alpha >= 0:
            alpha_t = self.alpha * labels + (1 - self.alpha) * (1 - labels)
            FL = alpha_t * FL
        poly1 = FL + self.epsilon * torch.pow(1 - pt, self.gamma + 1)
        if self.reduction == "mean":
            poly1 = _mean(poly1)
        elif self.reduction == "sum":
            poly1 = poly1.sum()
        return poly1


def get_class_weights(num_per_class, normalize=False):
    """openpoints/dataset/data_util.py:185-192."""
    num_per_class = np.asarray(num_per_class)
    weight = num_per_class / float(sum(num_per_class))
    ce_label_weight = 1 / (weight + 0.02)
    if normalize:
        ce_label_weight = (ce_label_weight * len(ce_label_weight)) / ce_label_weight.sum()
    return torch.from_numpy(ce_label_weight.astype(np.float32))


class PartSegStep:
    """One iteration of `train_one_epoch` (train_adapt.py:497-523) for step_per_update = 1: forward, loss, backward,
    gradient-norm clipping, AdamW, zero_grad.  data = {'pos' (B,N,3), 'x' (B,C,N), 'y' (B,N), 'cls' (B,1)} on the device.
    optimizer= / grad_sync= as `gan.ClassifierStep` takes them; with a capturable optimizer the step holds no host read
    and can be captured through `graphs.capture`."""

    def __init__(self, model, criterion=None, lr=1e-3, weight_decay=1e-4, grad_norm_clip=1.0, optimizer=None,
                 grad_sync=None):
        self.model = model
        self.criterion = Poly1FocalLoss() if criterion is None else criterion
        self.grad_sync, self.clip = grad_sync, grad_norm_clip
        self.opt = optimizer or torch.optim.AdamW(model.parameters(), lr=lr, weight_decay=weight_decay)

    def __call__(self, data):
        """-> (logits, loss), both detached (see `gan.ClassifierStep.__call__` on why)."""
        self.model.train()
        logits = self.model({'pos': data['pos'], 'x': data['x'], 'cls': data['cls']})
        loss = self.criterion(logits, data['y'].long())
        loss.backward()
        if self.grad_sync is not None:
            self.grad_sync([q.grad for q in self.model.parameters() if q.grad is not None])
        if self.clip is not None and self.clip > 0:
            nn.utils.clip_grad_norm_(self.model.parameters(), self.clip, norm_type=2)
        self.opt.step()
        self.model.zero_grad()
        return logits.detach(), loss.detach()


__all__ = ["PointNextPartDecoder", "SegHead", "BasePartSeg", "SmoothCrossEntropy", "Poly1FocalLoss", "get_class_weights",
           "PartSegStep", "POINTNEXT_S_ENCODER", "POINTNEXT_S_DECODER", "POINTNEXT_S_HEAD"]
