"""PointViT (openpoints/models/backbone/pointvit.py: the Pix4Point / Point-MAE encoder) over this build's operators.

Class, argument and parameter names are the reference's (`patch_embed.conv1.<i>.<j>.*`, `cls_token`, `cls_pos`,
`pos_embed.0.0.*`, `pos_embed.1.*`, `blocks.<i>.{norm1,attn.qkv,attn.proj,norm2,mlp.fc1,mlp.fc2}.*`, `norm.*`): a reference
`state_dict` loads unchanged.  What differs:

  * `Attention(fused=True)` (the default) hands the packed output of `qkv` to `token_attention.token_attention`
    (csrc/token_attention.hip: head dim 64, any token count, no (B,H,T,T) tensor) and its result to `proj`; `fused=False`
    is the reference's composition.  CPU tensors, other head dims and attention dropout in training run the composition
    too, counted by reason in `token_attention.COMPOSED_CALLS`.  LayerNorm, GELU, the residual adds, DropPath, dropout
    and the linear layers are PyTorch; on the GPU a biased linear layer over token rows takes its bias gradient from a
    matrix product (`_LinearRows`), so that a training step captures without a memset node.
  * `PointPatchEmbed` samples and groups with `layers.furthest_point_sample`, `layers.knn_query` / `layers.ball_query`,
    `layers.grouping_operation` and `layers.gather_operation`; its norms and activations are PyTorch, its 1x1
    convolutions PyTorch matrix products (`Conv1x1`: bit-reproducible weight gradients).
    `PointPatchEmbed.index(p)` returns the (sample, neighbour) index pair, a function of the coordinates alone, and
    `forward(..., index=)` takes it.  On the GPU the neighbours are `knn_query`'s (squared direct differences, ties to the
    smaller index); on CPU tensors the reference's own call (`torch.cdist`, `topk` over the support axis).  The two can
    differ at near-ties; the pooled result is independent of the order inside a neighbourhood.
  * `embed_args`, `norm_args` and `act_args` may be plain dicts.
"""
import copy

import torch
import torch.nn as nn

from . import layers
from . import token_attention as _ta
from .pointnext import ClsHead, SmoothCrossEntropy

_NORMS = dict(bn1d=nn.BatchNorm1d, bn2d=nn.BatchNorm2d, bn=nn.BatchNorm2d, in2d=nn.InstanceNorm2d, in1d=nn.InstanceNorm1d,
              gn=nn.GroupNorm, ln=nn.LayerNorm)
_ACTS = dict(relu=nn.ReLU, gelu=nn.GELU, silu=nn.SiLU, swish=nn.SiLU, leakyrelu=nn.LeakyReLU, leaky_relu=nn.LeakyReLU,
             elu=nn.ELU, selu=nn.SELU, sigmoid=nn.Sigmoid, tanh=nn.Tanh)
CHANNEL_MAP = {'fj': lambda c: c, 'df': lambda c: c, 'dp': lambda c: 3, 'dp_fj': lambda c: 3 + c, 'dp_df': lambda c: 3 + c}


def create_norm(norm_args, channels, dimension=None):
    """The reference's norm factory for the names PointViT uses ({'norm': name, **kwargs} or a name)."""
    if norm_args is None:
        return None
    kw = dict(norm_args) if hasattr(norm_args, 'keys') else {'norm': norm_args}
    name = kw.pop('norm', None)
    if name is None:
        return None
    name = name.lower()
    if dimension is not None and str(dimension).lower() not in name:
        name += str(dimension).lower()
    if name not in _NORMS:
        raise NotImplementedError(f"norm {name} is not supported")
    return _NORMS[name](channels, **kw)


def create_act(act_args):
    if act_args is None:
        return None
    kw = dict(act_args) if hasattr(act_args, 'keys') else {'act': act_args}
    name = kw.pop('act', None)
    if name is None:
        return None
    name = name.lower()
    if name not in _ACTS:
        raise NotImplementedError(f"activation {name} is not supported")
    inplace = kw.pop('inplace', True)
    if name in ('gelu', 'sigmoid', 'tanh'):
        return _ACTS[name](**kw)
    return _ACTS[name](inplace=inplace, **kw)


class Conv1x1(nn.Conv2d):
    """A 1x1 Conv2d (the reference's module: same parameters, same names) computed as one matrix product over the
    channel axis.  The convolution library's weight-gradient kernels for these shapes add with float atomics -- two
    training steps from the same state then differ in bits, and so do two replays of a captured step; the GEMM does not.
    On the GPU only."""

    def __init__(self, cin, cout, bias=True):
        super().__init__(cin, cout, 1, bias=bias)

    def forward(self, x):
        if not x.is_cuda:                       # the mirror on CPU tensors: the reference's own call
            return super().forward(x)
        x = x.permute(0, 2, 3, 1)
        w = self.weight.view(self.out_channels, self.in_channels)
        if self.bias is not None and torch.is_grad_enabled():
            y = _LinearRows.apply(x, w, self.bias)               # (its bias gradient without a memset node)
        else:
            y = torch.nn.functional.linear(x, w, self.bias)
        return y.permute(0, 3, 1, 2)


def create_convblock2d(cin, cout, norm_args=None, act_args=None, order='conv-norm-act', bias=True):
    """1x1 Conv2d [+ norm] [+ act] in the reference's slot order (conv.py:24-62, 'conv-norm-act')."""
    if order != 'conv-norm-act':
        raise NotImplementedError(f"{order} is not supported")
    norm = create_norm(norm_args, cout, dimension='2d')
    mods = [Conv1x1(cin, cout, bias=bias and norm is None)]
    if norm is not None:
        mods.append(norm)
    if act_args is not None:
        mods.append(create_act(act_args))
    return nn.Sequential(*mods)


def create_linearblock(cin, cout, norm_args=None, act_args=None):
    norm = create_norm(norm_args, cout, dimension='1d')
    mods = [nn.Linear(cin, cout, bias=norm is None)]
    if norm is not None:
        mods.append(norm)
    if act_args is not None:
        mods.append(create_act(act_args))
    return nn.Sequential(*mods)


class _LinearRows(torch.autograd.Function):
    """`F.linear` with a bias, whose bias gradient is a matrix product with a row of ones.  PyTorch's own is a column sum
    over the B T rows: from a few thousand rows on a multi-block reduction whose semaphore buffer is zeroed by a MEMSET
    before every launch -- a node `graphs.capture` refuses (it replays correctly once).  Same forward, same dx and dW."""

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        return torch.nn.functional.linear(x, w, b)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        g2, x2 = g.reshape(-1, g.shape[-1]), x.reshape(-1, x.shape[-1])
        dx = (g2 @ w).view(x.shape) if ctx.needs_input_grad[0] else None
        return dx, g2.t() @ x2, (g2.new_ones(1, g2.shape[0]) @ g2).view(-1)


def linear(x, lin):
    """`lin(x)` for an nn.Linear over token rows; on the GPU with a bias under autograd: `_LinearRows`."""
    if (x.is_cuda and lin.bias is not None and torch.is_grad_enabled() and x.dtype == torch.float32
            and not (lin._forward_hooks or lin._forward_pre_hooks)):
        return _LinearRows.apply(x, lin.weight, lin.bias)
    return lin(x)


def _through(x, seq):
    """A Sequential of linear blocks, its nn.Linear members through `linear`."""
    for m in seq:
        x = _through(x, m) if isinstance(m, nn.Sequential) else linear(x, m) if isinstance(m, nn.Linear) else m(x)
    return x


class DropPath(nn.Module):
    """Stochastic depth per sample: one Bernoulli(keep) draw per cloud from the tensor's generator, scaled by 1 / keep."""

    def __init__(self, drop_prob=0.0, scale_by_keep=True):
        super().__init__()
        self.drop_prob, self.scale_by_keep = drop_prob, scale_by_keep

    def forward(self, x):
        if self.drop_prob == 0.0 or not self.training:
            return x
        keep = 1 - self.drop_prob
        mask = x.new_empty((x.shape[0],) + (1,) * (x.ndim - 1)).bernoulli_(keep)
        if keep > 0.0 and self.scale_by_keep:
            mask.div_(keep)
        return x * mask


class Attention(nn.Module):
    """layers/attention.py:12-38.  fused: None (= True) / True: the head-dim-64 kernel wherever it applies."""

    def __init__(self, dim, num_heads=8, qkv_bias=False, attn_drop=0., proj_drop=0., fused=None):
        super().__init__()
        self.num_heads = num_heads
        self.scale = (dim // num_heads) ** -0.5
        self.fused = fused
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.attn_drop = nn.Dropout(attn_drop)
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(proj_drop)

    def forward(self, x):
        qkv = self.qkv(x)
        if self.fused is False:
            x = _ta.composed(qkv, self.num_heads, self.attn_drop)
        elif self.training and self.attn_drop.p > 0:
            x = _ta.fallback(qkv, self.num_heads, "attention dropout %g in training" % self.attn_drop.p, self.attn_drop)
        else:
            x = _ta.token_attention(qkv, self.num_heads)
        return self.proj_drop(linear(x, self.proj))


class Mlp(nn.Module):
    """layers/mlp.py:11-35."""

    def __init__(self, in_features, hidden_features=None, out_features=None, act_args={'act': 'gelu'}, norm_args=None,
                 drop=0.):
        super().__init__()
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features
        drops = drop if isinstance(drop, (tuple, list)) else (drop, drop)
        self.fc1 = nn.Linear(in_features, hidden_features)
        self.act = create_act(act_args)
        self.drop1 = nn.Dropout(drops[0])
        self.fc2 = nn.Linear(hidden_features, out_features)
        self.drop2 = nn.Dropout(drops[1])

    def forward(self, x):
        return self.drop2(linear(self.drop1(self.act(linear(x, self.fc1))), self.fc2))


class Block(nn.Module):
    """layers/attention.py:41-58."""

    def __init__(self, dim, num_heads, mlp_ratio=4., qkv_bias=False, drop=0., attn_drop=0., drop_path=0.,
                 act_args={'act': 'gelu'}, norm_args={'norm': 'ln'}, fused=None):
        super().__init__()
        self.norm1 = create_norm(norm_args, dim)
        self.attn = Attention(dim, num_heads=num_heads, qkv_bias=qkv_bias, attn_drop=attn_drop, proj_drop=drop, fused=fused)
        self.drop_path = DropPath(drop_path) if drop_path > 0. else nn.Identity()
        self.norm2 = create_norm(norm_args, dim)
        self.mlp = Mlp(in_features=dim, hidden_features=int(dim * mlp_ratio), act_args=act_args, drop=drop)

    def forward(self, x):
        x = x + self.drop_path(self.attn(self.norm1(x)))
        return x + self.drop_path(self.mlp(self.norm2(x)))


class TransformerEncoder(nn.Module):
    """layers/attention.py:61-103: the blocks with the position embedding added in front of each."""

    def __init__(self, embed_dim=768, depth=12, num_heads=12, mlp_ratio=4., qkv_bias=False, drop_rate=0.,
                 attn_drop_rate=0., drop_path_rate=0., act_args={'act': 'gelu'}, norm_args={'norm': 'ln'}, fused=None):
        super().__init__()
        self.blocks = nn.ModuleList([
            Block(dim=embed_dim, num_heads=num_heads, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, drop=drop_rate,
                  attn_drop=attn_drop_rate,
                  drop_path=drop_path_rate[i] if isinstance(drop_path_rate, list) else drop_path_rate,
                  norm_args=norm_args, act_args=act_args, fused=fused)
            for i in range(depth)])
        self.depth = depth

    def forward(self, x, pos):
        for block in self.blocks:
            x = block(x + pos)
        return x

    def forward_features(self, x, pos, num_outs=None):
        dilation = self.depth // num_outs
        out_depth = list(range(self.depth))[(self.depth - (num_outs - 1) * dilation - 1)::dilation]
        out = []
        for i, block in enumerate(self.blocks):
            x = block(x + pos)
            if i in out_depth:
                out.append(x)
        return out


def _take(features, idx):
    """features (B,C,N), idx (B,M[,K]) int32 -> (B,C,M[,K]): the library's copy kernels on the GPU, torch.gather on CPU."""
    if features.is_cuda:
        features = features.contiguous()
        return layers.gather_operation(features, idx) if idx.dim() == 2 else layers.grouping_operation(features, idx)
    B, C, _ = features.shape
    flat = idx.reshape(B, 1, -1).expand(-1, C, -1).long()
    return torch.gather(features, 2, flat).reshape(B, C, *idx.shape[1:])


class PointPatchEmbed(nn.Module):
    """layers/group_embed.py:58-172: sample, group, two stacks of 1x1 convolutions around a pooled-context concat."""

    def __init__(self, sample_ratio=0.0625, group_size=32, in_channels=3, layers=4, embed_dim=256, channels=None,
                 subsample='fps', group='ballquery', normalize_dp=False, radius=0.1, feature_type='dp_df',
                 relative_xyz=True, norm_args={'norm': 'bn1d'}, act_args={'act': 'relu'},
                 conv_args={'order': 'conv-norm-act'}, reduction='max', **kwargs):
        super().__init__()
        if subsample.lower() != 'fps':
            raise NotImplementedError(f"subsample {subsample}: only fps is built")
        if feature_type not in CHANNEL_MAP:
            raise NotImplementedError(f"feature_type {feature_type} is not supported")
        self.sample_ratio, self.group_size, self.feature_type = sample_ratio, group_size, feature_type
        self.group = group.lower()
        if not ('ball' in self.group or 'query' in self.group or 'knn' in self.group):
            raise NotImplementedError(f'{self.group} is not implemented. Only support ballquery, knn')
        self.knn = not ('ball' in self.group or 'query' in self.group)
        self.radius, self.relative_xyz, self.normalize_dp = radius, relative_xyz, normalize_dp
        if channels is None:
            channels = ([CHANNEL_MAP[feature_type](in_channels)] + [embed_dim] * (layers // 2)
                        + [embed_dim * 2] * (layers // 2 - 1) + [embed_dim])
        else:
            channels = [CHANNEL_MAP[feature_type](in_channels)] + list(channels) + [embed_dim]
            layers = len(channels) - 1
        conv_args = dict(conv_args)
        half = layers // 2
        self.conv1 = nn.Sequential(*[
            create_convblock2d(channels[i], channels[i + 1], norm_args=norm_args if i != half - 1 else None,
                               act_args=act_args if i != half - 1 else None, **conv_args) for i in range(half)])
        channels[half] *= 2
        self.conv2 = nn.Sequential(*[
            create_convblock2d(channels[i], channels[i + 1], norm_args=norm_args if i != layers - 1 else None,
                               act_args=act_args if i != layers - 1 else None, **conv_args) for i in range(half, layers)])
        self.mean_pool = reduction in ['mean', 'avg', 'meanpool', 'avgpool']
        self.out_channels = channels[-1]
        self.channel_list = [in_channels, embed_dim]

    def pool(self, x):
        return torch.mean(x, dim=-1, keepdim=True) if self.mean_pool else torch.max(x, dim=-1, keepdim=True)[0]

    @torch.no_grad()
    def index(self, p):
        """p (B,N,3) -> (sample (B,S) int32, neighbours (B,S,K) int32), a function of the coordinates alone."""
        p = p.detach().contiguous()
        idx = layers.furthest_point_sample(p, int(p.shape[1] * self.sample_ratio))
        center = torch.gather(p, 1, idx.long().unsqueeze(-1).expand(-1, -1, 3)).contiguous()
        if not self.knn:
            return idx, layers.ball_query(self.radius, self.group_size, p, center)
        if layers.knn_covers(p, center, self.group_size):
            return idx, layers.knn_query(p, center, self.group_size)
        # the reference's own call (group.py:26-28): Euclidean distances, topk over the support axis
        nbr = torch.cdist(p, center).topk(k=self.group_size, dim=1, largest=False).indices
        return idx, nbr.transpose(1, 2).contiguous().int()

    def forward(self, p, x=None, index=None):
        idx, nbr = self.index(p) if index is None else index
        center_p = torch.gather(p, 1, idx.long().unsqueeze(-1).expand(-1, -1, 3))
        dp = _take(p.transpose(1, 2), nbr)                                   # (B,3,S,K)
        if self.relative_xyz:
            dp = dp - center_p.transpose(1, 2).unsqueeze(-1)
            if self.normalize_dp and not self.knn:
                dp = dp / self.radius
        if self.normalize_dp and self.knn:
            dp = dp / torch.amax(torch.sqrt(torch.sum(dp ** 2, dim=1)), dim=(1, 2)).view(-1, 1, 1, 1)
        fj = _take(x, nbr) if x is not None else None
        if self.feature_type == 'dp':
            fj = dp
        elif self.feature_type == 'dp_fj':
            fj = torch.cat([dp, fj], dim=1)
        elif self.feature_type in ('dp_df', 'df'):
            df = fj - _take(x, idx).unsqueeze(-1)
            fj = torch.cat([dp, df], dim=1) if self.feature_type == 'dp_df' else df
        fj = self.conv1(fj)
        fj = torch.cat([self.pool(fj).expand(-1, -1, -1, self.group_size), fj], dim=1)
        out_f = self.pool(self.conv2(fj)).squeeze(-1)
        return [p, center_p], [x, out_f]


DEFAULT_EMBED_ARGS = {'NAME': 'PointPatchEmbed', 'num_groups': 256, 'group_size': 32, 'subsample': 'fps', 'group': 'knn',
                      'feature_type': 'fj', 'norm_args': {'norm': 'in2d'}}


class PointViT(nn.Module):
    """backbone/pointvit.py:17-173."""

    def __init__(self, in_channels=3, embed_dim=384, depth=12, num_heads=6, mlp_ratio=4., qkv_bias=False, drop_rate=0.,
                 attn_drop_rate=0., drop_path_rate=0., embed_args=None, norm_args={'norm': 'ln', 'eps': 1.0e-6},
                 act_args={'act': 'gelu'}, add_pos_each_block=True, global_feat='cls,max', distill=False, fused=None,
                 **kwargs):
        super().__init__()
        self.num_features = self.embed_dim = embed_dim
        embed_args = copy.deepcopy(dict(DEFAULT_EMBED_ARGS if embed_args is None else embed_args))
        name = embed_args.pop('NAME', 'PointPatchEmbed')
        if name != 'PointPatchEmbed':
            raise NotImplementedError(f"embed_args NAME {name}: only PointPatchEmbed is built")
        embed_args['in_channels'], embed_args['embed_dim'] = in_channels, embed_dim
        self.patch_embed = PointPatchEmbed(**embed_args)
        self.cls_token = nn.Parameter(torch.randn(1, 1, embed_dim))
        self.cls_pos = nn.Parameter(torch.randn(1, 1, embed_dim))
        self.pos_embed = nn.Sequential(create_linearblock(3, 128, norm_args=None, act_args=act_args),
                                       nn.Linear(128, embed_dim))
        if self.patch_embed.out_channels != embed_dim:
            self.proj = nn.Linear(self.patch_embed.out_channels, embed_dim)
        else:
            self.proj = nn.Identity()
        self.add_pos_each_block = add_pos_each_block
        self.pos_drop = nn.Dropout(p=drop_rate)
        dpr = [x.item() for x in torch.linspace(0, drop_path_rate, depth)]
        self.depth = depth
        self.blocks = nn.ModuleList([
            Block(dim=embed_dim, num_heads=num_heads, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, drop=drop_rate,
                  attn_drop=attn_drop_rate, drop_path=dpr[i], norm_args=norm_args, act_args=act_args, fused=fused)
            for i in range(depth)])
        self.norm = create_norm(norm_args, embed_dim)
        self.global_feat = global_feat.split(',')
        self.out_channels = len(self.global_feat) * embed_dim
        self.distill_channels = embed_dim
        self.channel_list = self.patch_embed.channel_list
        self.channel_list[-1] = embed_dim
        if distill:
            self.dist_token = nn.Parameter(torch.randn(1, 1, embed_dim))
            self.dist_pos = nn.Parameter(torch.randn(1, 1, embed_dim))
            self.n_tokens = 2
        else:
            self.dist_token = None
            self.n_tokens = 1
        self.initialize_weights()

    def initialize_weights(self):
        for t in (self.cls_token, self.cls_pos) + ((self.dist_token, self.dist_pos) if self.dist_token is not None else ()):
            nn.init.normal_(t, std=.02)
        self.apply(self._init_weights)

    @staticmethod
    def _init_weights(m):
        if isinstance(m, nn.Linear):
            nn.init.xavier_uniform_(m.weight)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, (nn.LayerNorm, nn.GroupNorm, nn.BatchNorm2d, nn.BatchNorm1d)):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)

    @torch.jit.ignore
    def no_weight_decay(self):
        return {'cls_token', 'dist_token', 'dist_token'}

    def get_num_layers(self):
        return self.depth

    def set_fused(self, fused):
        for block in self.blocks:
            block.attn.fused = fused
        return self

    def forward(self, p, x=None, index=None):
        if hasattr(p, 'keys'):
            p, x = p['pos'], p['x'] if 'x' in p.keys() else None
        if x is None:
            x = p.clone().transpose(1, 2).contiguous()
        p_list, x_list = self.patch_embed(p, x, index=index)
        center_p, x = p_list[-1], self.proj(x_list[-1].transpose(1, 2))
        pos = _through(center_p, self.pos_embed)
        pos_embed = [self.cls_pos.expand(x.shape[0], -1, -1), pos]
        tokens = [self.cls_token.expand(x.shape[0], -1, -1), x]
        if self.dist_token is not None:
            pos_embed.insert(1, self.dist_pos.expand(x.shape[0], -1, -1))
            tokens.insert(1, self.dist_token.expand(x.shape[0], -1, -1))
        pos_embed = torch.cat(pos_embed, dim=1)
        x = torch.cat(tokens, dim=1)
        if self.add_pos_each_block:
            for block in self.blocks:
                x = block(x + pos_embed)
        else:
            x = self.pos_drop(x + pos_embed)
            for block in self.blocks:
                x = block(x)
        return p_list, x_list, self.norm(x)

    def forward_cls_feat(self, p, x=None, index=None):
        _, _, x = self.forward(p, x, index=index)
        token_features = x[:, self.n_tokens:, :]
        cls_feats = []
        for token_type in self.global_feat:
            if 'cls' in token_type:
                cls_feats.append(x[:, 0, :])
            elif 'max' in token_type:
                cls_feats.append(torch.max(token_features, dim=1, keepdim=False)[0])
            elif token_type in ['avg', 'mean']:
                cls_feats.append(torch.mean(token_features, dim=1, keepdim=False))
        global_features = torch.cat(cls_feats, dim=1)
        if self.dist_token is not None and self.training:
            return global_features, x[:, 1, :]
        return global_features

    def forward_seg_feat(self, p, x=None, index=None):
        p_list, x_list, x = self.forward(p, x, index=index)
        x_list[-1] = x.transpose(1, 2)
        return p_list, x_list


class PointVitClassifier(nn.Module):
    """`PointViT` + `ClsHead` behind the classifiers' interface (`PointMlpClassifier`'s shape), SmoothCrossEntropy(0.3).
    The repository's clouds are (x, y, z, height): in_channels = 4.  The head is cfgs/scanobjectnn/pix4point.yaml's:
    mlps [256, 256], BatchNorm1d."""

    def __init__(self, num_classes=15, in_channels=4, fused=None, mlps=(256, 256), **encoder_args):
        super().__init__()
        self.encoder = PointViT(in_channels=in_channels, fused=fused, **encoder_args)
        self.prediction = ClsHead(num_classes, self.encoder.out_channels, mlps=mlps)
        self.criterion = SmoothCrossEntropy(0.3)

    def forward(self, data, index=None):
        feats = self.encoder.forward_cls_feat(data, index=index)
        return self.prediction(feats[0] if isinstance(feats, tuple) else feats)

    def get_logits_loss(self, data, gt, index=None):
        logits = self.forward(data, index=index)
        return logits, self.criterion(logits, gt.long())
