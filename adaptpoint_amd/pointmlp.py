"""PointMLP (openpoints/models/backbone/pointmlp.py) over this build's operators: the residual-MLP classification
backbone, behind the same `forward({'pos', 'x'}) -> logits` / `get_logits_loss` interface as the other classifiers, so
it drops into `ClassifierStep`, `GanStep` and `Evaluator`.

Class names, argument lists and parameter names are the reference's (`embedding.net.0.weight`,
`local_grouper_list.<i>.affine_alpha`, `pre_blocks_list.<i>.transfer.net.{0,1}.*`,
`pre_blocks_list.<i>.operation.<j>.net{1,2}.*`, `pos_blocks_list.<i>.operation.<j>.*`, `classifier.*`): a reference
`state_dict` loads unchanged.  What differs is how a stage runs:

  * INDEX UP FRONT.  A stage's sample and its kNN graph depend only on the coordinates, so `PointMLPEncoder.index(p)`
    returns every stage's `affine_group.GroupIndex` from p alone (FPS -> gather -> `layers.knn_query(xyz, new_xyz, k)` ->
    the reverse lists), and `forward(..., graphs=, keep_graphs=)` takes them / keeps them in `last_graphs`.
    On the GPU the neighbours are the kernel's: the k smallest keys (direct-difference d^2, index).  The reference (and
    this mirror on CPU tensors) ranks -2 a.b + |a|^2 + |b|^2 with topk(largest=False, sorted=False).  The neighbour SETS
    agree wherever a query's k-th and (k+1)-th distances differ by more than rounding; the order inside a set matters to
    nothing downstream (the max over K, the standard deviation and BatchNorm are symmetric in it).
  * with fused=True a stage with normalize="anchor", use_xyz=False, groups=1, bias=False and ReLU runs
        affine_group_bn_act (ReLU)                               the grouper + the transfer convolution, hoisted
        conv_bn_act(ReLU) -> conv_bn_act on (B,O,S K)            every ConvBNReLURes1D of the PreExtraction
        add + ReLU (torch); the last block ends in res_relu_max  (the last (B,O,S K) activation is never written)
        conv_bn_act pairs on (B,O,S), add + ReLU (torch)         PosExtraction
    (adaptpoint_amd.affine_group, csrc/affine_group.hip); whatever that does not cover takes the composed path with a
    `set_abstraction._note_fallback` entry.  The fused stage has no BatchNorm exchange over ranks: with sync_bn at world
    size > 1 it raises instead of normalising rank-locally.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import affine_group as _ag
from . import layers, pointwise
from .pointnext import SmoothCrossEntropy


def get_activation(activation):
    a = activation.lower()
    if a == 'gelu':
        return nn.GELU()
    if a == 'rrelu':
        return nn.RReLU(inplace=True)
    if a == 'selu':
        return nn.SELU(inplace=True)
    if a == 'silu':
        return nn.SiLU(inplace=True)
    if a == 'hardswish':
        return nn.Hardswish(inplace=True)
    if a == 'leakyrelu':
        return nn.LeakyReLU(inplace=True)
    return nn.ReLU(inplace=True)


def square_distance(src, dst):
    """pointmlp.py:44-64: -2 src dst^T + |src|^2 + |dst|^2, (B,N,M)."""
    B, N, _ = src.shape
    M = dst.shape[1]
    dist = -2 * torch.matmul(src, dst.permute(0, 2, 1))
    dist += torch.sum(src ** 2, -1).view(B, N, 1)
    dist += torch.sum(dst ** 2, -1).view(B, 1, M)
    return dist


def index_points(points, idx):
    """points (B,N,C), idx (B,S[,K]) -> (B,S[,K],C)."""
    B = points.shape[0]
    shape = [B] + [1] * (idx.dim() - 1)
    return points[torch.arange(B, device=points.device).view(shape), idx.long(), :]


def knn_point(nsample, xyz, new_xyz):
    """pointmlp.py:134-146: the reference's own distance form and selection."""
    return torch.topk(square_distance(new_xyz, xyz), nsample, dim=-1, largest=False, sorted=False)[1]


class LocalGrouper(nn.Module):
    """pointmlp.py:149-199.  `forward(xyz, points, graph=None)`: graph = the stage's `GroupIndex` computed ahead."""

    def __init__(self, channel, sample_ratio, kneighbors, use_xyz=True, normalize="center", **kwargs):
        super().__init__()
        self.sample_ratio = sample_ratio
        self.kneighbors = kneighbors
        self.use_xyz = use_xyz
        self.normalize = normalize.lower() if normalize is not None else None
        if self.normalize not in ("center", "anchor"):
            self.normalize = None
        if self.normalize is not None:
            add_channel = 3 if self.use_xyz else 0
            self.affine_alpha = nn.Parameter(torch.ones([1, 1, 1, channel + add_channel]))
            self.affine_beta = nn.Parameter(torch.zeros([1, 1, 1, channel + add_channel]))

    @torch.no_grad()
    def index(self, xyz):
        """The stage's index work, a function of the coordinates alone -> `GroupIndex`."""
        xyz = xyz.detach().contiguous()
        N = xyz.shape[1]
        S = N // self.sample_ratio
        fps_idx = layers.furthest_point_sample(xyz, S)
        new_xyz = torch.gather(xyz, 1, fps_idx.long().unsqueeze(-1).expand(-1, -1, 3))
        if layers.knn_covers(xyz, new_xyz, self.kneighbors):
            idx = layers.knn_query(xyz, new_xyz, self.kneighbors)
        else:
            idx = knn_point(self.kneighbors, xyz, new_xyz).int()
        return _ag.group_index(fps_idx, new_xyz, idx, N)

    def forward(self, xyz, points, graph=None):
        """xyz (B,N,3), points (B,N,C) -> new_xyz (B,S,3), new_points (B,S,K,2C[+3])."""
        if graph is None:
            graph = self.index(xyz)
        B = xyz.shape[0]
        S = graph.fps_idx.shape[1]
        new_xyz = graph.new_xyz
        new_points = index_points(points, graph.fps_idx)
        grouped_points = index_points(points, graph.idx)
        if self.use_xyz:
            grouped_points = torch.cat([grouped_points, index_points(xyz, graph.idx)], dim=-1)
        if self.normalize is not None:
            if self.normalize == "center":
                mean = torch.mean(grouped_points, dim=2, keepdim=True)
            else:
                mean = torch.cat([new_points, new_xyz], dim=-1) if self.use_xyz else new_points
                mean = mean.unsqueeze(dim=-2)
            std = torch.std((grouped_points - mean).reshape(B, -1), dim=-1, keepdim=True).unsqueeze(-1).unsqueeze(-1)
            grouped_points = (grouped_points - mean) / (std + 1e-5)
            grouped_points = self.affine_alpha * grouped_points + self.affine_beta
        new_points = torch.cat([grouped_points, new_points.view(B, S, 1, -1).repeat(1, 1, self.kneighbors, 1)], dim=-1)
        return new_xyz, new_points


class ConvBNReLU1D(nn.Module):
    def __init__(self, in_channels, out_channels, kernel_size=1, bias=True, activation='relu'):
        super().__init__()
        self.act = get_activation(activation)
        self.net = nn.Sequential(
            nn.Conv1d(in_channels=in_channels, out_channels=out_channels, kernel_size=kernel_size, bias=bias),
            nn.BatchNorm1d(out_channels),
            self.act)

    def forward(self, x):
        return self.net(x)


class ConvBNReLURes1D(nn.Module):
    def __init__(self, channel, kernel_size=1, groups=1, res_expansion=1.0, bias=True, activation='relu'):
        super().__init__()
        self.act = get_activation(activation)
        mid = int(channel * res_expansion)
        self.net1 = nn.Sequential(
            nn.Conv1d(in_channels=channel, out_channels=mid, kernel_size=kernel_size, groups=groups, bias=bias),
            nn.BatchNorm1d(mid),
            self.act)
        if groups > 1:
            self.net2 = nn.Sequential(
                nn.Conv1d(in_channels=mid, out_channels=channel, kernel_size=kernel_size, groups=groups, bias=bias),
                nn.BatchNorm1d(channel),
                self.act,
                nn.Conv1d(in_channels=channel, out_channels=channel, kernel_size=kernel_size, bias=bias),
                nn.BatchNorm1d(channel))
        else:
            self.net2 = nn.Sequential(
                nn.Conv1d(in_channels=mid, out_channels=channel, kernel_size=kernel_size, bias=bias),
                nn.BatchNorm1d(channel))

    def forward(self, x):
        return self.act(self.net2(self.net1(x)) + x)


class PreExtraction(nn.Module):
    """[b,g,k,d] -> [b,d,g]."""

    def __init__(self, channels, out_channels, blocks=1, groups=1, res_expansion=1, bias=True, activation='relu',
                 use_xyz=True):
        super().__init__()
        in_channels = 3 + 2 * channels if use_xyz else 2 * channels
        self.transfer = ConvBNReLU1D(in_channels, out_channels, bias=bias, activation=activation)
        self.operation = nn.Sequential(*[
            ConvBNReLURes1D(out_channels, groups=groups, res_expansion=res_expansion, bias=bias, activation=activation)
            for _ in range(blocks)])

    def forward(self, x):
        b, n, s, d = x.size()
        x = x.permute(0, 1, 3, 2).reshape(-1, d, s)
        x = self.transfer(x)
        batch_size = x.shape[0]
        x = self.operation(x)
        x = F.adaptive_max_pool1d(x, 1).view(batch_size, -1)
        return x.reshape(b, n, -1).permute(0, 2, 1)


class PosExtraction(nn.Module):
    """[b,d,g] -> [b,d,g]."""

    def __init__(self, channels, blocks=1, groups=1, res_expansion=1, bias=True, activation='relu'):
        super().__init__()
        self.operation = nn.Sequential(*[
            ConvBNReLURes1D(channels, groups=groups, res_expansion=res_expansion, bias=bias, activation=activation)
            for _ in range(blocks)])

    def forward(self, x):
        return self.operation(x)


def _plain_pair(conv, bn):
    """A bias-free ungrouped 1x1 convolution and a BatchNorm the contraction kernels serve, without hooks."""
    return (isinstance(conv, nn.Conv1d) and conv.bias is None and conv.groups == 1 and conv.kernel_size == (1,)
            and conv.stride == (1,) and conv.padding == (0,) and conv.dilation == (1,)
            and isinstance(bn, nn.BatchNorm1d) and bn.affine and (bn.momentum is not None or not bn.training)
            and (bn.training or bn.track_running_stats)
            and not (conv._forward_hooks or conv._forward_pre_hooks or bn._forward_hooks or bn._forward_pre_hooks))


def _res_blocks_plain(operation):
    for blk in operation:
        if not isinstance(blk.act, nn.ReLU) or len(blk.net2) != 2:
            return False
        if not (_plain_pair(blk.net1[0], blk.net1[1]) and _plain_pair(blk.net2[0], blk.net2[1])):
            return False
        if blk._forward_hooks or blk._forward_pre_hooks:
            return False
    return True


def _res_block(t, blk):
    """net2(net1(t)) of a ConvBNReLURes1D on the contraction kernels (the add + ReLU is the caller's)."""
    h = pointwise.conv_bn_act(t, blk.net1[0], blk.net1[1], relu=True)
    return pointwise.conv_bn_act(h, blk.net2[0], blk.net2[1], relu=False)


class PointMLPEncoder(nn.Module):
    """pointmlp.py:295-355, with `fused=` / `sync_bn=` and the stages' graphs handed in or kept."""
    keep_graphs = False        # keep every forward's graphs in last_graphs (as the keep_graphs argument does for one call)
    last_graphs = None

    def __init__(self, in_channels=3, embed_dim=64, groups=1, res_expansion=1.0, activation="relu", bias=False,
                 use_xyz=False, normalize="anchor", dim_expansion=[2, 2, 2, 2], pre_blocks=[2, 2, 2, 2],
                 pos_blocks=[2, 2, 2, 2], k_neighbors=[24, 24, 24, 24], reducers=[2, 2, 2, 2], fused=False,
                 sync_bn=False, **kwargs):
        super().__init__()
        self.stages = len(pre_blocks)
        self.fused, self.sync_bn = fused, sync_bn
        self.cfg = dict(groups=groups, bias=bias, use_xyz=use_xyz, activation=activation)
        self.embedding = ConvBNReLU1D(in_channels, embed_dim, bias=bias, activation=activation)
        assert len(pre_blocks) == len(k_neighbors) == len(reducers) == len(pos_blocks) == len(dim_expansion), \
            "Please check stage number consistent for pre_blocks, pos_blocks k_neighbors, reducers."
        self.local_grouper_list = nn.ModuleList()
        self.pre_blocks_list = nn.ModuleList()
        self.pos_blocks_list = nn.ModuleList()
        last_channel = embed_dim
        for i in range(len(pre_blocks)):
            out_channel = last_channel * dim_expansion[i]
            self.local_grouper_list.append(LocalGrouper(last_channel, reducers[i], k_neighbors[i], use_xyz, normalize))
            self.pre_blocks_list.append(PreExtraction(last_channel, out_channel, pre_blocks[i], groups=groups,
                                                      res_expansion=res_expansion, bias=bias, activation=activation,
                                                      use_xyz=use_xyz))
            self.pos_blocks_list.append(PosExtraction(out_channel, pos_blocks[i], groups=groups,
                                                      res_expansion=res_expansion, bias=bias, activation=activation))
            last_channel = out_channel
        self.out_channels = last_channel
        self.act = get_activation(activation)

    @torch.no_grad()
    def index(self, p):
        """Every stage's `GroupIndex` from the coordinates p (B,N,3) alone."""
        graphs = []
        for grouper in self.local_grouper_list:
            graphs.append(grouper.index(p))
            p = graphs[-1].new_xyz
        return graphs

    def _uncovered(self, i, x, graph):
        """None when the kernels cover stage i for this call, else the reason they do not."""
        grouper, pre, pos = self.local_grouper_list[i], self.pre_blocks_list[i], self.pos_blocks_list[i]
        B, C, N = x.shape
        S, K = graph.idx.shape[1:]
        conv, bn = pre.transfer.net[0], pre.transfer.net[1]
        if graph.nbr_list is None or graph.anc_list is None:
            return (f"PointMLP stage C={C} -> {conv.out_channels}: the GroupIndex handed in carries no reverse lists "
                    "(it was built from CPU tensors): build it with PointMLPEncoder.index on the device")
        ok = (_ag.covers(B, N, S, K, C, conv.out_channels, normalize=grouper.normalize, **self.cfg)
              and isinstance(pre.transfer.act, nn.ReLU)
              and conv.in_channels == 2 * C and _plain_pair(conv, bn)
              and not (grouper._forward_hooks or grouper._forward_pre_hooks or pre._forward_hooks or pre._forward_pre_hooks
                       or pos._forward_hooks or pos._forward_pre_hooks or pre.transfer._forward_hooks)
              and _res_blocks_plain(pre.operation) and _res_blocks_plain(pos.operation))
        if ok:
            return None
        return (f"PointMLP stage C={C} -> {conv.out_channels}, K={K}, normalize={grouper.normalize}, "
                f"use_xyz={self.cfg['use_xyz']}, groups={self.cfg['groups']}, bias={self.cfg['bias']}, "
                f"activation={self.cfg['activation']}: no fused kernel for this stage")

    def _fused_stage(self, i, x, graph, pos_blocks=True):
        """x (B,C,N) -> (B,O,S) on csrc/affine_group.hip and the contraction kernels (pos_blocks=False: without the
        stage's PosExtraction)."""
        grouper, pre, pos = self.local_grouper_list[i], self.pre_blocks_list[i], self.pos_blocks_list[i]
        K = graph.idx.shape[2]
        t = _ag.affine_group_bn_act(pointwise.transpose12(x), graph, grouper.affine_alpha, grouper.affine_beta,
                                    pre.transfer.net[0].weight, pre.transfer.net[1], relu=True)
        blocks = list(pre.operation)
        if not blocks:
            out = t.view(t.shape[0], t.shape[1], -1, K).max(dim=-1)[0]
        for j, blk in enumerate(blocks):
            z = _res_block(t, blk)
            if j == len(blocks) - 1:
                out = _ag.res_relu_max(z, t, K)
            else:
                t = torch.relu(z + t)
        for blk in (pos.operation if pos_blocks else ()):
            out = torch.relu(_res_block(out, blk) + out)
        return out

    def _stages(self, p, x, graphs, keep_graphs):
        from .set_abstraction import _note_fallback, _ranks
        if graphs is not None and len(graphs) != self.stages:
            raise ValueError(f"{type(self).__name__}: {self.stages} graphs expected, {len(graphs)} given")
        emb = self.embedding
        if (self.fused and x.is_cuda and x.dtype == torch.float32 and isinstance(emb.act, nn.ReLU)
                and _plain_pair(emb.net[0], emb.net[1]) and not (emb._forward_hooks or emb._forward_pre_hooks)):
            x = pointwise.conv_bn_act(x.contiguous(), emb.net[0], emb.net[1], relu=True)
        else:
            x = emb(x)
        used = []
        for i in range(self.stages):
            graph = graphs[i] if graphs is not None else self.local_grouper_list[i].index(p)
            used.append(graph)
            fused = False
            if self.fused and x.is_cuda and x.dtype == torch.float32:
                reason = self._uncovered(i, x, graph)
                if self.sync_bn and _ranks() > 1:
                    raise RuntimeError("PointMLP(fused=True, sync_bn=True): the fused stage has no BatchNorm exchange "
                                       "over ranks and never normalises rank-locally: convert the BatchNorm modules "
                                       "(adaptpoint_amd.dp.convert_sync_batchnorm) and build the model with fused=False")
                if reason is None:
                    fused = True
                else:
                    _note_fallback(reason)
            if fused:
                x = self._fused_stage(i, x.contiguous(), graph)
            else:
                _, g = self.local_grouper_list[i](p, x.permute(0, 2, 1), graph)
                x = self.pos_blocks_list[i](self.pre_blocks_list[i](g))
            p = graph.new_xyz
        self.last_graphs = used if (keep_graphs or self.keep_graphs) else None
        return F.adaptive_max_pool1d(x, 1).squeeze(dim=-1)

    @staticmethod
    def _inputs(p, x):
        if hasattr(p, 'keys'):
            p, x = p['pos'], p.get('x', None)
        if x is None:
            x = p.transpose(1, 2).contiguous()
        return p, x

    def forward(self, p, x=None, graphs=None, keep_graphs=False):
        return self.forward_cls_feat(p, x, graphs=graphs, keep_graphs=keep_graphs)

    def forward_cls_feat(self, p, x=None, graphs=None, keep_graphs=False):
        p, x = self._inputs(p, x)
        return self._stages(p, x, graphs, keep_graphs)


class PointMLP(PointMLPEncoder):
    """pointmlp.py:358-399: the encoder with its classifier head."""

    def __init__(self, in_channels=3, num_classes=15, embed_dim=64, groups=1, res_expansion=1.0, activation="relu",
                 bias=False, use_xyz=False, normalize="anchor", dim_expansion=[2, 2, 2, 2], pre_blocks=[2, 2, 2, 2],
                 pos_blocks=[2, 2, 2, 2], k_neighbors=[24, 24, 24, 24], reducers=[2, 2, 2, 2], group_args=None, **kwargs):
        super().__init__(in_channels, embed_dim, groups, res_expansion, activation, bias, use_xyz, normalize,
                         dim_expansion, pre_blocks, pos_blocks, k_neighbors, reducers, **kwargs)
        self.classifier = nn.Sequential(
            nn.Linear(self.out_channels, 512), nn.BatchNorm1d(512), self.act, nn.Dropout(0.5),
            nn.Linear(512, 256), nn.BatchNorm1d(256), self.act, nn.Dropout(0.5),
            nn.Linear(256, num_classes))

    def forward_cls_feat(self, p, x=None, graphs=None, keep_graphs=False):
        p, x = self._inputs(p, x)
        return self.classifier(self._stages(p, x, graphs, keep_graphs))


ELITE = dict(embed_dim=32, groups=1, res_expansion=0.25, activation="relu", bias=False, use_xyz=False,
             normalize="anchor", dim_expansion=[2, 2, 2, 1], pre_blocks=[1, 1, 2, 1], pos_blocks=[1, 1, 2, 1],
             k_neighbors=[24, 24, 24, 24], reducers=[2, 2, 2, 2])
FULL = dict(embed_dim=64, groups=1, res_expansion=1.0, activation="relu", bias=False, use_xyz=False,
            normalize="anchor", dim_expansion=[2, 2, 2, 2], pre_blocks=[2, 2, 2, 2], pos_blocks=[2, 2, 2, 2],
            k_neighbors=[24, 24, 24, 24], reducers=[2, 2, 2, 2])


def pointMLP(num_classes=40, **kwargs) -> PointMLPEncoder:
    return PointMLPEncoder(num_classes=num_classes, **FULL, **kwargs)


def pointMLPElite(num_classes=40, **kwargs) -> PointMLPEncoder:
    return PointMLPEncoder(num_classes=num_classes, **ELITE, **kwargs)


class PointMlpClassifier(nn.Module):
    """`PointMLP` behind the classifiers' interface (`dgcnn.GraphClassifier`'s shape): `encoder` is the whole reference
    model, head included; SmoothCrossEntropy(0.3).  The repository's clouds are (x, y, z, height): in_channels = 4."""

    def __init__(self, num_classes=15, in_channels=4, fused=False, **encoder_args):
        super().__init__()
        self.encoder = PointMLP(in_channels=in_channels, num_classes=num_classes, fused=fused, **encoder_args)
        self.criterion = SmoothCrossEntropy(0.3)

    def forward(self, data, graphs=None, keep_graphs=False):
        return self.encoder(data, graphs=graphs, keep_graphs=keep_graphs)

    def get_logits_loss(self, data, gt, graphs=None, keep_graphs=False):
        logits = self.forward(data, graphs=graphs, keep_graphs=keep_graphs)
        return logits, self.criterion(logits, gt.long())
