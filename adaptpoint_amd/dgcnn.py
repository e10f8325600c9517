"""DGCNN (openpoints/models/backbone/dgcnn.py) over this build's operators: the backbone the corruption-robustness
literature uses beside PointNeXt, behind the same `forward({'pos', 'x'}) -> logits` / `get_logits_loss` interface, so it
drops into `ClassifierStep`, `GanStep` and `Evaluator` unchanged.

Attribute names are the reference's (`head.gconv.nn.0.weight`, `backbone.<i>.gconv.nn.{0,1}.*`, `fusion_block.{0,1}.*`):
a reference `state_dict` loads unchanged.  What differs is how a block runs:

  * the kNN graph (layers/knn.py: `cdist(...).topk(...)`, a (B,N,N) tensor) comes from `layers.knn_query` on the GPU --
    exact distances by direct differences, ties to the smaller index; CPU tensors keep the reference's call;
  * with fused=True an EdgeConv block (layers/graph_conv.py:38-51: group, concatenate, Conv2d-BN-LeakyReLU, max over K)
    runs on csrc/edge_conv.hip (`adaptpoint_amd.edge_conv`) without the (B,2C,N,K) and (B,H,N,K) tensors; whatever the
    kernels do not cover takes the composed path with a `set_abstraction._note_fallback` entry.

DGCNN itself uses conv='edge', dilation 1, no stochastic graphs, LeakyReLU and no residual.  `EdgeConv`, `GraphConv` and
the bases of the backbone and the classifier are shared with `adaptpoint_amd.deepgcn`, which adds the dilated and
stochastic graphs and the residual blocks: so `EdgeConv` takes ReLU and a residual too.
"""
import torch
import torch.nn as nn

from . import edge_conv as _ec
from .layers import grouping_operation, knn_covers, knn_query
from .pointnext import ClsHead, SmoothCrossEntropy
from .set_abstraction import convblock

LEAKY = {'act': 'leakyrelu', 'negative_slope': 0.2}


@torch.no_grad()
def knn_graph(x, k):
    """The k nearest rows of every row of x (B,N,C), itself included: (B,N,k) int32.  On the GPU the kernel's graph
    (`layers.knn_query`), elsewhere the reference's own call (layers/knn.py:59-61)."""
    if knn_covers(x, x, k):
        x = x.contiguous()
        return knn_query(x, x, k)
    return torch.cdist(x, x).topk(k=k, dim=-1, largest=False, sorted=True).indices.int()


def _group(x, idx):
    """x (B,C,N), idx (B,N,K) -> (B,C,N,K): the grouping operator on the GPU, a gather elsewhere."""
    if x.is_cuda:
        return grouping_operation(x.contiguous(), idx.int().contiguous())
    return x.unsqueeze(2).expand(-1, -1, idx.shape[1], -1).gather(3, idx.long().unsqueeze(1).expand(-1, x.shape[1], -1, -1))


class EdgeConv(nn.Module):
    """graph_conv.py:38-51: max_k nn([x_i ; x_j - x_i]) [+ residual] for x (B,C,N,1), edge_index (B,N,K) and an optional
    residual (B,H,N,1) added behind the max -> (B,H,N,1).  The activation is ReLU or LeakyReLU(slope >= 0).
    edge_index may be an `edge_conv.EdgeIndex` (the graph with its reverse lists, built in the index step)."""

    def __init__(self, in_channels, out_channels, norm_args=None, act_args=None, order='conv-norm-act', fused=False,
                 sync_bn=False, **kwargs):
        super().__init__()
        self.nn = convblock(in_channels * 2, out_channels, 2, norm_args=norm_args, act_args=act_args, order=order, **kwargs)
        self.fused, self.sync_bn = fused, sync_bn

    def _uncovered(self, x, K):
        """None when csrc/edge_conv.hip covers this call, else the reason it does not."""
        blk = tuple(self.nn)
        ok = (len(blk) == 3 and isinstance(blk[0], nn.Conv2d) and isinstance(blk[1], nn.BatchNorm2d)
              and (isinstance(blk[2], nn.ReLU) or (isinstance(blk[2], nn.LeakyReLU) and blk[2].negative_slope >= 0))
              and (blk[1].training or blk[1].track_running_stats) and blk[1].affine
              and not (self.nn._forward_hooks or self.nn._forward_pre_hooks or blk[0]._forward_hooks or blk[1]._forward_hooks))
        if ok:
            ok = _ec.covers(x.shape[0], x.shape[2], K, x.shape[1], blk[0].out_channels, blk[0].bias is not None,
                            blk[1].momentum)
        if ok:
            return None
        return (f"EdgeConv C_in={x.shape[1]} -> {blk[0].out_channels}, K={K}: no fused kernel for this block")

    def forward(self, x, edge_index, residual=None):
        from .set_abstraction import _note_fallback, _ranks
        graph = edge_index if isinstance(edge_index, _ec.EdgeIndex) else None
        idx = graph.idx if graph is not None else edge_index
        if self.fused and x.is_cuda and x.dtype == torch.float32:
            reason = self._uncovered(x, idx.shape[-1])
            if self.sync_bn and _ranks() > 1:
                raise RuntimeError("EdgeConv(fused=True, sync_bn=True): the fused block has no BatchNorm exchange over "
                                   "ranks and never normalises rank-locally: convert the BatchNorm modules "
                                   "(adaptpoint_amd.dp.convert_sync_batchnorm) and build the block with fused=False")
            if reason is None:
                if graph is None:
                    graph = _ec.edge_index(idx)
                conv, bn, act = self.nn
                slope = 0.0 if isinstance(act, nn.ReLU) else act.negative_slope
                xs = x.squeeze(-1)
                res = None if residual is None else (xs if residual is x else residual.squeeze(-1))
                return _ec.edge_conv(xs, graph, conv, bn, slope, residual=res).unsqueeze(-1)
            _note_fallback(reason)
        x_j = _group(x.squeeze(-1), idx)
        y = self.nn(torch.cat([x.expand(-1, -1, -1, idx.shape[-1]), x_j - x], dim=1))
        y = torch.max(y, -1, keepdim=True)[0]
        return y if residual is None else y + residual


def _gconv(conv):
    if conv in ('mr', 'mrconv'):
        raise NotImplementedError("graph convolution 'mr' cannot run in the reference either ('mr' is a KeyError in its "
                                  "layer table and MRConv.forward calls x.unsequence, which does not exist): there is "
                                  "nothing to pin it against")
    if conv not in ('edge', 'edgeconv') and conv is not EdgeConv:
        raise NotImplementedError(f"graph convolution '{conv}' is outside the hot-path build (DGCNN and DeepGCN use 'edge')")
    return EdgeConv


class GraphConv(nn.Module):
    """graph_conv.py:61-72: a graph convolution on a graph that is handed in."""

    def __init__(self, in_channels, out_channels, conv='edge', fused=False, **kwargs):
        super().__init__()
        self.gconv = _gconv(conv)(in_channels, out_channels, fused=fused, **kwargs)

    def forward(self, x, edge_index, residual=None):
        return self.gconv(x, edge_index, residual)


class DynConv(GraphConv):
    """graph_conv.py:75-89: the graph is the kNN of the block's own input, rebuilt every forward.
    `forward(x, edge_index=None)`: edge_index = neighbours computed ahead; the graph used is kept in `last_graph`."""

    def __init__(self, in_channels, out_channels, conv='edge', k=9, dilation=1, stochastic=False, epsilon=0.0,
                 fused=False, **kwargs):
        if dilation != 1 or stochastic:
            raise NotImplementedError("dilated and stochastic kNN graphs are outside the hot-path build (DGCNN uses "
                                      "dilation 1, non-stochastic)")
        super().__init__(in_channels, out_channels, conv, fused=fused, **kwargs)
        self.k, self.d = k, dilation
        self.last_graph = None

    def forward(self, x, edge_index=None):
        if edge_index is None:
            edge_index = knn_graph(x.detach().squeeze(-1).transpose(1, 2), self.k)
        self.last_graph = edge_index.idx if isinstance(edge_index, _ec.EdgeIndex) else edge_index
        return super().forward(x, edge_index)


class GraphBackbone(nn.Module):
    """What DGCNN and DeepGCN share: `head` on the graph of the coordinates, the blocks of `backbone` each on the graph
    of its own input, all outputs concatenated into `fusion_block`.  A subclass builds those three, sets `n_graphs`
    (one per graph convolution) and says how the head's graph is made (`_head_graph`)."""
    n_graphs = 0
    keep_graphs = False        # keep every forward's graphs in last_graphs (as the keep_graphs argument does for one call)
    last_graphs = None

    def _head_graph(self, pts):
        raise NotImplementedError

    def _features(self, pts, features, graphs, keep_graphs):
        if hasattr(pts, 'keys'):
            pts, features = pts['pos'], pts['x']
        if features is None:
            features = pts.transpose(1, 2).contiguous()
        if features.dim() < 4:
            features = features.unsqueeze(-1)
        if graphs is not None and len(graphs) != self.n_graphs:
            raise ValueError(f"{type(self).__name__}: {self.n_graphs} graphs expected, {len(graphs)} given")
        g0 = graphs[0] if graphs is not None else self._head_graph(pts.detach())
        feats = [self.head(features, g0)]
        used = [g0.idx if isinstance(g0, _ec.EdgeIndex) else g0]
        for i, blk in enumerate(self.backbone):
            feats.append(blk(feats[-1], None if graphs is None else graphs[i + 1]))
            used.append(blk.last_graph)
        self.last_graphs = used if (keep_graphs or self.keep_graphs) else None
        return self.fusion_block(torch.cat(feats, dim=1).squeeze(-1))

    def forward(self, pts, features=None, graphs=None, keep_graphs=False):
        return self._features(pts, features, graphs, keep_graphs)

    def forward_seg_feat(self, pts, features=None):
        if hasattr(pts, 'keys'):
            pts, features = pts['pos'], pts['x']
        return pts, self._features(pts, features, None, False)

    def forward_cls_feat(self, pts, features=None, graphs=None, keep_graphs=False):
        fusion = self._features(pts, features, graphs, keep_graphs)
        return torch.cat((fusion.max(dim=-1)[0], fusion.mean(dim=-1)), dim=1)


class DGCNN(GraphBackbone):
    """dgcnn.py:13-104: a static EdgeConv on the coordinates' graph, n_blocks - 2 dynamic ones (the width doubling
    from the second on), all outputs concatenated into a Conv1d-BN-LeakyReLU fusion block; forward_cls_feat pools it
    to cat(max, mean)."""

    def __init__(self, in_channels=3, channels=64, embed_dim=1024, n_blocks=5, conv='edge', k=20, norm_args=None,
                 act_args=None, conv_args=None, is_seg=False, fused=False, sync_bn=False, **kwargs):
        super().__init__()
        if kwargs.get('dilation', 1) != 1 or kwargs.get('use_dilation', False) or kwargs.get('stochastic', False) \
                or kwargs.get('use_stochastic', False):
            raise NotImplementedError("dilated and stochastic kNN graphs are outside the hot-path build")
        norm_args = {'norm': 'bn'} if norm_args is None else norm_args
        act_args = dict(LEAKY) if act_args is None else act_args
        conv_args = {'order': 'conv-norm-act'} if conv_args is None else conv_args
        self.n_blocks, self.k, self.n_graphs = n_blocks, k, n_blocks - 1
        self.head = GraphConv(in_channels, channels, conv, fused=fused, sync_bn=sync_bn, norm_args=norm_args, act_args=act_args, **conv_args)
        out_channels = [channels]
        c_in = channels
        backbone = []
        for _ in range(n_blocks - 2):
            backbone.append(DynConv(c_in, channels, conv, k, fused=fused, sync_bn=sync_bn, act_args=act_args, norm_args=norm_args,
                                    **conv_args))
            out_channels.append(channels)
            c_in = channels
            channels *= 2
        self.backbone = nn.Sequential(*backbone)
        self.fusion_block = convblock(int(sum(out_channels)), embed_dim, 1, norm_args=norm_args, act_args=act_args,
                                      bias=False, **conv_args)
        self.out_channels = embed_dim if is_seg else embed_dim * 2

    def _head_graph(self, pts):
        return knn_graph(pts, self.k)


class GraphClassifier(nn.Module):
    """BaseCls (classification/cls_base.py:13-39) over `encoder_class`: the encoder, ClsHead(2 embed_dim -> 512 -> 256 ->
    num_classes) with BatchNorm1d, LeakyReLU(0.2) and dropout 0.5, SmoothCrossEntropy(0.3).  The repository's clouds are
    (x, y, z, height): in_channels = 4."""
    encoder_class = None

    def __init__(self, num_classes=15, in_channels=4, fused=False, **encoder_args):
        super().__init__()
        self.encoder = self.encoder_class(in_channels=in_channels, fused=fused, **encoder_args)
        self.prediction = ClsHead(num_classes, self.encoder.out_channels, mlps=(512, 256),
                                  act=lambda: nn.LeakyReLU(LEAKY['negative_slope'], inplace=True))
        self.criterion = SmoothCrossEntropy(0.3)

    def forward(self, data, graphs=None, keep_graphs=False):
        return self.prediction(self.encoder.forward_cls_feat(data, graphs=graphs, keep_graphs=keep_graphs))

    def get_logits_loss(self, data, gt, graphs=None, keep_graphs=False):
        logits = self.forward(data, graphs=graphs, keep_graphs=keep_graphs)
        return logits, self.criterion(logits, gt.long())


class DgcnnClassifier(GraphClassifier):
    """`GraphClassifier` over DGCNN."""
    encoder_class = DGCNN
