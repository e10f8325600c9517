"""DeepGCN / ResGCN (openpoints/models/backbone/deepgcn.py over layers/graph_conv.py and layers/knn.py) on this build's
operators: the other half of the reference's graph_conv.py -- `DilatedKNN`, dilated and stochastic `DynConv`,
`ResDynBlock` -- behind the `forward({'pos', 'x'}) -> logits` / `get_logits_loss` interface of `DgcnnClassifier`, so it
drops into `ClassifierStep`, `GanStep` and `Evaluator` unchanged.

Attribute names are the reference's (`head.gconv.nn.{0,1}.*`, `backbone.<i>.body.gconv.nn.{0,1}.*` for block='res',
`backbone.<i>.gconv.nn.{0,1}.*` for 'plain', `fusion_block.{0,1}.*`): a reference `state_dict` loads unchanged.  What
differs is how a block runs:

  * the dilated graph -- the reference's `cdist(x, x).topk(k d)` over a (B,N,N) tensor, then k of the k d columns --
    comes from `layers.knn_dilated` (csrc/knn.hip, k d <= 256) in one launch that writes only the k wanted ranks;
    CPU tensors keep the reference's lines, k d > 256 on the GPU takes them with a `_note_fallback` entry;
  * with fused=True an EdgeConv block runs on csrc/edge_conv.hip with ReLU (slope 0) and, in a `ResDynBlock`, the
    residual added in the output kernel (`edge_conv.edge_conv(..., residual=x)`): `body(x) + x` without another pass.

`EdgeConv`, `GraphConv` and the bases of the backbone and the classifier are `adaptpoint_amd.dgcnn`'s.

Random draws (stochastic=True) are the reference's, on the host from torch's CPU generator, in its order and number:
every `DilatedKNN.forward` draws `torch.rand(1)` -- in eval mode too -- and `torch.randperm(k d)[:k]` only when training
and that draw is below epsilon; the head's `DilatedKNN` first, then the blocks in order.  The chosen ranks (strided
j d, or the permutation's first k) go into the module's device buffer `slots`, which `knn_dilated` always reads, so the
launch is the same either way.  Under stream capture nothing is drawn or copied -- the buffer is used as it stands --
and `DeepGCN.redraw()` makes all modules' draws and refreshes the buffers between replays.

block='dense' and conv='mr' are refused: the reference itself cannot construct the first (`DenseDynBlock`'s own
`assert out_channels > in_channels` fails for every block of `DeepGCN(block='dense')`) or run the second ('mr' is a
KeyError in its layer table, and `MRConv.forward` calls `x.unsequence`, which does not exist), so nothing exists to pin
them against.
"""
import torch
import torch.nn as nn

from . import edge_conv as _ec
from .dgcnn import LEAKY, EdgeConv, GraphBackbone, GraphClassifier, GraphConv, _gconv      # noqa: F401 (EdgeConv: this module's too)
from .layers import knn_dilated, knn_dilated_covers
from .set_abstraction import convblock

RELU = {'act': 'relu'}


def _capturing(t):
    return t.is_cuda and torch.cuda.is_current_stream_capturing()


class DenseDilated(nn.Module):
    """layers/knn.py:65-88: k of the k d nearest neighbours -- every d-th, or (stochastic, training, with probability
    epsilon) the first k of a random permutation.  `draw()` makes the reference's host draws and returns the ranks;
    `forward(edge_index)` is the reference's call on an index tensor (B,N,k d)."""

    def __init__(self, k=9, dilation=1, stochastic=False, epsilon=0.0):
        super().__init__()
        self.dilation, self.stochastic, self.epsilon, self.k = dilation, stochastic, epsilon, k

    def draw(self):
        """-> the k ranks (int64, host).  torch's CPU generator moves exactly as in the reference's forward."""
        if self.stochastic:
            if torch.rand(1) < self.epsilon and self.training:
                return torch.randperm(self.k * self.dilation)[:self.k]
        return torch.arange(0, self.k * self.dilation, self.dilation)

    def forward(self, edge_index, ranks=None):
        if ranks is None:
            ranks = self.draw()
        return edge_index.index_select(2, ranks.to(edge_index.device).long()).contiguous()


class DilatedKNN(nn.Module):
    """layers/knn.py:91-108: the dilated kNN graph of query (B,N,C), itself included -> (B,N,k) int32."""

    def __init__(self, k=9, dilation=1, stochastic=False, epsilon=0.0):
        super().__init__()
        self.dilation, self.stochastic, self.epsilon, self.k = dilation, stochastic, epsilon, k
        self._dilated = DenseDilated(k, dilation, stochastic, epsilon)
        # the ranks `knn_dilated` reads: not a parameter of the model (the reference has none), so not in the state_dict
        self.register_buffer('slots', torch.arange(0, k * dilation, dilation, dtype=torch.int32), persistent=False)

    @torch.no_grad()
    def redraw(self):
        """Make this module's draws and refresh `slots`; -> the ranks.  Never under stream capture."""
        ranks = self._dilated.draw()
        if self.stochastic:                              # (without it the buffer holds the strided ranks for good)
            self.slots.copy_(ranks.int())
        return ranks

    @torch.no_grad()
    def forward(self, query):
        kd = self.k * self.dilation
        if kd > query.shape[1]:
            raise ValueError(f"DilatedKNN: k * dilation = {kd} neighbours of {query.shape[1]} points")
        capturing = _capturing(query)
        if not capturing:
            self.redraw()
        if knn_dilated_covers(query, query, self.k, self.dilation):
            query = query.contiguous()
            return knn_dilated(query, query, self.k, self.dilation, slots=self.slots)
        if query.is_cuda:
            from .set_abstraction import _note_fallback
            _note_fallback(f"DilatedKNN k={self.k} d={self.dilation} on {tuple(query.shape)} {query.dtype}: outside "
                           "knn_dilated's limits")
        idx = torch.cdist(query, query).topk(k=kd, dim=-1, largest=False, sorted=True).indices.int()
        return self._dilated(idx, self.slots)


class DynConv(GraphConv):
    """graph_conv.py:75-89: the graph is the dilated kNN of the block's own input, rebuilt every forward.
    `forward(x, edge_index=None, residual=None)`: edge_index = neighbours computed ahead (then nothing is drawn); the
    graph used is kept in `last_graph`."""

    def __init__(self, in_channels, out_channels, conv='edge', k=9, dilation=1, stochastic=False, epsilon=0.0,
                 fused=False, **kwargs):
        super().__init__(in_channels, out_channels, conv, fused=fused, **kwargs)
        self.k, self.d = k, dilation
        self.dilated_knn_graph = DilatedKNN(k, dilation, stochastic, epsilon)
        self.last_graph = None

    def forward(self, x, edge_index=None, residual=None):
        if edge_index is None:
            edge_index = self.dilated_knn_graph(x.detach().squeeze(-1).transpose(1, 2))
        self.last_graph = edge_index.idx if isinstance(edge_index, _ec.EdgeIndex) else edge_index
        return super().forward(x, edge_index, residual)


class ResDynBlock(nn.Module):
    """graph_conv.py:92-104: body(x) + x; fused, the sum is the EdgeConv output kernel's epilogue."""

    def __init__(self, in_channels, conv='edge', k=9, dilation=1, stochastic=False, epsilon=0.0, fused=False, **kwargs):
        super().__init__()
        self.body = DynConv(in_channels, in_channels, conv, k, dilation, stochastic, epsilon, fused=fused, **kwargs)

    @property
    def last_graph(self):
        return self.body.last_graph

    def forward(self, x, edge_index=None):
        return self.body(x, edge_index, residual=x)


class DeepGCN(GraphBackbone):
    """deepgcn.py:13-128: a static EdgeConv on the coordinates' graph, n_blocks - 1 dynamic blocks of constant width
    (block='res': residual, dilation 1 + i with use_dilation, stochastic with use_stochastic; 'plain': neither), all
    outputs concatenated into a Conv1d-BN-LeakyReLU(0.2) fusion block; forward_cls_feat pools it to cat(max, mean).
    `graphs=`: the n_blocks graphs computed ahead (then nothing is drawn); `keep_graphs` / `last_graphs` as `DGCNN`."""

    def __init__(self, in_channels=3, channels=64, emb_dims=1024, n_blocks=14, conv='edge', block='res', k=16,
                 epsilon=0.2, use_stochastic=True, use_dilation=True, norm_args=None, act_args=None, conv_args=None,
                 is_seg=False, fused=False, sync_bn=False, **kwargs):
        super().__init__()
        norm_args = {'norm': 'bn'} if norm_args is None else norm_args
        act_args = dict(RELU) if act_args is None else act_args
        conv_args = {'order': 'conv-norm-act'} if conv_args is None else conv_args
        _gconv(conv)
        self.n_blocks, self.k, self.n_graphs = n_blocks, k, n_blocks
        common = dict(fused=fused, sync_bn=sync_bn, act_args=act_args, norm_args=norm_args, **conv_args)
        self.knn = DilatedKNN(k, 1, use_stochastic, epsilon)
        self.head = GraphConv(in_channels, channels, conv, bias=False, **common)
        kind = block.lower()
        if kind == 'dense':
            raise NotImplementedError("DeepGCN(block='dense') cannot be constructed in the reference either "
                                      "(DenseDynBlock(channels + c_growth * i, c_growth, ...) fails its own `assert "
                                      "out_channels > in_channels`): there is nothing to pin it against")
        if kind == 'res':
            self.backbone = nn.Sequential(*[ResDynBlock(channels, conv, k, 1 + i if use_dilation else 1, use_stochastic,
                                                        epsilon, **common) for i in range(n_blocks - 1)])
        else:       # plain GCN: no dilation, no stochastic graphs, no residual connections
            self.backbone = nn.Sequential(*[DynConv(channels, channels, conv, k, 1, False, epsilon, **common)
                                            for i in range(n_blocks - 1)])
        self.fusion_block = convblock(int(channels * n_blocks), emb_dims, 1, norm_args=norm_args, act_args=dict(LEAKY),
                                      bias=False, **conv_args)
        self.model_init()
        self.out_channels = emb_dims if is_seg else emb_dims * 2

    def model_init(self):
        for m in self.modules():
            if isinstance(m, (nn.Conv2d, nn.Conv1d)):
                nn.init.kaiming_normal_(m.weight)
                if m.bias is not None:
                    m.bias.data.zero_()
            elif isinstance(m, (nn.BatchNorm2d, nn.BatchNorm1d)):
                nn.init.constant_(m.bias, 0)
                nn.init.constant_(m.weight, 1.0)

    def graph_modules(self):
        """The `DilatedKNN` modules in the order they draw: the head's, then the blocks'."""
        return [self.knn] + [(b.body if isinstance(b, ResDynBlock) else b).dilated_knn_graph for b in self.backbone]

    def redraw(self):
        """All modules' draws, in a forward's order, and their `slots` buffers refreshed: what a caller replaying a
        captured step does between replays (under capture a forward draws and copies nothing)."""
        for m in self.graph_modules():
            m.redraw()

    def _head_graph(self, pts):
        return self.knn(pts)


class DeepGcnClassifier(GraphClassifier):
    """`GraphClassifier` over DeepGCN: `DgcnnClassifier`'s head and criterion."""
    encoder_class = DeepGCN

    def redraw(self):
        self.encoder.redraw()
