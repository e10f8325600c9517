"""Point Transformer (openpoints/models/backbone/pointtransformer.py) over the stacked-cloud operators of
`adaptpoint_amd.pointops`: points (n,3), features (n,c) and an int32 `offset` (b) of cumulative END rows.

Class, constructor-argument and attribute names are the reference's (`enc2.1.transformer2.linear_w.2.weight`, ...): a
reference `state_dict` loads unchanged.  What differs is how the model runs:

  * ONE graph per level.  Every block of an encoder stage, and the decoder stage of the same level, sees the same
    (p, o, nsample); the reference queries the kNN twice per layer.  A `StageGraph` holds idx (n,k) and, lazily, the
    neighbours' offsets d = grouping(p, idx) - p[:,None] (no gradient); `PTSeg.forward` builds one per level and hands
    it along as an optional fourth entry of the [p, x, o] list.  A module given the reference's 3-list builds its own
    graph; `TransitionDown` drops the fourth entry (the point set changes).  5 kNN launches for the layers of a forward
    instead of 36.  The backward passes of all gathers through one idx share its reverse lists (`pointops.csr_of`);
  * CUDA float32 tensors run on the kernels through `adaptpoint_amd.pointops` (memset-free, atomic-free Functions);
    anything else -- CPU tensors, float64 -- takes the small torch statements below: kNN per cloud by ascending
    (d2, index) with the short-cloud padding rule (start of the cloud, 1e10), furthest sampling per cloud from its first
    point, gathers by indexing, interpolation with k = 3 in the reference's loop order;
  * `graphs=` / `keep_graphs=` as `DGCNN` has them: `last_graphs` holds the five stage graphs, the (sampled index,
    group index) of the four strided `TransitionDown`s and the interpolation index of the four `TransitionUp`s, so that
    a float64 run or a second model runs on identical graphs;
  * with fused=True a covered `PointTransformerLayer` runs on csrc/point_transformer.hip
    (`adaptpoint_amd.pt_layer`); what the kernels do not cover -- and a layer that carries a forward hook, which the
    kernels would skip -- runs composed with a `set_abstraction.FUSED_FALLBACKS` entry that says which; CPU tensors
    run composed without one.

`PTSeg(block=...)` takes the class or its name ('PointTransformerBlock', 'EdgeConvBlock').  The EdgeConv-style blocks
are composed only.
"""
import torch
import torch.nn as nn

from . import pointops

_FAR = 1e10                     # the padding distance of a cloud shorter than k (pointops.py)
_MAX_ROWS = 2 ** 24
PT_WIDTHS = (32, 64, 128, 256, 512)
PT_K_MAX = 32
PT_SHARE = 8

knn_hook = None                 # callable(who, k, n, m): told of every kNN query this module issues ('stage' | 'down')


def _on_kernels(*ts):
    return all(t.is_cuda and t.dtype == torch.float32 for t in ts)


# ------------------------------------------------------------------------------------- the five operators
@torch.no_grad()
def _knn_torch(k, p, q, o, qo):
    """idx (m,k) int32, dist2 (m,k): per cloud the k smallest (d2, row), ascending; short clouds pad."""
    n, m = p.shape[0], q.shape[0]
    idx = torch.zeros(m, k, dtype=torch.int32, device=p.device)
    d2 = torch.full((m, k), _FAR, dtype=p.dtype, device=p.device)
    ends, qends = o.tolist(), qo.tolist()
    for s, e, qs, qe in zip([0] + ends[:-1], ends, [0] + qends[:-1], qends):
        if qe <= qs:
            continue
        idx[qs:qe] = min(s, n - 1)
        if e <= s:
            continue
        t = q[qs:qe, None, :] - p[None, s:e, :]
        d, order = torch.sort((t * t).sum(-1), dim=1, stable=True)        # ties: ascending row
        kk = min(k, e - s)
        idx[qs:qe, :kk] = (order[:, :kk] + s).int()
        d2[qs:qe, :kk] = d[:, :kk]
    return idx, d2


@torch.no_grad()
def _fps_torch(p, o, n_o):
    """idx (m) int32: per cloud its first point, then the point farthest from everything picked (first maximum)."""
    ends, nends = o.tolist(), n_o.tolist()
    out = torch.zeros(nends[-1], dtype=torch.int32, device=p.device)
    for s, e, ms, me in zip([0] + ends[:-1], ends, [0] + nends[:-1], nends):
        if me <= ms:
            continue
        out[ms:me] = s
        if e <= s:
            continue
        dist = torch.full((e - s,), _FAR, dtype=p.dtype, device=p.device)
        old = 0
        for j in range(ms + 1, me):
            t = p[s:e] - p[s + old]
            dist = torch.minimum(dist, (t * t).sum(-1))
            old = int(torch.argmax(dist))
            out[j] = s + old
    return out


def knn(k, p, q, o, qo, who='stage'):
    """idx (m,k) int32 and dist (m,k) of the queries q among p."""
    if knn_hook is not None:
        knn_hook(who, k, p.shape[0], q.shape[0])
    if _on_kernels(p, q):
        return pointops.knnquery(k, p.contiguous(), q.contiguous(), o, qo)
    idx, d2 = _knn_torch(k, p, q, o, qo)
    return idx, torch.sqrt(d2)


def furthest_sampling(p, o, n_o):
    if _on_kernels(p):
        return pointops.furthestsampling(p.contiguous(), o, n_o)
    return _fps_torch(p, o, n_o)


def group(x, idx):
    """x (n,c), idx (m,k) -> (m,k,c)."""
    if _on_kernels(x):
        return pointops.grouping(x.contiguous(), idx)
    return x[idx.long()]


def interpolate(p2, p1, x2, o2, o1, idx=None):
    """Inverse-distance interpolation (k = 3) of x2 at p2 onto p1 -> ((n1,c), idx (n1,3)); idx: the neighbours to use
    (the torch statement only: the kernels query their own, which for equal float32 points are the same)."""
    if _on_kernels(p2, p1, x2):
        return pointops.interpolation(p2.contiguous(), p1.contiguous(), x2.contiguous(), o2, o1), idx
    if idx is None:
        idx, dist = knn(3, p2, p1, o2, o1, who='up')
    else:
        with torch.no_grad():
            t = p2[idx.long()] - p1[:, None, :]
            dist = torch.sqrt((t * t).sum(-1))
            ends, qends = o2.tolist(), o1.tolist()
            for s, e, qs, qe in zip([0] + ends[:-1], ends, [0] + qends[:-1], qends):
                if 0 <= e - s < idx.shape[1] and qe > qs:          # the slots a short coarse cloud pads
                    dist[qs:qe, e - s:] = _FAR ** 0.5
    recip = 1.0 / (dist + 1e-8)
    weight = recip / recip.sum(1, keepdim=True)
    out = torch.zeros(p1.shape[0], x2.shape[1], dtype=x2.dtype, device=x2.device)
    for i in range(idx.shape[1]):
        out = out + x2[idx[:, i].long(), :] * weight[:, i].unsqueeze(-1)
    return out, idx


class StageGraph:
    """The neighbour graph all layers of one level share: idx (n,k) int32 and, lazily, d (n,k,3) = the neighbours'
    offsets, which carry no gradient.  The reverse lists the backward passes walk are cached on `idx` by
    `pointops.csr_of`.  `StageGraph.builds` counts the graphs built (one kNN query each)."""
    builds = 0

    def __init__(self, p, o, nsample, idx=None):
        if idx is None:
            idx, _ = knn(nsample, p.detach(), p.detach(), o, o)
            StageGraph.builds += 1
        if idx.shape != (p.shape[0], nsample):
            raise ValueError(f"StageGraph: idx {tuple(idx.shape)} is not ({p.shape[0]}, {nsample})")
        self.p, self.o, self.idx, self.nsample = p.detach(), o, idx, nsample
        self._d = None

    @property
    def d(self):
        if self._d is None:
            with torch.no_grad():
                self._d = (group(self.p, self.idx) - self.p.unsqueeze(1)).contiguous()
        return self._d

    def csr(self):
        return pointops.csr_of(self.idx, self.p.shape[0])


def _unpack(pxo, nsample):
    """[p, x, o] or [p, x, o, graph] -> p, x, o, the graph to use, whether it was handed in."""
    p, x, o = pxo[:3]
    g = pxo[3] if len(pxo) > 3 else None
    if g is not None and g.nsample != nsample:
        raise ValueError(f"the stage's graph has {g.nsample} neighbours, the layer takes {nsample}")
    return p, x, o, (StageGraph(p, o, nsample) if g is None else g), g is not None


def _channel_bn(layer, t):
    """BatchNorm1d over the channels of t (n,k,c), as the reference applies it: on the (n,c,k) transpose."""
    return layer(t.transpose(1, 2).contiguous()).transpose(1, 2).contiguous()


# --------------------------------------------------------------------------------------------------- layers
def pt_layer_covers(device_type, dtype, contiguous, in_planes, out_planes, share_planes, k, n):
    """Whether csrc/point_transformer.hip covers a layer call, on plain values: float32 CUDA contiguous inputs,
    in_planes == out_planes in PT_WIDTHS, share_planes 8, 1 <= k <= 32, n < 2^24."""
    return (device_type == 'cuda' and dtype == torch.float32 and bool(contiguous) and in_planes == out_planes
            and out_planes in PT_WIDTHS and share_planes == PT_SHARE and 1 <= k <= PT_K_MAX and 1 <= n < _MAX_ROWS)


def _bn_relu(width):
    return [nn.BatchNorm1d(width), nn.ReLU(inplace=True)]


class PointTransformerLayer(nn.Module):
    """Vector attention over the k neighbours of every row.  State: `linear_q/k/v`, `linear_p` (Linear(3,3), BN, ReLU,
    Linear(3,C): the positional term) and `linear_w` (BN, ReLU, Linear(C,C/share), BN, ReLU, Linear: the weights)."""

    def __init__(self, in_planes, out_planes, share_planes=8, nsample=16, fused=False):
        super().__init__()
        width, shared = out_planes, out_planes // share_planes
        self.mid_planes = self.out_planes = width
        self.share_planes, self.nsample, self.fused = share_planes, nsample, fused
        self.linear_q, self.linear_k, self.linear_v = (nn.Linear(in_planes, width) for _ in range(3))
        self.linear_p = nn.Sequential(nn.Linear(3, 3), *_bn_relu(3), nn.Linear(3, width))
        self.linear_w = nn.Sequential(*_bn_relu(width), nn.Linear(width, shared), *_bn_relu(shared),
                                      nn.Linear(shared, shared))

    def _uncovered(self, p, x):
        """None when csrc/point_transformer.hip takes this call, else the reason it does not."""
        what = (f"PointTransformerLayer C={self.linear_q.in_features} -> {self.out_planes}, share {self.share_planes}, "
                f"k={self.nsample}, {x.dtype}")
        if any(m._forward_hooks or m._forward_pre_hooks for m in self.modules()):
            return what + ": a forward hook is attached to the layer or one of its modules (the kernels would skip it)"
        bns = (self.linear_w[0], self.linear_w[3])
        ok = pt_layer_covers(x.device.type, x.dtype, x.is_contiguous() and p.is_contiguous(), self.linear_q.in_features,
                             self.out_planes, self.share_planes, self.nsample, x.shape[0])
        ok = ok and all(b.affine and b.momentum is not None and (b.training or b.track_running_stats) for b in bns)
        return None if ok else what + ": no fused kernel for this layer"

    def _composed(self, x, graph):
        idx = graph.idx
        q = self.linear_q(x)
        k_nb, v_nb = group(self.linear_k(x), idx), group(self.linear_v(x), idx)           # (n, k, C) each
        lin0, bn0, act0, lin1 = self.linear_p
        pos = lin1(act0(_channel_bn(bn0, lin0(graph.d.to(x.dtype)))))                      # (n, k, C)
        bn1, act1, lin2, bn2, act2, lin3 = self.linear_w
        hidden = lin2(act1(_channel_bn(bn1, k_nb - q[:, None, :] + pos)))                  # (n, k, C / share)
        attn = torch.softmax(lin3(act2(_channel_bn(bn2, hidden))), dim=1)                  # over the k slots
        n, k, width = v_nb.shape
        shares = (v_nb + pos).reshape(n, k, self.share_planes, -1) * attn[:, :, None, :]   # channel c: weight c mod C/share
        return shares.sum(1).reshape(n, width)

    def forward(self, pxo):
        p, x, o, graph, _ = _unpack(pxo, self.nsample)
        if self.fused and x.is_cuda:
            from . import pt_layer
            from .set_abstraction import _note_fallback
            reason = self._uncovered(p, x)
            if reason is None:
                return pt_layer.point_transformer_layer(self, x, graph)
            _note_fallback(reason)
        return self._composed(x, graph)


class EdgeConvLayer(nn.Module):
    """max_k conv([x_j - x_i ; x_i]) with Conv2d(2C, H, 1) - BatchNorm2d - LeakyReLU(0.2); `linear_q` is state the
    reference carries without using it."""

    def __init__(self, in_planes, out_planes, share_planes=8, nsample=16):
        super().__init__()
        self.mid_planes = self.out_planes = out_planes
        self.share_planes, self.nsample = share_planes, nsample
        self.linear_q = nn.Linear(in_planes, out_planes)
        self.conv = nn.Sequential(nn.Conv2d(2 * in_planes, out_planes, kernel_size=1, bias=False),
                                  nn.BatchNorm2d(out_planes), nn.LeakyReLU(negative_slope=0.2))

    def forward(self, pxo):
        p, x, o, graph, _ = _unpack(pxo, self.nsample)
        centre = x[:, None, :].expand(-1, self.nsample, -1)
        edges = torch.cat((group(x, graph.idx) - centre, centre), dim=-1)                  # (n, k, 2C)
        y = self.conv(edges.permute(2, 0, 1).contiguous()[None])                           # (1, H, n, k)
        return y.max(dim=-1)[0][0].t().contiguous()


class PointNet2EdgeConvLayer(nn.Module):
    """max_k conv([p_j - p_i ; x_j]) with Conv1d(3 + C, H, 1) - BatchNorm1d - ReLU."""

    def __init__(self, in_planes, out_planes, share_planes=8, nsample=16):
        super().__init__()
        self.mid_planes = self.out_planes = out_planes
        self.nsample = nsample
        self.conv = nn.Sequential(nn.Conv1d(3 + in_planes, out_planes, kernel_size=1, bias=False), *_bn_relu(out_planes))

    def forward(self, pxo):
        p, x, o, graph, _ = _unpack(pxo, self.nsample)
        grouped = torch.cat((graph.d.to(x.dtype), group(x, graph.idx)), dim=-1)            # (n, k, 3 + C)
        return self.conv(grouped.transpose(1, 2).contiguous()).max(dim=-1)[0]


def _cloud_sizes(o):
    """The clouds' row counts from the cumulative ends (one host read)."""
    ends = o.tolist()
    return [e - s for s, e in zip([0] + ends[:-1], ends)]


class TransitionDown(nn.Module):
    """stride 1: Linear - BN - ReLU on the rows.  Otherwise every cloud keeps size // stride furthest-sampled points,
    each the max over its nsample neighbours of Linear(3 + C) - BN - ReLU of [offset ; feature]."""

    def __init__(self, in_planes, out_planes, stride=1, nsample=16):
        super().__init__()
        strided = stride != 1
        self.stride = stride
        self.nsample = nsample
        self.linear = nn.Linear(in_planes + 3 * strided, out_planes, bias=False)
        if strided:
            self.pool = nn.MaxPool1d(nsample)
        self.bn = nn.BatchNorm1d(out_planes)
        self.relu = nn.ReLU(inplace=True)
        self.last_graph = None

    def forward(self, pxo, graph=None):
        """graph: (sampled index (m), group index (m,nsample)) to use instead of sampling and querying; the pair used
        is kept in `last_graph`.  Returns a 3-list: a stage graph handed in is dropped with the point set."""
        p, x, o = pxo[:3]
        if self.stride == 1:
            return [p, self.relu(self.bn(self.linear(x))), o]
        kept = [size // self.stride for size in _cloud_sizes(o)]
        new_o = torch.tensor(kept, device=o.device).cumsum(0).to(torch.int32)
        if graph is None:
            sampled = furthest_sampling(p, o, new_o)
            new_p = p[sampled.long()].contiguous()
            nb, _ = knn(self.nsample, p.detach(), new_p.detach(), o, new_o, who='down')
        else:
            sampled, nb = graph
            new_p = p[sampled.long()].contiguous()
        self.last_graph = (sampled, nb)
        with torch.no_grad():
            offsets = group(p.detach(), nb) - new_p.detach()[:, None, :]
        y = self.linear(torch.cat((offsets.to(x.dtype), group(x, nb)), dim=-1))           # (m, k, H)
        y = self.relu(self.bn(y.transpose(1, 2).contiguous()))                             # (m, H, k)
        return [new_p, self.pool(y)[..., 0], new_o]


class TransitionUp(nn.Module):
    """The decoder's entry.  Head (out_planes None): every row joined with linear2 of its cloud's mean row, through
    linear1.  Otherwise linear1 of the fine rows plus linear2 of the coarse rows interpolated onto them (k = 3)."""

    def __init__(self, in_planes, out_planes=None):
        super().__init__()
        head = out_planes is None
        width = in_planes if head else out_planes
        self.linear1 = nn.Sequential(nn.Linear(2 * in_planes if head else width, width), *_bn_relu(width))
        self.linear2 = nn.Sequential(nn.Linear(in_planes, width), *(_bn_relu(width)[1:] if head else _bn_relu(width)))
        self.last_idx = None

    def forward(self, pxo1, pxo2=None, idx=None):
        """idx (n1,3): the interpolation's neighbours for the torch statement (see `interpolate`); kept in `last_idx`."""
        p1, x1, o1 = pxo1[:3]
        if pxo2 is None:
            sizes = _cloud_sizes(o1)
            # (linear2 cloud by cloud, as the reference applies it: a batched product rounds differently, and the
            # BatchNorms over the few rows of the deep levels amplify that beyond the golden's bar)
            context = [self.linear2(rows.sum(0, keepdim=True) / len(rows)).expand(len(rows), -1) for rows in x1.split(sizes)]
            return self.linear1(torch.cat((x1, torch.cat(context)), dim=1))
        p2, x2, o2 = pxo2[:3]
        up, self.last_idx = interpolate(p2, p1, self.linear2(x2), o2, o1, idx)
        return self.linear1(x1) + up


class _ResidualBlock(nn.Module):
    """Linear - BN - ReLU, a local aggregation on the level's graph, Linear - BN, the residual, ReLU.  A subclass names
    its aggregation module and says what follows it."""
    expansion = 1

    def _ends(self, in_planes, planes):
        self.linear1, self.bn1 = nn.Linear(in_planes, planes, bias=False), nn.BatchNorm1d(planes)

    def _tail(self, planes):
        self.linear3 = nn.Linear(planes, planes * self.expansion, bias=False)
        self.bn3 = nn.BatchNorm1d(planes * self.expansion)
        self.relu = nn.ReLU(inplace=True)


class PointTransformerBlock(_ResidualBlock):
    def __init__(self, in_planes, planes, share_planes=8, nsample=16, fused=False, **kwargs):
        super().__init__()
        self._ends(in_planes, planes)
        self.transformer2 = PointTransformerLayer(planes, planes, share_planes, nsample, fused=fused)
        self.bn2 = nn.BatchNorm1d(planes)
        self._tail(planes)

    def forward(self, pxo):
        p, x, o, graph, handed = _unpack(pxo, self.transformer2.nsample)
        y = self.relu(self.bn1(self.linear1(x)))
        y = self.relu(self.bn2(self.transformer2([p, y, o, graph])))
        y = self.relu(self.bn3(self.linear3(y)) + x)
        return [p, y, o, graph] if handed else [p, y, o]


class EdgeConvBlock(_ResidualBlock):
    def __init__(self, in_planes, planes, share_planes=8, nsample=16, mid_res=False, fused=False):
        super().__init__()
        self._ends(in_planes, planes)
        self.local_aggr = PointNet2EdgeConvLayer(planes, planes, share_planes, nsample)
        self._tail(planes)
        self.mid_res = mid_res                     # the residual leaves behind linear1 instead of in front of it

    def forward(self, pxo):
        p, x, o, graph, handed = _unpack(pxo, self.local_aggr.nsample)
        y = self.relu(self.bn1(self.linear1(x)))
        skip = y if self.mid_res else x
        y = self.bn3(self.linear3(self.local_aggr([p, y, o, graph])))
        y = self.relu(y + skip)
        return [p, y, o, graph] if handed else [p, y, o]


BLOCKS = {'PointTransformerBlock': PointTransformerBlock, 'EdgeConvBlock': EdgeConvBlock}
STRIDES = (1, 4, 4, 4, 4)
SHARE_PLANES = 8


class PTSeg(nn.Module):
    """Five encoder stages enc1..enc5 (a `TransitionDown`, then blocks[i] - 1 blocks) and five decoder stages dec5..dec1
    (a `TransitionUp`, then one block when dec_local_aggr) at widths width * 2^i, and the head `cls`."""
    keep_graphs = False        # keep every forward's graphs in last_graphs (as the keep_graphs argument does for one call)
    last_graphs = None

    def __init__(self, block, blocks, width=32, nsample=[8, 16, 16, 16, 16], in_channels=6, num_classes=13,
                 dec_local_aggr=True, mid_res=False, fused=False):
        super().__init__()
        if isinstance(block, str):
            if block not in BLOCKS:
                raise ValueError(f"PTSeg: block '{block}' is not one of {sorted(BLOCKS)}")
            block = BLOCKS[block]
        self.nsample = list(nsample)
        self.mid_res, self.dec_local_aggr, self.fused = mid_res, dec_local_aggr, fused
        widths = [width * 2 ** i * block.expansion for i in range(len(blocks))]

        def members(first, planes, count, k):
            return nn.Sequential(first, *(block(planes, planes, SHARE_PLANES, nsample=k, mid_res=mid_res, fused=fused)
                                          for _ in range(count)))
        coming = in_channels
        for i, planes in enumerate(widths):
            down = TransitionDown(coming, planes, STRIDES[i], self.nsample[i])
            setattr(self, f"enc{i + 1}", members(down, planes, blocks[i] - 1, self.nsample[i]))
            coming = planes
        for i in reversed(range(len(widths))):
            up = TransitionUp(coming, None if i == len(widths) - 1 else widths[i])
            setattr(self, f"dec{i + 1}", members(up, widths[i], 1 if dec_local_aggr else 0, self.nsample[i]))
            coming = widths[i]
        self.cls = nn.Sequential(nn.Linear(widths[0], widths[0]), *_bn_relu(widths[0]), nn.Linear(widths[0], num_classes))

    def forward(self, p0, x0=None, o0=None, graphs=None, keep_graphs=False):
        """p0 (n,3), x0 (n,c), o0 (b) int32 -- or the reference's dict {'pos', 'x', 'o'} -- -> logits (n,num_classes).
        graphs: a `last_graphs` dict to run on instead of sampling and querying."""
        if o0 is None:
            batch = p0
            p0, x0, o0 = batch['pos'], batch.get('x'), batch['o']
        x0 = p0 if x0 is None else x0
        if graphs is not None and (len(graphs['stage']) != 5 or len(graphs['down']) != 4 or len(graphs['up']) != 4):
            raise ValueError("PTSeg: graphs holds 5 stage graphs, 4 (sample, group) pairs and 4 interpolation indices")
        keep = keep_graphs or self.keep_graphs
        pxo, lv, stage = [p0, x0, o0], [], []
        for i in range(5):
            enc = getattr(self, f"enc{i + 1}")
            given = graphs['down'][i - 1] if graphs is not None and i > 0 else None
            p, x, o = enc[0](pxo, given)
            g = StageGraph(p, o, self.nsample[i], None if graphs is None else graphs['stage'][i])
            stage.append(g)
            pxo = enc[1:]([p, x, o, g])[:3]
            lv.append(pxo)
        up = [None] * 4
        for i in range(4, -1, -1):
            dec = getattr(self, f"dec{i + 1}")
            if i == 4:
                x = dec[0](lv[4])
            else:
                x = dec[0](lv[i], lv[i + 1], None if graphs is None else graphs['up'][i])
                up[i] = dec[0].last_idx
                if up[i] is None and keep:                   # the kernels query inside: once more, to keep it
                    up[i], _ = knn(3, lv[i + 1][0].detach(), lv[i][0].detach(), lv[i + 1][2], lv[i][2], who='up')
            x = dec[1:]([lv[i][0], x, lv[i][2], stage[i]])[1]
            lv[i] = [lv[i][0], x, lv[i][2]]
        self.last_graphs = None
        if keep:
            self.last_graphs = {'stage': [g.idx for g in stage],
                                'down': [getattr(self, f"enc{i + 1}")[0].last_graph for i in range(1, 5)], 'up': up}
        return self.cls(lv[0][1])
