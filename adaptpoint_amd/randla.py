"""RandLA-Net (openpoints/models/backbone/randlenet.py) on the gfx950 kernels.

`SharedMLP`, `LocalSpatialEncoding`, `AttentivePooling`, `LocalFeatureAggregation` and `RandLANet` keep the reference's
names, constructor arguments and parameter names -- the `ConvTranspose2d` decoder weights of shape (in,out,1,1) and the
full 2C x 2C `score_fn.0.weight` included -- so a reference `state_dict` loads unchanged.  Called as the reference calls
them they run the reference's operator sequence in PyTorch on whatever device the tensors live on (the composed path);
the graphs come from `layers.knn_query` on the GPU (a sorted direct-difference statement on the CPU), once per encoder
level, shared by both `lse` layers of the block, and never through the host.

fused=True (`RandLANet(..., fused=True)`) runs `LocalSpatialEncoding` + the score / softmax / sum of `AttentivePooling`
as ONE layer on csrc/randla.hip:

    h_k = relu(W' (e_k - mu) + b'),   pooled = [ sum_k softmax_k(A_hh h_k) * h_k ; f ]

with e_k = [p_n, p_j, p_n - p_j, dist], W' / b' / mu the BatchNorm folded into the 10 -> C convolution, A_hh the top-left
C x C block of `score_fn.0.weight` and f the centre's features.  The other three blocks of the score weight multiply a
term that is constant over the K neighbours: it cancels in the softmax, so they receive EXACT ZERO gradients on this
path (the composed path gives them rounding noise around zero), and so does the convolution bias in front of a
training-mode BatchNorm.  The BatchNorm's batch statistics follow from the 10 sums and 55 products of e over all pairs:
one moment pass per block serves both layers.  No (B,C,N,K) tensor exists, forward or backward.

On the fused path the per-point layers (mlp1, mlp2, shortcut, the pool MLPs, the decoder, fc_end) run their convolution
+ bias on `pointwise.conv_bias_act` and their BatchNorm / LeakyReLU on PyTorch; `fc_start` is PyTorch's linear layer.
The point shuffle is a gather both ways (its inverse permutation) and the decoder's nearest-coarse-point copy is
`pointops.grouping` (reverse lists, no atomics): forward + backward with a supplied device permutation captures into a
hipGraph and replays to the same bits.

Limits: those of `knn_query` (B * N < 2^24, K <= 64); the fused layer takes C in {8, 16, 32, 64, 128} and K <= 32.  A
layer outside them runs composed with a `set_abstraction.FUSED_FALLBACKS` entry that says why; CPU tensors run
composed without one.

`dist`: 'squared' (the default) hands the encoding the squared distance `knn_query` returns, 'euclidean' its root.  The
reference takes the value from `torch_points_kernels.knn`; which of the two that library returns was NOT verified
(INTEGRATION.md).
"""
import torch
import torch.nn as nn

from . import batchnorm

RL_WIDTHS = (8, 16, 32, 64, 128)
RL_K_MAX = 32
_MAX_POINTS = 2 ** 24


# ---------------------------------------------------------------------------------------------------- graphs
def _knn_torch(support, query, k):
    """`knn_query`'s statement in torch for tensors the kernel does not take (CPU, float64): squared distances by
    direct differences, the k smallest keys (distance, index) ascending, ties to the smaller index."""
    idx, d2 = [], []
    for s, q in zip(support, query):
        d = ((q[:, None, :] - s[None, :, :]) ** 2).sum(-1)
        v, i = torch.sort(d, dim=-1, stable=True)
        idx.append(i[:, :k])
        d2.append(v[:, :k])
    return torch.stack(idx).to(torch.int32), torch.stack(d2)


@torch.no_grad()
def knn_graph(support, query, k):
    """-> (idx (B,M,k) int32, squared distances (B,M,k)) of the k nearest `support` rows of every `query` row."""
    from . import layers
    support, query = support.contiguous(), query.contiguous()
    if k > support.shape[1]:
        raise ValueError(f"RandLANet: {k} neighbours asked of {support.shape[1]} points")
    if support.is_cuda and support.dtype == torch.float32:
        if not layers.knn_covers(support, query, k):
            raise ValueError(f"RandLANet: knn_query does not take support {tuple(support.shape)} / query "
                             f"{tuple(query.shape)} with k = {k} (B * N < 2^24, k <= {layers.KNN_MAX_K})")
        return layers.knn_query(support, query, k, return_dist=True)
    return _knn_torch(support, query, k)


# ---------------------------------------------------------------------------------------------------- modules
class SharedMLP(nn.Module):
    def __init__(self, in_channels, out_channels, kernel_size=1, stride=1, transpose=False, padding_mode='zeros',
                 bn=False, activation_fn=None):
        super().__init__()
        conv_fn = nn.ConvTranspose2d if transpose else nn.Conv2d
        self.conv = conv_fn(in_channels, out_channels, kernel_size, stride=stride, padding_mode=padding_mode)
        self.batch_norm = nn.BatchNorm2d(out_channels, eps=1e-6, momentum=0.99) if bn else None
        self.activation_fn = activation_fn

    def forward(self, input):
        """input (B, d_in, N, K) -> (B, d_out, N, K)."""
        x = self.conv(input)
        if self.batch_norm:
            x = self.batch_norm(x)
        if self.activation_fn:
            x = self.activation_fn(x)
        return x


def _per_point(mlp, x, fused):
    """`mlp(x)` for x (B, C, N, 1); fused: the convolution + bias on the contraction kernels (csrc/pointwise.hip)."""
    conv = mlp.conv
    one = lambda t, v: all(s == v for s in t)
    if not (fused and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[3] == 1
            and 0 < x.shape[0] <= 65535 and x.shape[2] > 0 and one(conv.kernel_size, 1) and one(conv.stride, 1)
            and one(conv.padding, 0) and conv.groups == 1 and conv.weight.dtype == torch.float32
            and not (mlp._forward_hooks or mlp._forward_pre_hooks or conv._forward_hooks or conv._forward_pre_hooks)):
        return mlp(x)
    from . import pointwise
    w = conv.weight[:, :, 0, 0]
    if isinstance(conv, nn.ConvTranspose2d):
        w = w.t()
    relu = mlp.batch_norm is None and isinstance(mlp.activation_fn, nn.ReLU)
    y = pointwise.conv_bias_act(x.squeeze(3).contiguous(), w, conv.bias, relu=relu).unsqueeze(3)
    if mlp.batch_norm:
        y = mlp.batch_norm(y)
    if mlp.activation_fn and not relu:
        y = mlp.activation_fn(y)
    return y


class LocalSpatialEncoding(nn.Module):
    def __init__(self, d, num_neighbors, device):
        super().__init__()
        self.num_neighbors = num_neighbors
        self.mlp = SharedMLP(10, d, bn=True, activation_fn=nn.ReLU())
        self.device = device

    def forward(self, coords, features, knn_output):
        """coords (B,N,3), features (B,d,N,1), knn_output (idx (B,N,K), dist (B,N,K)) -> (B, 2d, N, K)."""
        idx, dist = knn_output
        B, N, K = idx.size()
        extended_idx = idx.long().unsqueeze(1).expand(B, 3, N, K)
        extended_coords = coords.transpose(-2, -1).unsqueeze(-1).expand(B, 3, N, K)
        neighbors = torch.gather(extended_coords, 2, extended_idx)
        concat = torch.cat((extended_coords, neighbors, extended_coords - neighbors, dist.unsqueeze(-3)), dim=-3)
        return torch.cat((self.mlp(concat), features.expand(B, -1, N, K)), dim=-3)


class AttentivePooling(nn.Module):
    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.score_fn = nn.Sequential(nn.Linear(in_channels, in_channels, bias=False), nn.Softmax(dim=-2))
        self.mlp = SharedMLP(in_channels, out_channels, bn=True, activation_fn=nn.ReLU())

    def pooled(self, x):
        """x (B, d_in, N, K) -> (B, d_in, N, 1): the score-weighted sum over the neighbours."""
        scores = self.score_fn(x.permute(0, 2, 3, 1)).permute(0, 3, 1, 2)
        return torch.sum(scores * x, dim=-1, keepdim=True)

    def forward(self, x):
        """x (B, d_in, N, K) -> (B, d_out, N, 1)."""
        return self.mlp(self.pooled(x))


# ---------------------------------------------------------------------------------------------------- the fused layer
def encoding_moments(coords, idx, dist2, sqrt_dist):
    """The 10 sums and 55 products (float64, (65,)) of the encoding over all B N K pairs (apn_rl_moments)."""
    from . import _lib
    from .fused import _call
    B, N, K = idx.shape
    dev = coords.device
    part = torch.empty(max(1, _lib.load().apn_rl_moment_rows(B, N, K)), 65, dtype=torch.float64, device=dev)
    mom = torch.empty(65, dtype=torch.float64, device=dev)
    _call("apn_rl_moments", dev, B, N, K, coords.data_ptr(), idx.data_ptr(), dist2.data_ptr(), int(sqrt_dist),
          part.data_ptr(), mom.data_ptr())
    return mom


class _EncodePool(torch.autograd.Function):
    """pooled (B,C,N) of one lse + score + sum layer; gradients for the convolution, its BatchNorm and the score weight."""

    @staticmethod
    def forward(ctx, coords, idx, dist2, w, b, gamma, beta, A, bn, mom, sqrt_dist):
        from .fused import _call, _ptr
        dev = coords.device
        B, N, K = idx.shape
        C = w.shape[0]
        bna = batchnorm.args(bn)
        training = bool(bna.training)
        f32 = dict(dtype=torch.float32, device=dev)
        with torch.no_grad():
            w2 = w.detach().reshape(C, 10).contiguous()
            wf = torch.empty(11 * C + 10, **f32)
            stat = torch.empty(3 * C, dtype=torch.float64, device=dev)
            _call("apn_rl_fold", dev, C, _ptr(mom) if training else None, float(B * N * K), w2.data_ptr(), _ptr(b),
                  _ptr(gamma), _ptr(beta), bna.eps, bna.momentum, bna.training, bna.running_mean, bna.running_var,
                  bna.num_batches_tracked, wf.data_ptr(), stat.data_ptr())
            a = A.detach()[:C, :C].contiguous()
            at = A.detach()[:C, :C].t().contiguous()
            pooled = torch.empty(B, C, N, **f32)
            _call("apn_rl_forward", dev, B, N, K, C, coords.data_ptr(), idx.data_ptr(), dist2.data_ptr(),
                  int(sqrt_dist), wf.data_ptr(), at.data_ptr(), pooled.data_ptr())
        ctx.save_for_backward(coords, idx, dist2, wf, a, at, stat, mom if training else None, w2, b, gamma)
        ctx.cfg = (training, int(sqrt_dist), w.shape, A.shape, beta is not None)
        return pooled

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        from . import _lib, ops
        from .fused import _call, _ptr
        coords, idx, dist2, wf, a, at, stat, mom, w2, b, gamma = ctx.saved_tensors
        training, sqrt_dist, wshape, ashape, has_beta = ctx.cfg
        dev = coords.device
        B, N, K = idx.shape
        C = w2.shape[0]
        g = g.float().contiguous()
        rows = _lib.load().apn_rl_bwd_rows(B, N, K, C)
        part = torch.empty(max(1, rows), C * C + 11 * C, dtype=torch.float32, device=dev)
        _call("apn_rl_backward", dev, B, N, K, C, coords.data_ptr(), idx.data_ptr(), dist2.data_ptr(), sqrt_dist,
              wf.data_ptr(), a.data_ptr(), at.data_ptr(), g.data_ptr(), part.data_ptr())
        grads = torch.empty(C * C + 13 * C, dtype=torch.float32, device=dev)
        sums = torch.empty(C * C + 11 * C, dtype=torch.float64, device=dev)
        _call("apn_rl_finalize", dev, C, rows, part.data_ptr(), _ptr(mom), float(B * N * K), w2.data_ptr(), _ptr(b),
              _ptr(gamma), stat.data_ptr(), int(training), sums.data_ptr(), grads.data_ptr())
        cc = C * C
        dA = ops.zeros(*ashape, dtype=torch.float32, device=dev)          # the three dead blocks: exact zeros
        dA[:C, :C] = grads[:cc].view(C, C)
        return (None, None, None, grads[cc + 2 * C:cc + 12 * C].reshape(wshape),
                grads[cc + 12 * C:] if b is not None else None, grads[cc:cc + C] if gamma is not None else None,
                grads[cc + C:cc + 2 * C] if has_beta else None, dA, None, None, None)


def fused_layer_reason(lse, pool, coords, idx):
    """Why the kernels do not take this layer (None: they do).  Attribute and shape checks only."""
    mlp, bn, lin = lse.mlp, lse.mlp.batch_norm, pool.score_fn[0]
    C, K = mlp.conv.out_channels, idx.shape[-1]
    if not (coords.is_cuda and coords.dtype == torch.float32 and mlp.conv.weight.dtype == torch.float32):
        return "RandLA layer: tensors are not float32 on the GPU"
    if C not in RL_WIDTHS:
        return f"RandLA layer: width {C} is not one of {RL_WIDTHS}"
    if not 1 <= K <= RL_K_MAX:
        return f"RandLA layer: K = {K} is beyond the fused layer's {RL_K_MAX}"
    if coords.shape[0] * coords.shape[1] >= _MAX_POINTS:
        return "RandLA layer: B * N >= 2^24"
    if not (isinstance(mlp.conv, nn.Conv2d) and mlp.conv.in_channels == 10 and isinstance(bn, nn.BatchNorm2d)
            and isinstance(mlp.activation_fn, nn.ReLU) and tuple(lin.weight.shape) == (2 * C, 2 * C) and lin.bias is None):
        return "RandLA layer: not the reference's lse / pool structure"
    if bn.momentum is None or not (bn.training or bn.track_running_stats):
        return "RandLA layer: BatchNorm without a numeric momentum or without statistics"
    mods = (lse, mlp, mlp.conv, bn, pool.score_fn, lin)
    if any(m._forward_hooks or m._forward_pre_hooks for m in mods):
        return "RandLA layer: a forward hook sits on a module the kernels would skip"
    return None


def encode_pool(lse, pool, coords, features, idx, dist2, mom, sqrt_dist):
    """[pooled ; f] (B, 2C, N, 1) of `pool.pooled(lse(coords, features, (idx, dist)))` on csrc/randla.hip."""
    mlp, bn = lse.mlp, lse.mlp.batch_norm
    pooled = _EncodePool.apply(coords, idx, dist2, mlp.conv.weight, mlp.conv.bias, bn.weight, bn.bias,
                               pool.score_fn[0].weight, bn, mom, sqrt_dist)
    return torch.cat((pooled.unsqueeze(3), features), dim=1)


class LocalFeatureAggregation(nn.Module):
    def __init__(self, d_in, d_out, num_neighbors, device, fused=False, dist='squared'):
        super().__init__()
        if dist not in ('squared', 'euclidean'):
            raise ValueError(f"LocalFeatureAggregation: dist must be 'squared' or 'euclidean', got {dist!r}")
        self.num_neighbors, self.fused, self.dist = num_neighbors, fused, dist

        self.mlp1 = SharedMLP(d_in, d_out // 2, activation_fn=nn.LeakyReLU(0.2))
        self.mlp2 = SharedMLP(d_out, 2 * d_out)
        self.shortcut = SharedMLP(d_in, 2 * d_out, bn=True)

        self.lse1 = LocalSpatialEncoding(d_out // 2, num_neighbors, device)
        self.lse2 = LocalSpatialEncoding(d_out // 2, num_neighbors, device)

        self.pool1 = AttentivePooling(d_out, d_out // 2)
        self.pool2 = AttentivePooling(d_out, d_out)

        self.lrelu = nn.LeakyReLU()

    def forward(self, coords, features, graph=None):
        """coords (B,N,3), features (B,d_in,N,1) -> (B, 2 d_out, N, 1); graph: (idx, squared distances) of the level."""
        coords = coords.contiguous()
        idx, dist2 = knn_graph(coords, coords, self.num_neighbors) if graph is None else graph
        fused = self.fused and features.is_cuda
        reason = None
        if fused:
            reason = (fused_layer_reason(self.lse1, self.pool1, coords, idx)
                      or fused_layer_reason(self.lse2, self.pool2, coords, idx))
            if reason is not None:
                from .set_abstraction import _note_fallback
                _note_fallback(reason)
        x = _per_point(self.mlp1, features, fused)
        if fused and reason is None:
            root = self.dist == 'euclidean'
            bns = (self.lse1.mlp.batch_norm, self.lse2.mlp.batch_norm)
            mom = (encoding_moments(coords, idx, dist2, root)
                   if any(batchnorm.mode(bn)[0] for bn in bns) else None)
            x = _per_point(self.pool1.mlp, encode_pool(self.lse1, self.pool1, coords, x, idx, dist2, mom, root), True)
            x = _per_point(self.pool2.mlp, encode_pool(self.lse2, self.pool2, coords, x, idx, dist2, mom, root), True)
        else:
            knn_output = (idx, dist2.sqrt() if self.dist == 'euclidean' else dist2)
            x = _per_point(self.pool1.mlp, self.pool1.pooled(self.lse1(coords, x, knn_output)), fused)
            x = _per_point(self.pool2.mlp, self.pool2.pooled(self.lse2(coords, x, knn_output)), fused)
        return self.lrelu(_per_point(self.mlp2, x, fused) + _per_point(self.shortcut, features, fused))


class _Shuffle(torch.autograd.Function):
    """x[..., perm] along the given dimension for a PERMUTATION perm: the gradient is the gather by its inverse (no
    scatter-add, so no atomics and the same bits every run)."""

    @staticmethod
    def forward(ctx, x, dim, perm, inverse):
        ctx.dim, ctx.inverse = dim, inverse
        return x.index_select(dim, perm)

    @staticmethod
    def backward(ctx, g):
        return g.index_select(ctx.dim, ctx.inverse), None, None, None


def _nearest_copy(x, idx, fused):
    """x (B,C,Nc,1), idx (B,Nf,1) -> (B,C,Nf,1): every fine point takes its nearest coarse point's features."""
    B, C, Nc, _ = x.shape
    Nf = idx.shape[1]
    if fused and x.is_cuda and x.dtype == torch.float32 and B * max(Nc, Nf) < _MAX_POINTS:
        from . import pointops, pointwise
        rows = pointwise.transpose12(x.squeeze(3).contiguous()).reshape(B * Nc, C)
        base = torch.arange(B, device=x.device, dtype=torch.int32).view(B, 1, 1) * Nc
        taken = pointops.grouping(rows, (idx + base).reshape(B * Nf, 1).contiguous())
        return pointwise.transpose12(taken.view(B, Nf, C)).unsqueeze(3)
    extended = idx.long().unsqueeze(1).expand(-1, C, -1, 1)
    return torch.gather(x, -2, extended)


class RandLANet(nn.Module):
    """`forward(input (B,N,d_in)) -> (B,num_classes,N)`.  permutation=: a device int64 permutation of N to shuffle the
    points with (so that a step can be captured); None draws the reference's host `torch.randperm(N)` at the same place
    in the host stream.  keep_graphs / `last_graphs`: {'encoder': [(idx, dist2)], 'decoder': [idx]} of the last call."""
    keep_graphs = False
    last_graphs = None

    def __init__(self, d_in, num_classes, num_neighbors=16, decimation=4, device=torch.device('cuda'), fused=True,
                 dist='squared', **kwargs):
        super().__init__()
        self.num_neighbors = num_neighbors
        self.decimation = decimation
        self.fused = fused

        self.fc_start = nn.Linear(d_in, 8)
        self.bn_start = nn.Sequential(nn.BatchNorm2d(8, eps=1e-6, momentum=0.99), nn.LeakyReLU(0.2))

        lfa = dict(fused=fused, dist=dist)
        self.encoder = nn.ModuleList([
            LocalFeatureAggregation(8, 16, num_neighbors, device, **lfa),
            LocalFeatureAggregation(32, 64, num_neighbors, device, **lfa),
            LocalFeatureAggregation(128, 128, num_neighbors, device, **lfa),
            LocalFeatureAggregation(256, 256, num_neighbors, device, **lfa)
        ])

        self.mlp = SharedMLP(512, 512, activation_fn=nn.ReLU())

        decoder_kwargs = dict(transpose=True, bn=True, activation_fn=nn.ReLU())
        self.decoder = nn.ModuleList([
            SharedMLP(1024, 256, **decoder_kwargs),
            SharedMLP(512, 128, **decoder_kwargs),
            SharedMLP(256, 32, **decoder_kwargs),
            SharedMLP(64, 8, **decoder_kwargs)
        ])

        self.fc_end = nn.Sequential(
            SharedMLP(8, 64, bn=True, activation_fn=nn.ReLU()),
            SharedMLP(64, 32, bn=True, activation_fn=nn.ReLU()),
            nn.Dropout(),
            SharedMLP(32, num_classes)
        )
        self.device = device
        self.to(device)

    def forward(self, input, permutation=None, keep_graphs=False):
        N = input.size(1)
        d = self.decimation
        fused = self.fused and input.is_cuda
        if N // d ** (len(self.encoder) - 1) < max(self.num_neighbors, 1) or N % d ** len(self.encoder):
            raise ValueError(f"RandLANet: {N} points do not divide into {len(self.encoder)} levels of decimation {d} "
                             f"with {self.num_neighbors} neighbours at the last")
        keep = keep_graphs or self.keep_graphs
        graphs = {'encoder': [], 'decoder': []}

        coords = input[..., :3].clone()
        x = self.fc_start(input).transpose(-2, -1).unsqueeze(-1)
        x = self.bn_start(x)                                   # (B, 8, N, 1)

        decimation_ratio = 1
        x_stack = []

        if permutation is None:
            permutation = torch.randperm(N)
        permutation = permutation.to(input.device)
        inverse = torch.empty_like(permutation)
        inverse[permutation] = torch.arange(N, device=permutation.device, dtype=permutation.dtype)
        coords = coords[:, permutation]
        x = _Shuffle.apply(x, 2, permutation, inverse)

        for lfa in self.encoder:
            level = coords[:, :N // decimation_ratio].contiguous()
            graph = knn_graph(level, level, lfa.num_neighbors)
            if keep:
                graphs['encoder'].append(graph)
            x = lfa(level, x, graph)
            x_stack.append(x.clone())
            decimation_ratio *= d
            x = x[:, :, :N // decimation_ratio]

        x = _per_point(self.mlp, x, fused)

        for mlp in self.decoder:
            neighbors, _ = knn_graph(coords[:, :N // decimation_ratio].contiguous(),            # the coarse set
                                     coords[:, :d * N // decimation_ratio].contiguous(), 1)     # the upsampled set
            if keep:
                graphs['decoder'].append(neighbors)
            x = torch.cat((_nearest_copy(x, neighbors, fused), x_stack.pop()), dim=1)
            x = _per_point(mlp, x, fused)
            decimation_ratio //= d

        x = _Shuffle.apply(x, 2, inverse, permutation)         # the inverse permutation
        for m in self.fc_end:
            x = _per_point(m, x, fused) if isinstance(m, SharedMLP) else m(x)
        if keep:
            self.last_graphs = graphs
        return x.squeeze(-1)
