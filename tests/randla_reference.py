"""Statements of RandLA-Net's LocalSpatialEncoding + AttentivePooling layer for the tests, in torch at any dtype / device.

`full_layer` is the reference's own, UNREDUCED sequence (openpoints/models/backbone/randlenet.py:84-136): the
(B,10,N,K) encoding, the 10 -> C convolution, a BatchNorm over (B,C,N,K), ReLU, the concatenation with the centre's
features to (B,2C,N,K), the full 2C x 2C score layer, the softmax over K and the weighted sum.  `reduced_layer` is what
csrc/randla.hip computes, `moment_statistics` the BatchNorm statistics from the encoding's moments.  Inputs are seeded;
integer-lattice clouds are `knn_reference.integer_cloud`'s.
"""
import numpy as np
import torch

import golden_inputs as GI
import knn_reference as KR

EPS, MOMENTUM = 1e-6, 0.99

# (B, N, K, C) of the GPU layer suite: a single point, a partial tile, K = 1, a K tail and the K maximum, every width
CASES = [(1, 1, 1, 8), (1, 37, 3, 8), (3, 130, 16, 8), (1, 37, 16, 32), (3, 130, 5, 32), (1, 130, 16, 64),
         (1, 37, 32, 64), (1, 130, 16, 128), (3, 37, 1, 128), (2, 130, 16, 16)]

# the model golden (tests/golden/make_golden_randla.py)
MODEL = dict(d_in=6, num_classes=5, num_neighbors=8, decimation=2)
MODEL_B, MODEL_N, MODEL_SEED = 2, 256, 4242


def rel(a, b):
    """|a - b| / |b| (L2) in float64; 0 / 0 = 0."""
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    den = b.norm().item()
    num = (a - b).norm().item()
    return num / den if den > 0 else num


def projection(g, g64):
    """<g - g64, g64> / |g64|^2: a dropped or doubled term shows here however small rounding is."""
    g, g64 = torch.as_tensor(g).double().cpu().ravel(), torch.as_tensor(g64).double().cpu().ravel()
    return abs(((g - g64) @ g64).item()) / max((g64 @ g64).item(), 1e-300)


def sample_index(name, numel, keep=8192):
    return GI.gradient_sample_index(name, numel, keep)


def layer_inputs(B, N, K, C, seed=0, integer=False):
    """Seeded float32 numpy inputs of one layer: coords, the exact graph (idx int32, squared distances), the centre's
    features f (B,C,N), the convolution (w, b), its BatchNorm (gamma, beta, running mean / variance), the score weight A
    (2C,2C) and an upstream gradient g (B,2C,N).  integer: lattice coordinates and small-integer weights."""
    rng = np.random.default_rng(1000 * seed + 7 * B + 13 * N + 17 * K + C)
    if integer:
        coords = KR.integer_cloud((B, N, 3), seed + N + K)
    else:
        coords = rng.uniform(-1.0, 1.0, size=(B, N, 3)).astype(np.float32)
    idx, d2 = KR.knn(coords, coords, K)
    out = dict(coords=coords, idx=idx.astype(np.int32), dist=d2.astype(np.float32))
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    if integer:
        out.update(w=f32(rng.integers(-2, 3, size=(C, 10))), b=f32(rng.integers(-2, 3, size=C)),
                   gamma=f32(np.ones(C)), beta=f32(rng.integers(-3, 4, size=C)))
    else:
        out.update(w=f32(rng.normal(size=(C, 10)) * 0.5), b=f32(rng.normal(size=C) * 0.1),
                   gamma=f32(0.75 + 0.5 * rng.random(C)), beta=f32(rng.normal(size=C) * 0.2))
    out.update(f=f32(rng.normal(size=(B, C, N))), A=f32(rng.normal(size=(2 * C, 2 * C)) * (0.5 / np.sqrt(C))),
               g=f32(rng.normal(size=(B, 2 * C, N))), rm=f32(rng.normal(size=C) * 0.1), rv=f32(0.5 + rng.random(C)))
    return out


def encoding(coords, idx, dist):
    """(B,10,N,K): [p_n, p_j, p_n - p_j, dist] as randlenet.py:88-100 builds it."""
    B, N, K = idx.shape
    ext = coords.transpose(-2, -1).unsqueeze(-1).expand(B, 3, N, K)
    nb = torch.gather(ext, 2, idx.long().unsqueeze(1).expand(B, 3, N, K))
    return torch.cat((ext, nb, ext - nb, dist.unsqueeze(-3)), dim=-3)


def hidden(e, w, b, gamma, beta, rm=None, rv=None, training=True, eps=EPS):
    """relu(bn(conv(e))) (B,C,N,K) and the (mean, biased variance) the BatchNorm used."""
    pre = torch.einsum('ci,bink->bcnk', w, e) + b.view(1, -1, 1, 1)
    if training:
        mean = pre.mean(dim=(0, 2, 3))
        var = ((pre - mean.view(1, -1, 1, 1)) ** 2).mean(dim=(0, 2, 3))
    else:
        mean, var = rm, rv
    y = (pre - mean.view(1, -1, 1, 1)) / torch.sqrt(var.view(1, -1, 1, 1) + eps) * gamma.view(1, -1, 1, 1)
    return torch.relu(y + beta.view(1, -1, 1, 1)), mean, var


def full_layer(coords, idx, dist, f, w, b, gamma, beta, A, rm=None, rv=None, training=True):
    """The unreduced layer -> (out (B,2C,N), mean, var): concatenation and the whole 2C x 2C score layer."""
    B, N, K = idx.shape
    h, mean, var = hidden(encoding(coords, idx, dist), w, b, gamma, beta, rm, rv, training)
    x = torch.cat((h, f.unsqueeze(-1).expand(B, -1, N, K)), dim=1)
    scores = torch.softmax(x.permute(0, 2, 3, 1) @ A.t(), dim=-2).permute(0, 3, 1, 2)
    return torch.sum(scores * x, dim=-1), mean, var


def reduced_layer(coords, idx, dist, f, w, b, gamma, beta, A, rm=None, rv=None, training=True):
    """[sum_k softmax_k(A_hh h_k) h_k ; f]: the form the kernels compute."""
    C = w.shape[0]
    h, mean, var = hidden(encoding(coords, idx, dist), w, b, gamma, beta, rm, rv, training)
    scores = torch.softmax(h.permute(0, 2, 3, 1) @ A[:C, :C].t(), dim=-2).permute(0, 3, 1, 2)
    return torch.cat((torch.sum(scores * h, dim=-1), f), dim=1), mean, var


def moment_statistics(e, w, b):
    """(mean, biased variance) per channel of conv(e) from the encoding's 10 means and its 10 x 10 second moments."""
    flat = e.permute(1, 0, 2, 3).reshape(10, -1)
    mu = flat.mean(dim=1)
    sigma = flat @ flat.t() / flat.shape[1] - torch.outer(mu, mu)
    return w @ mu + b, torch.einsum('ci,ij,cj->c', w, sigma, w)


def tensors(inputs, device, dtype):
    """The numpy inputs as tensors: the floats at `dtype`, the graph's index as int32."""
    out = {}
    for k, v in inputs.items():
        t = torch.from_numpy(np.ascontiguousarray(v)).to(device)
        out[k] = t if k == 'idx' else t.to(dtype)
    return out


PARAMS = ('w', 'b', 'gamma', 'beta', 'A', 'f')


def layer_with_gradients(layer, inputs, device, dtype, training=True, root=False):
    """`layer` (full_layer / reduced_layer) on the inputs -> (out, {name: gradient of sum(out * g)}, mean, var)."""
    t = tensors(inputs, device, dtype)
    leaves = {k: t[k].clone().requires_grad_() for k in PARAMS}
    dist = t['dist'].sqrt() if root else t['dist']
    out, mean, var = layer(t['coords'], t['idx'], dist, leaves['f'], leaves['w'], leaves['b'], leaves['gamma'],
                           leaves['beta'], leaves['A'], t['rm'], t['rv'], training)
    grads = torch.autograd.grad((out * t['g']).sum(), [leaves[k] for k in PARAMS], allow_unused=True)
    grads = {k: (torch.zeros_like(leaves[k]) if g is None else g) for k, g in zip(PARAMS, grads)}
    return out.detach(), grads, mean.detach(), var.detach()


# ---------------------------------------------------------------------------------------------------- the model golden
def model_inputs(seed=MODEL_SEED):
    """(input (B,N,6) float32, labels (B,N) int64): coordinates on the lattice of eighths in [-4, 4] -- every squared
    distance is exact in float32 whatever the order, ties go to the smaller index -- and three seeded feature columns."""
    rng = np.random.default_rng(seed)
    xyz = KR.integer_cloud((MODEL_B, MODEL_N, 3), seed, lo=-32, hi=32) / np.float32(8.0)
    feats = rng.normal(size=(MODEL_B, MODEL_N, 3)).astype(np.float32)
    labels = rng.integers(0, MODEL['num_classes'], size=(MODEL_B, MODEL_N))
    return torch.from_numpy(np.concatenate([xyz, feats], axis=-1)), torch.from_numpy(labels)


def knn_standin(support, query, k):
    """What the golden's `torch_points_kernels.knn` is: `knn_reference.knn` on float32 coordinates by direct
    differences, ties to the smaller index, SQUARED distances -> (idx (B,M,k) int64, dist (B,M,k) float32)."""
    idx, d2 = KR.knn(support.detach().cpu().numpy().astype(np.float32), query.detach().cpu().numpy().astype(np.float32), k)
    return torch.from_numpy(idx.astype(np.int64)), torch.from_numpy(d2.astype(np.float32))


def model_loss(logits, labels):
    return torch.nn.functional.cross_entropy(logits, labels, reduction='sum')
