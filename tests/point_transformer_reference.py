"""Inputs from seeds and the float64 statements of the Point Transformer layer and model
(tests/test_point_transformer_cpu.py, tests/test_gpu_point_transformer_layer.py, tests/test_gpu_point_transformer.py,
tests/golden/make_golden_point_transformer.py).

The float64 statement is the composed module itself in `.double()` on graphs that are handed in: the restatement is about
the arithmetic behind the graphs.  As `dgcnn_reference.run_classifier64` it reports the decision margin of its ReLU
gates and pool winners: how close the nearest one is to switching, relative to its tensor's rms."""
import copy

import numpy as np
import torch

import pointops_reference as PR
from invres_reference import rel, sample_index  # noqa: F401

NARROW = dict(width=8, blocks=[2, 2, 2, 2, 2], nsample=[8, 16, 16, 16, 16], in_channels=6, num_classes=13)
NARROW_SIZES = (300, 520, 257)          # the deep levels hold (1, 2, 1) points: fewer than k, the padding rule
FULL_BLOCKS = [2, 3, 4, 6, 3]
GOLDEN_FIRST_SEED = 0


def pack(tag, group, dtype):
    """{name: array} -> three members: the names, their sizes and one flat array."""
    names = list(group)
    return {tag + "names": np.array(names), tag + "sizes": np.array([np.size(group[n]) for n in names], dtype=np.int64),
            tag + "flat": np.concatenate([np.asarray(group[n], dtype=dtype).ravel() for n in names])}


def unpack(gold, tag):
    """The {name: flat array} that `pack` stored under `tag`."""
    names, sizes, flat = gold[tag + "names"].tolist(), gold[tag + "sizes"], gold[tag + "flat"]
    ends = np.cumsum(sizes)
    return {n: flat[e - s:e] for n, s, e in zip(names, sizes, ends)}


def model_inputs(sizes, seed, in_channels=6, num_classes=13):
    """p (n,3) uniform in [-1,1]^3, x (n,in_channels) = [p | normal features], o (b) int32, w (n,num_classes): the
    weights of the loss sum(logits * w)."""
    n = int(sum(sizes))
    p = PR.seeded_clouds(sizes, 2100 + seed)
    feats = PR.features((n, in_channels - 3), 2200 + seed)
    w = PR.features((n, num_classes), 2300 + seed)
    t = torch.from_numpy
    return t(p), t(np.concatenate([p, feats], 1)), t(PR.offsets(sizes)), t(w)


def layer_inputs(sizes, C, seed):
    """p (n,3), x (n,C), o (b), w (n,C) from a seed."""
    n = int(sum(sizes))
    t = torch.from_numpy
    return (t(PR.seeded_clouds(sizes, 2400 + seed)), t(PR.features((n, C), 2500 + seed)), t(PR.offsets(sizes)),
            t(PR.features((n, C), 2600 + seed)))


def seed_module(module, seed):
    """Weights and BatchNorm buffers of a bare module from a seed: the scheme of `fill_parameters_by_name`, the seed
    mixed into every name."""
    import zlib
    with torch.no_grad():
        for name, t in module.state_dict().items():
            g = torch.Generator().manual_seed(zlib.crc32(f"{seed}/{name}".encode()) & 0x7FFFFFFF)
            if name.endswith('num_batches_tracked'):
                continue
            if name.endswith('running_var'):
                v = 0.5 + torch.rand(t.shape, generator=g)
            elif name.endswith('running_mean'):
                v = 0.1 * torch.randn(t.shape, generator=g)
            elif t.dim() == 1 and name.endswith('weight'):            # a BatchNorm's gamma
                v = 0.75 + 0.5 * torch.rand(t.shape, generator=g)
            elif t.dim() == 1:
                v = 0.05 * torch.randn(t.shape, generator=g)
            else:
                v = torch.randn(t.shape, generator=g) * (1.0 / t[0].numel()) ** 0.5
            t.copy_(v.to(t.dtype))
    return module


class _Margin:
    """Pre-hooks on every ReLU and MaxPool1d: the smallest |pre-activation| and the smallest lead of a pool winner,
    each relative to its tensor's rms."""

    def __init__(self, model):
        self.margin = float('inf')
        for m in model.modules():
            if isinstance(m, torch.nn.ReLU):
                m.register_forward_pre_hook(self._relu)
            elif isinstance(m, torch.nn.MaxPool1d):
                m.register_forward_pre_hook(self._pool)

    def _note(self, gap, x):
        rms = float(x.detach().pow(2).mean().sqrt())
        gap = gap[gap > 0]              # exact ties are the repeated rows of a padded neighbourhood: equal values, no decision
        if gap.numel() and rms > 0:
            self.margin = min(self.margin, float(gap.min()) / rms)

    def _relu(self, m, inp):
        self._note(inp[0].detach().abs(), inp[0])

    def _pool(self, m, inp):
        x = inp[0].detach()
        if x.shape[-1] > 1:
            top = x.topk(2, dim=-1)[0]
            self._note(top[..., 0] - top[..., 1], x)


def _double(module):
    m = copy.deepcopy(module).double()
    for sub in m.modules():
        if hasattr(sub, 'fused'):
            sub.fused = False
    return m


def _graphs_to(graphs, dev):
    mv = lambda t: None if t is None else t.to(dev)
    return {'stage': [mv(g) for g in graphs['stage']], 'down': [(mv(a), mv(b)) for a, b in graphs['down']],
            'up': [mv(g) for g in graphs['up']]}


def run_model64(model, p, x, o, graphs, w=None, training=True):
    """`adaptpoint_amd.point_transformer.PTSeg` in float64 on the graphs given (a `last_graphs` dict), on the device
    of p.  -> dict: logits; with w: grads {name: dL/dparam} of sum(logits * w); buffers after the step; margin."""
    m64 = _double(model).to(p.device).train(training)
    mg = _Margin(m64)
    logits = m64(p.double(), x.double(), o, graphs=_graphs_to(graphs, p.device))
    res = {'logits': logits.detach(), 'margin': mg.margin}
    if w is not None:
        (logits * w.double()).sum().backward()
        res['grads'] = {n: q.grad for n, q in m64.named_parameters()}
    res['buffers'] = dict(m64.named_buffers())
    return res


def run_layer64(layer, p, x, o, idx, w=None, training=True):
    """`PointTransformerLayer` in float64 on the graph idx (n,k).  -> dict: out; with w: dx and grads of
    sum(out * w); buffers after the step; margin."""
    from adaptpoint_amd.point_transformer import StageGraph
    l64 = _double(layer).to(p.device).train(training)
    mg = _Margin(l64)
    x64 = x.detach().double().requires_grad_(True)
    p64 = p.double()
    out = l64([p64, x64, o, StageGraph(p64, o, layer.nsample, idx)])
    res = {'out': out.detach(), 'margin': mg.margin}
    if w is not None:
        (out * w.double()).sum().backward()
        res.update(dx=x64.grad, grads={n: q.grad for n, q in l64.named_parameters()})
    res['buffers'] = dict(l64.named_buffers())
    return res
