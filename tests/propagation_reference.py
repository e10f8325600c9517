"""Shared pieces of the feature-propagation tests (test_propagation_cpu.py, test_gpu_propagation.py): layers with
seeded parameters, three-nearest indices / weights made in float64, and the COMPOSED block -- interpolate, concatenate,
Conv1d + BatchNorm1d (+ ReLU) -- evaluated by float64 torch modules."""
import copy

import torch
import torch.nn as nn

# (C1, C2, O, n, m): the imitator's four decoders (B = 2 in the tests), then a shape that is a multiple of nothing
DECODER_SHAPES = [(512, 1024, 512, 128, 64), (256, 512, 256, 256, 128), (128, 256, 128, 512, 256), (64, 128, 64, 1024, 512)]
RAGGED = (37, 70, 45, 333, 101)

# the project's bars for a per-point layer with fp32-class operands (tests/test_gpu_pointwise.py): relative L2 on the
# output / on the gradients, and on the running statistics
TOL_OUT, TOL_GRAD, TOL_STAT = 2e-6, 1e-5, 1e-5


def rel(a, ref):
    return float((a.detach().double().cpu() - ref.double().cpu()).norm() / ref.double().norm().clamp_min(1e-30))


def layer(C, O, seed):
    g = torch.Generator().manual_seed(seed)
    conv = nn.Conv1d(C, O, 1, bias=False)
    bn = nn.BatchNorm1d(O)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(O, C, 1, generator=g) / C ** 0.5)
        bn.weight.copy_(0.5 + torch.rand(O, generator=g))
        bn.bias.copy_(0.3 * torch.randn(O, generator=g))
        bn.running_mean.copy_(0.1 * torch.randn(O, generator=g))
        bn.running_var.copy_(0.5 + torch.rand(O, generator=g))
    return conv, bn


def nearest_weights(xyz1, xyz2):
    """The three nearest of xyz2 (B,m,3) for every point of xyz1 (B,n,3) by float64 distances and their
    inverse-distance weights 1 / (d + 1e-8), normalised: (idx (B,n,3) int32, weights (B,n,3) float32)."""
    d, idx = torch.cdist(xyz1.double(), xyz2.double()).topk(3, dim=2, largest=False)
    w = 1.0 / (d + 1e-8)
    return idx.int(), (w / w.sum(2, keepdim=True)).float()


def blend64(u, idx, w):
    B, O, _ = u.shape
    n = idx.shape[1]
    ix = idx.long()
    return sum(torch.gather(u, 2, ix[:, :, j].unsqueeze(1).expand(B, O, n)) * w[:, :, j].double().unsqueeze(1) for j in range(3))


def composed64(conv, bn, f1, f2, idx, w, gout, relu=True):
    """The composed block in float64 on the CPU.  With the ReLU, `gout` is zeroed IN PLACE where the float64
    pre-activation lies within 1e-4 of zero (there a 1e-5 difference decides the mask, tests/test_gpu_pointwise.py);
    -> dict of results and the zeroed share."""
    conv64, bn64 = copy.deepcopy(conv).double().cpu(), copy.deepcopy(bn).double().cpu()
    a1 = None if f1 is None else f1.detach().double().cpu().requires_grad_(True)
    a2 = f2.detach().double().cpu().requires_grad_(True)
    up = blend64(a2, idx.cpu(), w.cpu())
    out = bn64(conv64(up if a1 is None else torch.cat([a1, up], dim=1)))
    share = 0.0
    if relu:
        keep = (out.detach().abs() > 1e-4)
        share = 1.0 - float(keep.double().mean())
        gout.mul_(keep.to(device=gout.device, dtype=gout.dtype))
        out = torch.relu(out)
    if conv64.weight.requires_grad:
        out.backward(gout.detach().double().cpu())
    return dict(out=out.detach(), g_f1=None if a1 is None else a1.grad, g_f2=a2.grad, g_w=conv64.weight.grad,
                g_gamma=bn64.weight.grad, g_beta=bn64.bias.grad, bn=bn64, share=share)


def inputs(B, C1, C2, n, m, seed, dev="cpu", skip=True):
    g = torch.Generator().manual_seed(seed)
    xyz1 = torch.rand(B, n, 3, generator=g)
    xyz2 = xyz1[:, torch.randperm(n, generator=g)[:m]].contiguous() if m <= n else torch.rand(B, m, 3, generator=g)
    f1 = torch.randn(B, C1, n, generator=g).to(dev).requires_grad_(True) if skip else None
    f2 = torch.randn(B, C2, m, generator=g).to(dev).requires_grad_(True)
    return xyz1, xyz2, f1, f2
