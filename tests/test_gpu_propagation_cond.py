"""GPU: the hoisted feature-propagation block with a per-cloud conditioning vector in front of its concatenation
(apn_fp_blend_stats_cond, apn_fp_cond_grad, adaptpoint_amd.propagation.propagate(..., cond=)) -- against float64 torch
modules evaluated on the same indices and weights by the method and constants of tests/propagation_reference.py, on a
case in which every sum is exact in float32, against the unconditioned call, against itself, and the raw entries'
argument checks."""
import copy

import pytest
import torch

import propagation_reference as PR

pytestmark = pytest.mark.gpu

# (B, Cc, C1, C2, O, n, m): n below / straddling / above one 128-column tile, O below / across the 64-channel chunk,
# m = 1, 2, 3 (fewer coarse points than neighbours) and 40, a conditioning vector of the 'curvenet' map's width
SHAPES = [(3, 16, 8, 12, 3, 5, 1), (3, 16, 8, 12, 65, 130, 2), (3, 7, 8, 12, 65, 257, 3), (3, 16, 5, 12, 3, 257, 40),
          (3, 208, 32, 64, 65, 130, 40)]
IDS = lambda s: "x".join(map(str, s))


def _setup(dev, shape, seed, skip=True, training=True):
    B, Cc, C1, C2, O, n, m = shape
    conv, bn = PR.layer(Cc + (C1 if skip else 0) + C2, O, seed)
    conv, bn = conv.to(dev), bn.to(dev)
    bn.train(training)
    g = torch.Generator().manual_seed(seed + 1)
    f1 = torch.randn(B, C1, n, generator=g).to(dev).requires_grad_(True) if skip else None
    f2 = torch.randn(B, C2, m, generator=g).to(dev).requires_grad_(True)
    cond = torch.randn(B, Cc, generator=g)
    cond[1] = 0.0                                      # one cloud without conditioning; the others differ from each other
    cond = cond.to(dev).requires_grad_(True)
    nearest = torch.randint(0, m, (B, n, 3), generator=g).int().to(dev)
    w = torch.rand(B, n, 3, generator=g) + 0.05
    weights = (w / w.sum(2, keepdim=True)).to(dev)
    gout = torch.randn(B, O, n, generator=g).to(dev)
    return conv, bn, cond, f1, f2, nearest, weights, gout


def _composed64(conv, bn, cond, f1, f2, idx, w, gout):
    """PR.composed64 with the repeated vector in front of the concatenation."""
    conv64, bn64 = copy.deepcopy(conv).double().cpu(), copy.deepcopy(bn).double().cpu()
    leaf = lambda t: None if t is None else t.detach().double().cpu().requires_grad_(True)
    c0, a1, a2 = leaf(cond), leaf(f1), leaf(f2)
    n = idx.shape[1]
    up = PR.blend64(a2, idx.cpu(), w.cpu())
    cat = [c0.unsqueeze(-1).expand(-1, -1, n)] + ([] if a1 is None else [a1]) + [up]
    pre = bn64(conv64(torch.cat(cat, dim=1)))
    keep = pre.detach().abs() > 1e-4
    gout.mul_(keep.to(device=gout.device, dtype=gout.dtype))
    torch.relu(pre).backward(gout.detach().double().cpu())
    return dict(out=torch.relu(pre).detach(), g_cond=c0.grad, g_f1=None if a1 is None else a1.grad, g_f2=a2.grad,
                g_w=conv64.weight.grad, g_gamma=bn64.weight.grad, g_beta=bn64.bias.grad, bn=bn64,
                share=1.0 - float(keep.double().mean()))


def _composed(conv, bn, cond, f1, f2, nearest, weights, gout):
    """The composed path of the library: repeat, three_interpolate, cat, pointwise.conv_bn_act, on copies."""
    from adaptpoint_amd import layers, pointwise
    c, b = copy.deepcopy(conv), copy.deepcopy(bn)
    leaf = lambda t: None if t is None else t.detach().clone().requires_grad_(True)
    c0, a1, a2 = leaf(cond), leaf(f1), leaf(f2)
    n = nearest.shape[1]
    up = layers.three_interpolate(a2, nearest, weights)
    x = torch.cat([c0.unsqueeze(-1).expand(-1, -1, n)] + ([] if a1 is None else [a1]) + [up], dim=1).contiguous()
    assert pointwise.supported(x, c, b)
    out = pointwise.conv_bn_act(x, c, b, relu=True)
    out.backward(gout)
    return dict(out=out.detach(), g_cond=c0.grad, g_f1=None if a1 is None else a1.grad, g_f2=a2.grad, g_w=c.weight.grad,
                g_gamma=b.weight.grad, g_beta=b.bias.grad)


def _run(conv, bn, cond, f1, f2, nearest, weights, gout):
    from adaptpoint_amd import propagation
    assert propagation.supported(f1, f2, conv, bn, cond)
    out = propagation.propagate(f1, f2, nearest, weights, conv, bn, relu=True, cond=cond)
    leaves = [cond, f2, conv.weight, bn.weight, bn.bias] + ([] if f1 is None else [f1])
    grads = torch.autograd.grad(out, leaves, gout)
    res = dict(zip(["g_cond", "g_f2", "g_w", "g_gamma", "g_beta", "g_f1"], grads))
    res["out"] = out.detach()
    return res


def _check(dev, shape, training, skip, seed):
    conv, bn, cond, f1, f2, nearest, weights, gout = _setup(dev, shape, seed, skip, training)
    ref = _composed64(conv, bn, cond, f1, f2, nearest, weights, gout)
    assert ref["share"] < 0.05
    comp = _composed(conv, bn, cond, f1, f2, nearest, weights, gout)
    before = (bn.running_mean.clone(), bn.running_var.clone(), int(bn.num_batches_tracked))
    res = _run(conv, bn, cond, f1, f2, nearest, weights, gout)
    keys = ["out", "g_cond", "g_f2", "g_w", "g_gamma", "g_beta"] + (["g_f1"] if skip else [])
    e_h = {k: PR.rel(res[k], ref[k]) for k in keys}
    e_c = {k: PR.rel(comp[k], ref[k]) for k in keys}
    print("shape", shape, "train" if training else "eval", "skip" if skip else "no-skip",
          "| conditioned", {k: "%.2e" % v for k, v in e_h.items()}, "| composed", {k: "%.2e" % v for k, v in e_c.items()})
    for k in keys:
        bar = max(PR.TOL_OUT if k == "out" else PR.TOL_GRAD, 2.0 * e_c[k])
        assert e_h[k] < bar, (k, e_h[k], "composed", e_c[k])
    if training:
        assert PR.rel(bn.running_mean, ref["bn"].running_mean) < PR.TOL_STAT
        assert PR.rel(bn.running_var, ref["bn"].running_var) < PR.TOL_STAT
        assert int(bn.num_batches_tracked) == before[2] + 1
    else:
        assert torch.equal(bn.running_mean, before[0]) and torch.equal(bn.running_var, before[1])
        assert int(bn.num_batches_tracked) == before[2]


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_conditioned_block_matches_float64_modules(dev, shape, training):
    _check(dev, shape, training, True, seed=sum(shape))


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[3]], ids=IDS)
def test_conditioned_block_without_skip_features(dev, shape, training):
    _check(dev, shape, training, False, seed=sum(shape) + 5)


def _integers(shape, lo, hi, seed):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).float()


@pytest.mark.parametrize("skip", [True, False], ids=["skip", "no-skip"])
def test_conditioned_block_on_an_exact_case(dev, skip):
    """Small-integer weights, features and cond, one-hot interpolation weights, BatchNorm in eval mode with identity
    statistics (mean 0, variance 1, eps 0, gamma 1, beta 0): every product and sum is an integer below 2^24, exact in
    float32 in any order, so the output and every gradient equal the integer statement bit for bit."""
    from adaptpoint_amd import propagation
    B, Cc, C1, C2, O, n, m = 3, 6, 4, 5, 65, 130, 7
    conv = torch.nn.Conv1d(Cc + (C1 if skip else 0) + C2, O, 1, bias=False)
    bn = torch.nn.BatchNorm1d(O, eps=0.0)
    with torch.no_grad():
        conv.weight.copy_(_integers(tuple(conv.weight.shape), -2, 2, 1))
    conv, bn = conv.to(dev), bn.to(dev).eval()
    cond = _integers((B, Cc), -3, 3, 2)
    cond[2] = 0.0
    f1 = _integers((B, C1, n), -3, 3, 3) if skip else None
    f2 = _integers((B, C2, m), -3, 3, 4)
    nearest = torch.randint(0, m, (B, n, 3), generator=torch.Generator().manual_seed(5)).int()
    weights = torch.zeros(B, n, 3)
    weights[:, :, 0] = 1.0
    gout = _integers((B, O, n), -2, 2, 6)
    # the integer statement
    W = conv.weight.detach().cpu().long()[:, :, 0]
    c1 = Cc + (C1 if skip else 0)
    up = torch.gather(f2.long(), 2, nearest[:, :, 0].long().unsqueeze(1).expand(B, C2, n))
    y = torch.einsum("ok,bk->bo", W[:, :Cc], cond.long()).unsqueeze(-1) + torch.einsum("ok,bkn->bon", W[:, c1:], up)
    if skip:
        y = y + torch.einsum("ok,bkn->bon", W[:, Cc:c1], f1.long())
    gy = gout.long() * (y > 0)
    gc = gy.sum(2)
    gu = torch.zeros(B, O, m, dtype=torch.long).scatter_add_(2, nearest[:, :, 0].long().unsqueeze(1).expand(B, O, n), gy)
    want = dict(out=y.clamp_min(0), g_cond=gc @ W[:, :Cc], g_f2=torch.einsum("ok,bom->bkm", W[:, c1:], gu),
                g_w=torch.cat([gc.t() @ cond.long()] + ([torch.einsum("bon,bkn->ok", gy, f1.long())] if skip else [])
                              + [torch.einsum("bom,bkm->ok", gu, f2.long())], dim=1).unsqueeze(-1))
    if skip:
        want["g_f1"] = torch.einsum("ok,bon->bkn", W[:, Cc:c1], gy)
    assert max(int(v.abs().max()) for v in want.values()) < 2 ** 24
    leaf = lambda t: None if t is None else t.to(dev).requires_grad_(True)
    res = _run(conv, bn, leaf(cond), leaf(f1), leaf(f2), nearest.to(dev), weights.to(dev), gout.to(dev))
    for k, v in want.items():
        assert torch.equal(res[k].cpu(), v.float()), k
    # the raw row-sum entry on the same integers
    from adaptpoint_amd import _lib
    lib = _lib.load()
    g = gy.float().to(dev).contiguous()
    out = torch.full((B, O), -1.0, device=dev)
    assert lib.apn_fp_cond_grad(B, O, n, g.data_ptr(), out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream) == 0
    assert torch.equal(out.cpu(), gc.float())
    assert propagation.supported(leaf(f1), leaf(f2), conv, bn, leaf(cond))


def test_zero_conditioning_gives_the_bits_of_the_unconditioned_call(dev):
    """cond=None is today's call; a conv widened by Cc columns with an all-zero cond adds c = 0 to the same sums: the
    output and the feature gradients are the unconditioned call's, bit for bit."""
    from adaptpoint_amd import propagation
    shape = (3, 16, 8, 12, 65, 257, 40)
    B, Cc = shape[0], shape[1]
    conv, bn, cond, f1, f2, nearest, weights, gout = _setup(dev, shape, 21)
    plain_conv = torch.nn.Conv1d(conv.in_channels - Cc, conv.out_channels, 1, bias=False).to(dev)
    with torch.no_grad():
        plain_conv.weight.copy_(conv.weight[:, Cc:])
    plain_bn = copy.deepcopy(bn)
    a1, a2 = f1.detach().clone().requires_grad_(True), f2.detach().clone().requires_grad_(True)
    out0 = propagation.propagate(a1, a2, nearest, weights, plain_conv, plain_bn, cond=None)
    g0 = torch.autograd.grad(out0, [a1, a2, plain_conv.weight, plain_bn.weight, plain_bn.bias], gout)
    zero = torch.zeros(B, Cc, device=dev, requires_grad=True)
    res = _run(conv, bn, zero, f1, f2, nearest, weights, gout)
    assert torch.equal(res["out"], out0.detach())
    assert torch.equal(res["g_f1"], g0[0]) and torch.equal(res["g_f2"], g0[1])
    assert torch.equal(res["g_w"][:, Cc:], g0[2])
    assert torch.equal(res["g_gamma"], g0[3]) and torch.equal(res["g_beta"], g0[4])
    assert torch.equal(bn.running_mean, plain_bn.running_mean) and torch.equal(bn.running_var, plain_bn.running_var)
    assert not res["g_w"][:, :Cc].any()                # gc^T 0


def test_conditioned_block_is_bit_reproducible(dev):
    conv, bn, cond, f1, f2, nearest, weights, gout = _setup(dev, (3, 208, 32, 64, 65, 1024, 256), 9)
    runs = [_run(conv, bn, cond, f1, f2, nearest, weights, gout) for _ in range(2)]
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k


def test_conditioned_entries_check_their_arguments(dev):
    """Host-side checks only: every call returns before a launch."""
    from adaptpoint_amd import _lib
    lib = _lib.load()
    buf = torch.zeros(64, device=dev)
    ibuf = torch.zeros(64, dtype=torch.int32, device=dev)
    p, ip = buf.data_ptr(), ibuf.data_ptr()
    stream = torch.cuda.current_stream(dev).cuda_stream

    def call(b=1, o=2, m=3, n=4, a=p, u=p, idx=ip, w=p, c=p, y=p, part=p, training=1, rm=p, rv=p, out=p):
        return lib.apn_fp_blend_stats_cond(b, o, m, n, a, u, idx, w, c, y, part, training, None, None, rm, rv, 1e-5, 1, None,
                                           out, stream)
    EINVAL, OK = -1, 0
    for kw in (dict(c=None), dict(b=-1), dict(o=-1), dict(m=-1), dict(n=-1), dict(b=65536), dict(u=None), dict(idx=None),
               dict(w=None), dict(y=None), dict(part=None), dict(training=0, out=None), dict(training=0, rm=None), dict(m=0)):
        assert call(**kw) == EINVAL, kw
    for kw in (dict(b=0), dict(o=0), dict(n=0)):
        assert call(**kw) == OK, kw
    grad = lambda b=1, o=2, n=4, gy=p, gc=p: lib.apn_fp_cond_grad(b, o, n, gy, gc, stream)
    for kw in (dict(b=-1), dict(o=-1), dict(n=-1), dict(b=65536), dict(gy=None), dict(gc=None)):
        assert grad(**kw) == EINVAL, kw
    for kw in (dict(b=0), dict(o=0)):
        assert grad(**kw) == OK, kw
    torch.cuda.synchronize()
    assert not buf.any() and not ibuf.any()          # nothing was launched
