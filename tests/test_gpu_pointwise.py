"""The per-point MLP layer (csrc/pointwise.hip, adaptpoint_amd.pointwise) against a float64 evaluation of the same
three modules -- Conv1d(kernel 1, no bias) + BatchNorm1d + ReLU, `ConvBNReLU1D` of
openpoints/models_adaptpoint/generator_component4_15.py:92-104 -- forward, every gradient, the running statistics."""
import copy

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

# (B, C_in, C_out, N): the imitator's layers at B = 2 (embedding, extract_feat 1 and 4, decoders 1 and 4), then
# sizes that are multiples of nothing (tile edges in all three contractions, the scalar loaders)
SHAPES = [(2, 3, 64, 1024), (2, 64, 128, 1024), (2, 512, 1024, 128), (2, 1536, 512, 256), (2, 192, 64, 1024),
          (3, 130, 70, 77), (1, 5, 33, 257), (5, 36, 200, 130),
          (40, 16, 24, 1024)]      # B * N above 32768: BatchNorm's gradient as two launches (below: one, csrc/pointwise.hip)

# planes per operand -> (bar on out, bar on gradients), relative L2 against float64: two bf16 planes keep 16 bits
# of each operand (~4e-6 measured), three keep all 24 (5e-8 .. 6e-7 measured, growing with the contraction length up to
# 1536: f32 accumulation -- fp32-class, the default)
TOL = {2: (3e-5, 2e-4), 3: (2e-6, 1e-5)}


def _rel(a, ref):
    return float((a.double() - ref).norm() / ref.norm().clamp_min(1e-30))


def _layer(C, O, dev, seed):
    g = torch.Generator().manual_seed(seed)
    conv = nn.Conv1d(C, O, 1, bias=False)
    bn = nn.BatchNorm1d(O)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(O, C, 1, generator=g) / C ** 0.5)
        bn.weight.copy_(0.5 + torch.rand(O, generator=g))
        bn.bias.copy_(0.3 * torch.randn(O, generator=g))
        bn.running_mean.copy_(0.1 * torch.randn(O, generator=g))
        bn.running_var.copy_(0.5 + torch.rand(O, generator=g))
    return conv.to(dev), bn.to(dev)


def _reference(conv, bn, x, gout, relu):
    """float64 modules.  With the ReLU, `gout` is zeroed IN PLACE where the pre-activation lies within 1e-4 of
    zero: there a 1e-5 difference in y decides the mask, and one flipped position (3 of 130,000 in the last
    shape) would move every gradient by ~1e-3 -- the comparison is of everything else."""
    conv64, bn64 = copy.deepcopy(conv).double(), copy.deepcopy(bn).double()
    x64 = x.detach().double().requires_grad_(True)
    out = bn64(conv64(x64))
    if relu:
        gout.mul_((out.detach().abs() > 1e-4).to(gout.dtype))
        out = torch.relu(out)
    out.backward(gout.double())
    return out.detach(), x64.grad, conv64.weight.grad, bn64.weight.grad, bn64.bias.grad, bn64


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("relu", [True, False], ids=["relu", "linear"])
@pytest.mark.parametrize("planes", [3, 2])
def test_layer_matches_float64_modules(dev, shape, relu, planes, monkeypatch):
    from adaptpoint_amd import pointwise
    monkeypatch.setattr(pointwise, "PRECISION", planes)
    TOL_OUT, TOL_GRAD = TOL[planes]
    B, C, O, N = shape
    conv, bn = _layer(C, O, dev, seed=B + C + O + N)
    g = torch.Generator(dev).manual_seed(1)
    x = torch.randn(B, C, N, device=dev, generator=g).requires_grad_(True)
    gout = torch.randn(B, O, N, device=dev, generator=g)
    ref_out, ref_gx, ref_gw, ref_gg, ref_gb, bn64 = _reference(conv, bn, x, gout, relu)
    assert pointwise.supported(x, conv, bn)
    out = pointwise.conv_bn_act(x, conv, bn, relu=relu)
    out.backward(gout)
    assert _rel(out, ref_out) < TOL_OUT
    assert float((out.double() - ref_out).abs().max()) < 10 * TOL_OUT
    assert _rel(x.grad, ref_gx) < TOL_GRAD
    assert _rel(conv.weight.grad, ref_gw) < TOL_GRAD
    assert _rel(bn.weight.grad, ref_gg) < TOL_GRAD
    assert _rel(bn.bias.grad, ref_gb) < TOL_GRAD
    assert _rel(bn.running_mean, bn64.running_mean) < 1e-5
    assert _rel(bn.running_var, bn64.running_var) < 1e-5
    assert int(bn.num_batches_tracked) == 1


def test_layer_with_running_statistics(dev):
    """eval(): the running statistics normalise, BatchNorm's gradient has no batch terms, nothing is updated."""
    from adaptpoint_amd import pointwise
    B, C, O, N = 3, 96, 160, 300
    conv, bn = _layer(C, O, dev, seed=5)
    bn.eval()
    g = torch.Generator(dev).manual_seed(2)
    x = torch.randn(B, C, N, device=dev, generator=g).requires_grad_(True)
    gout = torch.randn(B, O, N, device=dev, generator=g)
    ref_out, ref_gx, ref_gw, ref_gg, ref_gb, _ = _reference(conv, bn, x, gout, True)
    rm, rv = bn.running_mean.clone(), bn.running_var.clone()
    out = pointwise.conv_bn_act(x, conv, bn)
    out.backward(gout)
    TOL_OUT, TOL_GRAD = TOL[pointwise.PRECISION]
    assert _rel(out, ref_out) < TOL_OUT and _rel(x.grad, ref_gx) < TOL_GRAD and _rel(conv.weight.grad, ref_gw) < TOL_GRAD
    assert _rel(bn.weight.grad, ref_gg) < TOL_GRAD and _rel(bn.bias.grad, ref_gb) < TOL_GRAD
    assert torch.equal(bn.running_mean, rm) and torch.equal(bn.running_var, rv) and int(bn.num_batches_tracked) == 0


def test_gradients_are_bit_reproducible(dev):
    from adaptpoint_amd import pointwise
    B, C, O, N = 8, 192, 64, 1024
    conv, bn = _layer(C, O, dev, seed=9)
    g = torch.Generator(dev).manual_seed(3)
    x0 = torch.randn(B, C, N, device=dev, generator=g)
    gout = torch.randn(B, O, N, device=dev, generator=g)
    runs = []
    for _ in range(2):
        x = x0.clone().requires_grad_(True)
        conv.weight.grad = bn.weight.grad = bn.bias.grad = None
        out = pointwise.conv_bn_act(x, conv, bn)
        out.backward(gout)
        runs.append((out.detach().clone(), x.grad.clone(), conv.weight.grad.clone(), bn.weight.grad.clone(),
                     bn.bias.grad.clone()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_module_falls_back_where_the_kernels_do_not_apply(dev):
    """`ConvBNReLU1D(fused=True)` with a bias keeps the reference's three modules; without one it runs the
    kernels and agrees with its own unfused twin (same state_dict)."""
    from adaptpoint_amd.imitator import ConvBNReLU1D
    from adaptpoint_amd import pointwise
    x = torch.randn(2, 16, 200, device=dev, generator=torch.Generator(dev).manual_seed(4))
    biased = ConvBNReLU1D(16, 32, bias=True).to(dev)
    assert not pointwise.supported(x, biased.net[0], biased.net[1])
    assert biased(x).shape == (2, 32, 200)
    fused = ConvBNReLU1D(16, 32, bias=False, fused=True).to(dev)
    plain = ConvBNReLU1D(16, 32, bias=False, fused=False).to(dev)
    plain.load_state_dict(fused.state_dict())
    a, b = fused(x), plain(x)
    assert _rel(a, b.double()) < 1e-5
    assert _rel(fused.net[1].running_var, plain.net[1].running_var.double()) < 1e-5


@pytest.mark.parametrize("shape", [(2, 128, 1024, 1024), (3, 128, 1024, 2048), (2, 37, 70, 333), (4, 5, 130, 64)],
                         ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("relu", [True, False], ids=["relu", "linear"])
def test_conv_max_matches_float64_composition(dev, shape, relu):
    """convolution + bias (+ ReLU) + max over the points, fused (the discriminator's last group-all layer,
    point_discriminator.py:183-189), against the composed float64 evaluation: output, arg-max consistency, and the
    three gradients (the pooled gradient reaches one position per (cloud, channel))."""
    from adaptpoint_amd import pointwise
    B, C, O, N = shape
    g = torch.Generator(dev).manual_seed(B + C + O + N)
    x = torch.randn(B, C, N, device=dev, generator=g).requires_grad_(True)
    w = (torch.randn(O, C, 1, 1, device=dev, generator=g) / C ** 0.5).requires_grad_(True)
    bias = (0.3 * torch.randn(O, device=dev, generator=g)).requires_grad_(True)
    gout = torch.randn(B, O, device=dev, generator=g)
    x64, w64, b64 = (t.detach().double().requires_grad_(True) for t in (x, w, bias))
    y = torch.einsum("oc,bcn->bon", w64.view(O, C), x64) + b64.view(1, O, 1)
    ref = (torch.relu(y) if relu else y).amax(dim=2)
    # near-ties of the maximum (and of the ReLU kink) decide where the gradient goes: keep them out of the comparison
    top2 = y.detach().topk(2, dim=2)[0]
    clear = ((top2[..., 0] - top2[..., 1]) > 1e-4) & ((top2[..., 0].abs() > 1e-4) | (not relu))
    gout = gout * clear
    ref.backward(gout.double())
    assert pointwise.conv_max_supported(x, C)
    out = pointwise.conv_max(x, w, bias, relu=relu)
    out.backward(gout)
    assert _rel(out, ref.detach()) < 1e-6
    assert _rel(x.grad, x64.grad) < 5e-6 and _rel(w.grad, w64.grad) < 5e-6 and _rel(bias.grad, b64.grad) < 5e-6


@pytest.mark.parametrize("shape", [(32, 128, 1024), (3, 70, 77), (1, 1, 5), (2, 1024, 128), (5, 64, 1), (4, 65, 129)])
def test_transpose12_is_the_permuted_copy_both_ways(dev, shape):
    """`pointwise.transpose12` (apn_pw_transpose): bit-identical to `permute(0, 2, 1).contiguous()`, gradient included."""
    from adaptpoint_amd import pointwise
    torch.manual_seed(3)
    x = torch.randn(*shape, device=dev, requires_grad=True)
    y = pointwise.transpose12(x)
    assert y.is_contiguous() and torch.equal(y, x.detach().permute(0, 2, 1).contiguous())
    g = torch.randn_like(y)
    y.backward(g)
    assert torch.equal(x.grad, g.permute(0, 2, 1).contiguous())


@pytest.mark.parametrize("n,m", [(1024, 512), (512, 256), (77, 5), (128, 64)])
def test_three_nn_weights_equal_the_composed_form(dev, n, m):
    """`layers.three_nn_weights` (one launch for the weights) against `three_nn` + `inverse_distance_weights` (the
    reference's five elementwise operators, upsampling.py:97-100): same neighbours, weights to the last bit or one ulp."""
    from adaptpoint_amd import layers
    torch.manual_seed(4)
    unknown = torch.rand(3, n, 3, device=dev)
    known = torch.rand(3, m, 3, device=dev)
    known[0, :3] = unknown[0, :3]                      # exact hits: a zero distance (weight ~1, the others ~1e-8 x)
    dist, nearest = layers.three_nn(unknown, known)
    want = layers.inverse_distance_weights(dist)
    got_nearest, got = layers.three_nn_weights(unknown, known)
    assert torch.equal(got_nearest, nearest)
    assert float((got - want).abs().max()) <= 2e-7 and float((got.sum(-1) - 1).abs().max()) <= 3e-7


# ---- the Python entry points around the contraction kernel ----------------------------------------------------------

def _grads(out, gout, *leaves):
    for t in leaves:
        t.grad = None
    out.backward(gout)
    return [t.grad for t in leaves]


@pytest.mark.parametrize("shape", [(3, 130, 70, 77), (1, 5, 33, 257), (2, 3, 64, 1024)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("conv2d", [False, True], ids=["conv1d", "conv2d"])
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("relu", [True, False], ids=["relu", "linear"])
def test_conv_bias_act_matches_float64(dev, shape, conv2d, bias, relu):
    """`conv_bias_act` (the discriminator's per-point layers: no BatchNorm) with Conv1d- and Conv2d-shaped weights against
    float64: output and the gradients of input, weight and bias."""
    from adaptpoint_amd import pointwise
    B, C, O, N = shape
    g = torch.Generator(dev).manual_seed(B + C + O + N)
    x = torch.randn(B, C, N, device=dev, generator=g).requires_grad_(True)
    w = (torch.randn(*((O, C, 1, 1) if conv2d else (O, C, 1)), device=dev, generator=g) / C ** 0.5).requires_grad_(True)
    b = (0.3 * torch.randn(O, device=dev, generator=g)).requires_grad_(True) if bias else None
    gout = torch.randn(B, O, N, device=dev, generator=g)
    leaves = [x, w] + ([b] if bias else [])
    l64 = [t.detach().double().requires_grad_(True) for t in leaves]
    y = torch.einsum("oc,bcn->bon", l64[1].view(O, C), l64[0]) + (l64[2].view(1, O, 1) if bias else 0.0)
    if relu:
        gout = gout * (y.detach().abs() > 1e-4)          # (the mask's near-ties: see _reference)
        y = torch.relu(y)
    y.backward(gout.double())
    out = pointwise.conv_bias_act(x, w, b, relu=relu)
    grads = _grads(out, gout, *leaves)
    TOL_OUT, TOL_GRAD = TOL[pointwise.PRECISION]
    assert _rel(out, y.detach()) < TOL_OUT
    for got, ref in zip(grads, l64):
        assert got.shape == ref.grad.shape and _rel(got, ref.grad) < TOL_GRAD


def _conv_bn_block(C, O, dev, bias, seed, conv2d=False, relu=False, norm=True):
    g = torch.Generator().manual_seed(seed)
    conv = (nn.Conv2d if conv2d else nn.Conv1d)(C, O, 1, bias=bias)
    mods = [conv]
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) / C ** 0.5)
        if bias:
            conv.bias.copy_(0.3 * torch.randn(O, generator=g))
        if norm:
            bn = (nn.BatchNorm2d if conv2d else nn.BatchNorm1d)(O)
            bn.weight.copy_(0.5 + torch.rand(O, generator=g))
            bn.bias.copy_(0.3 * torch.randn(O, generator=g))
            bn.running_mean.copy_(0.1 * torch.randn(O, generator=g))
            bn.running_var.copy_(0.5 + torch.rand(O, generator=g))
            mods.append(bn)
    if relu:
        mods.append(nn.ReLU())
    return nn.Sequential(*mods).to(dev)


def _block_reference(block, x, gout, conv2d=False):
    """The block's own modules in float64 (a deep copy: buffers updated there) -> out, gradients of x and of every
    parameter in order, the copy.  `gout` is zeroed in place at the ReLU's near-ties (see _reference)."""
    b64 = copy.deepcopy(block).double()
    for m in b64.modules():
        m._forward_hooks.clear()
        m._forward_pre_hooks.clear()
    x64 = x.detach().double().requires_grad_(True)
    mods = list(b64)
    pre = x64.unsqueeze(2) if conv2d else x64
    for m in mods:
        if isinstance(m, nn.ReLU):
            gout.mul_((pre.detach().reshape(gout.shape).abs() > 1e-4).to(gout.dtype))
        pre = m(pre)
    out = pre.squeeze(2) if conv2d else pre
    out.backward(gout.double())
    return out.detach(), [x64.grad] + [p.grad for p in b64.parameters()], b64


def _check_block(run, block, x, gout, conv2d=False, tol=None):
    from adaptpoint_amd import pointwise
    TOL_OUT, TOL_GRAD = tol or TOL[pointwise.PRECISION]
    ref_out, ref_grads, b64 = _block_reference(block, x, gout, conv2d)
    out = run(x, block)
    grads = _grads(out, gout, x, *block.parameters())
    assert _rel(out, ref_out) < TOL_OUT
    top = max(float(r.norm()) for r in ref_grads[1:]) if len(ref_grads) > 1 else 0.0
    for got, ref in zip(grads, ref_grads):
        assert got.shape == ref.shape
        if float(ref.norm()) < 1e-9 * top:
            # an analytic zero (a convolution bias in front of a training-mode BatchNorm, which cancels it): float64
            # leaves ~1e-12 of rounding, float32 its own; held against the largest parameter gradient instead
            assert float(got.norm()) < 1e-5 * top
        else:
            assert _rel(got, ref) < TOL_GRAD
    for (name, buf), (_, buf64) in zip(block.named_buffers(), b64.named_buffers()):
        if buf.dtype.is_floating_point:
            assert _rel(buf, buf64) < 1e-5, name
        else:
            assert int(buf) == int(buf64), name
    return out


@pytest.mark.parametrize("bias", [False, True], ids=["nobias-fused", "bias"])
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_conv_then_bn_matches_float64_modules(dev, bias, training):
    """Sequential(Conv1d, BatchNorm1d): fused without a convolution bias, contraction + torch BatchNorm with one; output,
    every gradient, the running statistics (training) or their constancy (eval)."""
    from adaptpoint_amd import pointwise
    B, C, O, N = 3, 35, 70, 130
    block = _conv_bn_block(C, O, dev, bias, seed=21)
    block.train(training)
    g = torch.Generator(dev).manual_seed(6)
    x = torch.randn(B, C, N, device=dev, generator=g).requires_grad_(True)
    gout = torch.randn(B, O, N, device=dev, generator=g)
    before = int(block[1].num_batches_tracked)
    _check_block(pointwise.conv_then_bn, block, x, gout)
    assert int(block[1].num_batches_tracked) == before + int(training)


def test_conv_then_bn_hooks(dev, monkeypatch):
    """A forward hook on the block sees (and may replace) the fused result; a hook on the convolution forces the
    modules' own path."""
    from adaptpoint_amd import pointwise
    B, C, O, N = 2, 16, 32, 200
    block = _conv_bn_block(C, O, dev, False, seed=22)
    x = torch.randn(B, C, N, device=dev, generator=torch.Generator(dev).manual_seed(7))
    twin = copy.deepcopy(block)
    want = twin(x)
    seen = []
    handle = block.register_forward_hook(lambda mod, inp, out: (seen.append((inp[0], out)), out * 2.0)[1])
    calls = []
    real = pointwise._ConvBNAct.apply
    monkeypatch.setattr(pointwise._ConvBNAct, "apply", lambda *a: (calls.append(1), real(*a))[1])
    out = pointwise.conv_then_bn(x, block)
    assert len(calls) == 1 and len(seen) == 1 and seen[0][0] is x
    assert _rel(seen[0][1], want.double()) < 1e-5 and torch.equal(out, seen[0][1] * 2.0)
    handle.remove()
    conv_seen = []
    block[0].register_forward_hook(lambda mod, inp, out: conv_seen.append(out))
    twin2 = copy.deepcopy(twin)
    twin2.load_state_dict(block.state_dict())
    twin2.train()
    want2 = twin2(x)
    out2 = pointwise.conv_then_bn(x, block)
    assert len(calls) == 1 and len(conv_seen) == 1                 # the kernels were not entered again
    assert torch.equal(out2, want2)


@pytest.mark.parametrize("kind", ["conv1d-bn-relu", "conv2d-bn-relu", "conv2d-bn", "conv1d-relu", "conv2d-bias", "unknown"])
def test_run_block_matches_float64_modules(dev, kind, monkeypatch):
    """`run_block` on the `convblock`s of the PointNeXt mirror -- Conv1d / Conv2d, BatchNorm1d / 2d, no norm -- against
    the modules in float64; a structure it does not know runs the modules themselves and still agrees."""
    from adaptpoint_amd import pointwise
    B, C, O, N = 3, 35, 70, 130
    conv2d = kind.startswith("conv2d")
    if kind == "unknown":
        block = _conv_bn_block(C, O, dev, False, seed=23, relu=True)
        block = nn.Sequential(*block, nn.Identity()).to(dev)
    else:
        block = _conv_bn_block(C, O, dev, "bias" in kind, seed=23, conv2d=conv2d, relu="relu" in kind, norm="bn" in kind)
    calls = []
    real = pointwise._ConvBNAct.apply
    monkeypatch.setattr(pointwise._ConvBNAct, "apply", lambda *a: (calls.append(1), real(*a))[1])
    g = torch.Generator(dev).manual_seed(8)
    x = torch.randn(B, C, N, device=dev, generator=g).requires_grad_(True)
    gout = torch.randn(B, O, N, device=dev, generator=g)
    # (the unknown structure is PyTorch's own float32 path: its bars are those of an fp32 library, not of the kernels)
    _check_block(pointwise.run_block, block, x, gout, conv2d, tol=(1e-5, 1e-4) if kind == "unknown" else None)
    assert len(calls) == (0 if kind == "unknown" else 1)


@pytest.mark.parametrize("shape", [(256, 512, 256), (70, 130, 33), (3, 5, 1)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("planes", [3, 2])
def test_matmul_nt_matches_float64(dev, shape, planes, monkeypatch):
    from adaptpoint_amd import pointwise
    monkeypatch.setattr(pointwise, "PRECISION", planes)
    R, K, Q = shape
    g = torch.Generator(dev).manual_seed(R + K + Q)
    a = torch.randn(R, K, device=dev, generator=g)
    b = torch.randn(Q, K, device=dev, generator=g)
    out = pointwise.matmul_nt(a, b)
    assert out.shape == (R, Q) and _rel(out, a.double() @ b.double().t()) < TOL[planes][0]
    assert torch.equal(out, pointwise.matmul_nt(a, b))


@pytest.mark.parametrize("lead", [(4, 1024), (32, 1024)], ids=["4096rows", "32768rows"])
def test_linear_nobias_matches_float64(dev, lead):
    """`linear_nobias` (the imitator's `to_qkv`): forward and the input gradient are library GEMMs, the weight gradient
    the split-K contraction over all rows."""
    from adaptpoint_amd import pointwise
    C, O = 64, 192
    g = torch.Generator(dev).manual_seed(9)
    lin = nn.Linear(C, O, bias=False).to(dev)
    x = torch.randn(*lead, C, device=dev, generator=g).requires_grad_(True)
    gout = torch.randn(*lead, O, device=dev, generator=g)
    x64, w64 = x.detach().double().requires_grad_(True), lin.weight.detach().double().requires_grad_(True)
    ref = x64 @ w64.t()
    ref.backward(gout.double())
    out = pointwise.linear_nobias(x, lin)
    gx, gw = _grads(out, gout, x, lin.weight)
    TOL_OUT, TOL_GRAD = TOL[pointwise.PRECISION]
    assert out.shape == ref.shape and _rel(out, ref.detach()) < TOL_OUT
    assert _rel(gx, x64.grad) < TOL_GRAD and _rel(gw, w64.grad) < TOL_GRAD


def test_linear_nobias_falls_back_to_the_module(dev, monkeypatch):
    from adaptpoint_amd import pointwise
    monkeypatch.setattr(pointwise._LinearNoBias, "apply", lambda *a: pytest.fail("the kernel path was taken"))
    g = torch.Generator(dev).manual_seed(10)
    biased = nn.Linear(64, 96, bias=True).to(dev)
    x = torch.randn(4, 1024, 64, device=dev, generator=g)
    assert torch.equal(pointwise.linear_nobias(x, biased), biased(x))
    plain = nn.Linear(64, 96, bias=False).to(dev)
    few = torch.randn(3, 1000, 64, device=dev, generator=g)                 # fewer than 4096 rows
    assert torch.equal(pointwise.linear_nobias(few, plain), plain(few))


@pytest.mark.parametrize("shape", [(3, 36, 72, 260), (40, 16, 24, 1024)], ids=lambda s: "x".join(map(str, s)))
def test_layer_on_views_one_float_into_a_buffer(dev, shape):
    """`x` and the incoming gradient are contiguous views that start 4 bytes into their buffers (N a multiple of 4): no
    kernel of the layer may take them for 16-byte aligned -- the contractions and the BatchNorm passes decide their
    float4 form from the pointers."""
    from adaptpoint_amd import pointwise
    B, C, O, N = shape
    conv, bn = _layer(C, O, dev, seed=31)
    g = torch.Generator(dev).manual_seed(12)
    x = torch.randn(B * C * N + 1, device=dev, generator=g)[1:].view(B, C, N).requires_grad_(True)
    gout = torch.randn(B * O * N + 1, device=dev, generator=g)[1:].view(B, O, N)
    assert x.is_contiguous() and gout.is_contiguous() and x.data_ptr() % 16 == 4 and gout.data_ptr() % 16 == 4
    ref_out, ref_gx, ref_gw, ref_gg, ref_gb, bn64 = _reference(conv, bn, x, gout, True)
    out = pointwise.conv_bn_act(x, conv, bn)
    out.backward(gout)
    TOL_OUT, TOL_GRAD = TOL[pointwise.PRECISION]
    assert _rel(out, ref_out) < TOL_OUT and _rel(x.grad, ref_gx) < TOL_GRAD and _rel(conv.weight.grad, ref_gw) < TOL_GRAD
    assert _rel(bn.weight.grad, ref_gg) < TOL_GRAD and _rel(bn.bias.grad, ref_gb) < TOL_GRAD
    assert _rel(bn.running_var, bn64.running_var) < 1e-5
