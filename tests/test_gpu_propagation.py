"""GPU: the feature-propagation block with its convolution hoisted to the coarse points (csrc/feature_prop.hip,
apn_pw_contract2, adaptpoint_amd.propagation) against float64 torch modules evaluated on the same indices and weights,
against the composed path of the same library in the same run, against the reference-made goldens of the modules that
take `hoisted=`, bit for bit against itself, and replayed from a hipGraph."""
import copy
import gc

import numpy as np
import pytest
import torch

import golden_inputs as GI
import propagation_reference as PR

pytestmark = pytest.mark.gpu

# (B, C1, C2, O, n, m): the CPU suite's shapes, one decoder at the bench's batch and N = 2048, a segmentation-sized level
SHAPES = [(2,) + s for s in PR.DECODER_SHAPES] + [(2,) + PR.RAGGED, (32, 64, 128, 64, 2048, 1024), (4, 32, 64, 32, 15000, 3750)]
REPRO = (8, 64, 128, 64, 1024, 512)


def _setup(dev, shape, seed, skip=True, training=True):
    from adaptpoint_amd import layers
    B, C1, C2, O, n, m = shape
    conv, bn = PR.layer((C1 if skip else 0) + C2, O, seed)
    conv, bn = conv.to(dev), bn.to(dev)
    bn.train(training)
    xyz1, xyz2, f1, f2 = PR.inputs(B, C1, C2, n, m, seed + 1, dev=dev, skip=skip)
    nearest, weights = layers.three_nn_weights(xyz1.to(dev).contiguous(), xyz2.to(dev).contiguous())
    gout = torch.randn(B, O, n, generator=torch.Generator().manual_seed(seed + 2)).to(dev)
    return conv, bn, f1, f2, nearest, weights, gout


def _composed(conv, bn, f1, f2, nearest, weights, gout):
    """The composed path of the library (three_interpolate + cat + pointwise.conv_bn_act) on copies of the modules."""
    from adaptpoint_amd import layers, pointwise
    c, b = copy.deepcopy(conv), copy.deepcopy(bn)
    a1 = None if f1 is None else f1.detach().clone().requires_grad_(True)
    a2 = f2.detach().clone().requires_grad_(True)
    up = layers.three_interpolate(a2, nearest, weights)
    x = up if a1 is None else torch.cat([a1, up], dim=1)
    assert pointwise.supported(x, c, b)
    out = pointwise.conv_bn_act(x, c, b, relu=True)
    out.backward(gout)
    return dict(out=out.detach(), g_f1=None if a1 is None else a1.grad, g_f2=a2.grad, g_w=c.weight.grad, g_gamma=b.weight.grad,
                g_beta=b.bias.grad, bn=b)


def _errors(res, ref, skip):
    keys = ["out", "g_f2", "g_w", "g_gamma", "g_beta"] + (["g_f1"] if skip else [])
    return {k: PR.rel(res[k], ref[k]) for k in keys}


def _check(dev, shape, training, skip, seed):
    from adaptpoint_amd import propagation
    conv, bn, f1, f2, nearest, weights, gout = _setup(dev, shape, seed, skip, training)
    ref = PR.composed64(conv, bn, f1, f2, nearest, weights, gout)
    assert ref["share"] < 1e-3
    comp = _composed(conv, bn, f1, f2, nearest, weights, gout)
    before = (bn.running_mean.clone(), bn.running_var.clone(), int(bn.num_batches_tracked))
    assert propagation.supported(f1, f2, conv, bn)
    out = propagation.propagate(f1, f2, nearest, weights, conv, bn, relu=True)
    out.backward(gout)
    res = dict(out=out.detach(), g_f1=None if f1 is None else f1.grad, g_f2=f2.grad, g_w=conv.weight.grad,
               g_gamma=bn.weight.grad, g_beta=bn.bias.grad)
    e_h, e_c = _errors(res, ref, skip), _errors(comp, ref, skip)
    print("shape", shape, "train" if training else "eval", "skip" if skip else "no-skip",
          "| hoisted", {k: "%.2e" % v for k, v in e_h.items()}, "| composed", {k: "%.2e" % v for k, v in e_c.items()})
    for k in e_h:
        bar = max(PR.TOL_OUT if k == "out" else PR.TOL_GRAD, 2.0 * e_c[k])
        assert e_h[k] < bar, (k, e_h[k], "composed", e_c[k])
    if training:
        assert PR.rel(bn.running_mean, ref["bn"].running_mean) < PR.TOL_STAT
        assert PR.rel(bn.running_var, ref["bn"].running_var) < PR.TOL_STAT
        assert int(bn.num_batches_tracked) == before[2] + 1
    else:
        assert torch.equal(bn.running_mean, before[0]) and torch.equal(bn.running_var, before[1])
        assert int(bn.num_batches_tracked) == before[2]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_hoisted_block_matches_float64_modules(dev, shape):
    _check(dev, shape, True, True, seed=sum(shape))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_hoisted_block_with_running_statistics(dev, shape):
    """eval(): scale, shift and ReLU in the blend's launch; the running statistics stay untouched."""
    _check(dev, shape, False, True, seed=sum(shape) + 3)


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("shape", [SHAPES[3], SHAPES[4]], ids=lambda s: "x".join(map(str, s)))
def test_hoisted_block_without_skip_features(dev, shape, training):
    _check(dev, shape, training, False, seed=sum(shape) + 5)


def _five(dev, conv, bn, f1_0, f2_0, nearest, weights, gout):
    from adaptpoint_amd import propagation
    f1, f2 = f1_0.clone().requires_grad_(True), f2_0.clone().requires_grad_(True)
    out = propagation.propagate(f1, f2, nearest, weights, conv, bn)
    grads = torch.autograd.grad(out, [f1, f2, conv.weight, bn.weight, bn.bias], gout)
    return (out.detach(),) + tuple(grads)


def test_hoisted_block_is_bit_reproducible(dev):
    conv, bn, f1, f2, nearest, weights, gout = _setup(dev, REPRO, 9)
    runs = [[t.clone() for t in _five(dev, conv, bn, f1.detach(), f2.detach(), nearest, weights, gout)] for _ in range(2)]
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_hoisted_block_replayed_from_a_hipgraph_equals_eager(dev):
    """Forward + backward of the layer alone: no memset node, and -- fixed-order sums only -- the replay's output and
    gradients are the eager call's, bit for bit."""
    from adaptpoint_amd import graphs
    conv, bn, f1, f2, nearest, weights, gout = _setup(dev, REPRO, 11)
    f1, f2 = f1.detach(), f2.detach()
    rm, rv = bn.running_mean.clone(), bn.running_var.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                       # warm-up: allocator pools, lazy initialisation
        for _ in range(2):
            _five(dev, conv, bn, f1, f2, nearest, weights, gout)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    with torch.no_grad():
        bn.running_mean.copy_(rm)
        bn.running_var.copy_(rv)
    eager = [t.clone() for t in _five(dev, conv, bn, f1, f2, nearest, weights, gout)]
    torch.cuda.synchronize()
    gc.collect()
    graph, captured, census = graphs.capture(lambda: _five(dev, conv, bn, f1, f2, nearest, weights, gout),
                                             leaves=[conv.weight, bn.weight, bn.bias], what="the hoisted block's graph")
    graphs.assert_replayable(graph, "the hoisted block's graph")
    print("hoisted block graph:", census)
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, captured):
        assert torch.equal(a, b)


def _run_imitator(dev, oracle, hoisted):
    """tests/test_gpu_imitator.py's run of SAComponent(fused=True), with the decoders' switch."""
    from adaptpoint_amd.imitator import SAComponent
    from adaptpoint_amd.pointnext import fill_parameters_by_name
    m = fill_parameters_by_name(SAComponent(fused=True, hoisted=hoisted)).to(dev)
    assert sum(q.numel() for q in m.parameters()) == 5998062
    m.train()
    xyz = GI.unit_sphere_cloud(2, 512, seed=81)
    x = torch.from_numpy(xyz).to(dev)
    anchor = torch.from_numpy(oracle.furthest_point_sampling(xyz, 4)).long().to(dev)
    prob, logits = m(x, anchor, return_logits=True)
    w = torch.from_numpy(GI.seeded_normal((2, 2, 512), seed=82)).to(dev).permute(0, 2, 1)
    (prob.sum() + (logits * w).sum()).backward()
    res = {"g8_sac_prob": prob, "g8_sac_mask_logits": logits,
           "g8_sac_grad_embed_w": m.embedding.net[0].weight.grad,
           "g8_sac_grad_alpha0": m.pointset_grouper_list[0].affine_alpha.grad}
    return {k: v.detach().cpu().numpy() for k, v in res.items()}


def test_imitator_with_hoisted_decoders_matches_reference_golden(dev, golden, oracle):
    err = lambda a, ref: float(np.abs(a - ref).max() / max(1.0, np.abs(ref).max()))
    hoisted = _run_imitator(dev, oracle, True)
    plain = _run_imitator(dev, oracle, False)
    for key, tol in (("g8_sac_prob", 1e-2), ("g8_sac_mask_logits", 1e-2),
                     ("g8_sac_grad_embed_w", 5e-2), ("g8_sac_grad_alpha0", 5e-2)):
        assert err(hoisted[key], golden[key]) <= tol, (key, "hoisted vs reference", err(hoisted[key], golden[key]))
    for key, tol in (("g8_sac_prob", 1e-4), ("g8_sac_mask_logits", 1e-3),
                     ("g8_sac_grad_embed_w", 2e-2), ("g8_sac_grad_alpha0", 2e-2)):
        print(key, "hoisted vs plain", err(hoisted[key], plain[key]))
        assert err(hoisted[key], plain[key]) <= tol, (key, "hoisted vs plain", err(hoisted[key], plain[key]))


def test_pointnext_feature_propagation_hoisted_on_the_device(dev, golden_ap, oracle):
    from adaptpoint_amd import propagation
    from adaptpoint_amd.pointnext import FeaturePropagation, fill_parameters_by_name
    fp = fill_parameters_by_name(FeaturePropagation([64 + 32, 32, 32], hoisted=True)).to(dev).train()
    p1 = GI.unit_sphere_cloud(2, 512, seed=141)
    p2 = GI.take_points(p1, oracle.furthest_point_sampling(p1, 128))
    f1 = torch.from_numpy(GI.seeded_normal((2, 32, 512), seed=142)).to(dev).requires_grad_(True)
    f2 = torch.from_numpy(GI.seeded_normal((2, 64, 128), seed=143)).to(dev).requires_grad_(True)
    parts = propagation.block_parts(fp.convs[0])
    assert parts is not None and propagation.supported(f1, f2, parts[0], parts[1])       # the kernels, not the torch form
    out = fp([torch.from_numpy(p1).to(dev), f1], [torch.from_numpy(p2).to(dev), f2])
    (out * torch.from_numpy(GI.seeded_normal(tuple(out.shape), seed=144)).to(dev)).sum().backward()
    np.testing.assert_allclose(out.detach().cpu().numpy(), golden_ap["g14_fp_out"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(f1.grad.cpu().numpy(), golden_ap["g14_fp_grad_f1"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(f2.grad.cpu().numpy(), golden_ap["g14_fp_grad_f2"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(fp.convs[0][0].weight.grad.cpu().numpy(), golden_ap["g14_fp_grad_w0"], rtol=1e-4, atol=1e-5)


def test_joint_step_with_hoisted_decoders_replayed_from_a_hipgraph_equals_eager(dev):
    """GanStep(capturable=True) over AdaptPointAugmentor(fused=True, hoisted=True): three replayed steps against three
    eager steps from the same snapshot, by the method and the bars of tests/test_gpu_graph_replay.py (whose helpers this
    test uses as they are)."""
    import test_gpu_graph_replay as R
    from adaptpoint_amd import graphs
    from adaptpoint_amd.augmentor import AdaptPointAugmentor, Noise, draw_noise_on
    from adaptpoint_amd.discriminator import PointDiscriminator1
    from adaptpoint_amd.gan import GanStep
    from adaptpoint_amd.pointnext import PointNextSClassifier, SmoothCrossEntropy, fill_parameters_by_name
    B, N, STEPS = 4, 1024, R.STEPS
    G = fill_parameters_by_name(AdaptPointAugmentor(fused=True, hoisted=True)).to(dev)
    assert all(d.hoisted for d in G.predict_prob_layer.decode_list)
    D = R._no_dropout(fill_parameters_by_name(PointDiscriminator1(num_classes=15, fused=True))).to(dev)
    C = fill_parameters_by_name(PointNextSClassifier(fused=True)).to(dev)
    step = GanStep(G, D, C, SmoothCrossEntropy(0.3), capturable=True)
    torch.manual_seed(5)
    batches = []
    for i in range(STEPS + 1):
        pos = torch.from_numpy(GI.unit_sphere_cloud(B, N, seed=700 + i)).to(dev)
        batches.append((torch.cat([pos, R._height(pos)], -1), torch.randint(0, 15, (B,), device=dev),
                        draw_noise_on(dev, B, N, G.num_anchor)))
    points, label = batches[0][0].clone(), batches[0][1].clone()
    fields = lambda nz: (nz.keep, nz.axes, nz.kernel_axes, nz.gumbel_expo)
    noise = Noise(*[t.clone() for t in fields(batches[0][2])])

    def load(i):
        points.copy_(batches[i][0])
        label.copy_(batches[i][1])
        for dst, src in zip(fields(noise), fields(batches[i][2])):
            dst.copy_(src)

    keys = ("g_loss_raw", "feedback_loss", "g_loss", "d_loss")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            load(STEPS)
            step(points, label, noise=noise)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    mods, opts = (G, D, C), (step.opt_g, step.opt_d)
    snap = R._snapshot(mods, opts)

    def eager_run():
        out = []
        for i in range(STEPS):
            load(i)
            res = step(points, label, noise=noise)
            out.append({k: res[k].item() for k in keys})
        return out, [copy.deepcopy(m.state_dict()) for m in mods]
    eager, eager_w = eager_run()
    R._restore(mods, opts, snap)
    eager2, eager_w2 = eager_run()
    R._restore(mods, opts, snap)
    gc.collect()
    load(STEPS)
    graph, captured, census = graphs.capture(lambda: step(points, label, noise=noise), what="the hoisted joint step's graph",
                                             leaves=[q for m in mods for q in m.parameters()])
    print("hoisted joint step graph:", census)
    R._restore(mods, opts, snap)
    replayed = []
    for i in range(STEPS):
        load(i)
        graph.replay()
        torch.cuda.synchronize()
        replayed.append({k: captured[k].item() for k in keys})
    R._compare("joint step, hoisted decoders", eager, replayed, mods, eager_w, snap[0], floor=eager_w2, floor_losses=eager2)


def test_blend_entry_checks_its_arguments(dev):
    """Host-side checks only: every call returns before a launch."""
    from adaptpoint_amd import _lib
    lib = _lib.load()
    buf = torch.zeros(64, device=dev)
    ibuf = torch.zeros(64, dtype=torch.int32, device=dev)
    p, ip = buf.data_ptr(), ibuf.data_ptr()
    stream = torch.cuda.current_stream(dev).cuda_stream

    def call(b=1, o=2, m=3, n=4, a=p, u=p, idx=ip, w=p, y=p, part=p, training=1, rm=p, rv=p, out=p):
        return lib.apn_fp_blend_stats(b, o, m, n, a, u, idx, w, y, part, training, None, None, rm, rv, 1e-5, 1, None, out, stream)
    EINVAL, OK = -1, 0
    for kw in (dict(b=-1), dict(o=-1), dict(m=-1), dict(n=-1), dict(b=65536), dict(u=None), dict(idx=None), dict(w=None),
               dict(y=None), dict(part=None), dict(training=0, out=None), dict(training=0, rm=None), dict(training=0, rv=None),
               dict(m=0)):
        assert call(**kw) == EINVAL, kw
    for kw in (dict(b=0), dict(o=0), dict(n=0)):
        assert call(**kw) == OK, kw
    torch.cuda.synchronize()
    assert not buf.any() and not ibuf.any()          # nothing was launched
