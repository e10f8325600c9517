"""CPU suite for the feature-propagation block with its convolution hoisted to the coarse points
(adaptpoint_amd.propagation): W [f1 ; blend(f2)] = W[:, :C1] f1 + blend(W[:, C1:] f2).  On CPU tensors `propagate` runs
that algebra as plain torch operations; here it meets the composed block in float64, the concatenation's slice order,
the reference-made goldens of the three modules that take `hoisted=`, and an unchanged state_dict."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import golden_inputs as GI
import propagation_reference as PR


def _check(B, shape, training, skip, seed):
    from adaptpoint_amd import propagation
    C1, C2, O, n, m = shape
    conv, bn = PR.layer((C1 if skip else 0) + C2, O, seed)
    bn.train(training)
    xyz1, xyz2, f1, f2 = PR.inputs(B, C1, C2, n, m, seed + 1, skip=skip)
    idx, w = PR.nearest_weights(xyz1, xyz2)
    gout = torch.randn(B, O, n, generator=torch.Generator().manual_seed(seed + 2))
    ref = PR.composed64(conv, bn, f1, f2, idx, w, gout)
    assert ref["share"] < 1e-3, ref["share"]
    before = (bn.running_mean.clone(), bn.running_var.clone(), int(bn.num_batches_tracked))
    out = propagation.propagate(f1, f2, idx, w, conv, bn, relu=True)
    out.backward(gout)
    errs = {"out": PR.rel(out, ref["out"]), "g_f2": PR.rel(f2.grad, ref["g_f2"]), "g_w": PR.rel(conv.weight.grad, ref["g_w"]),
            "g_gamma": PR.rel(bn.weight.grad, ref["g_gamma"]), "g_beta": PR.rel(bn.bias.grad, ref["g_beta"])}
    if skip:
        errs["g_f1"] = PR.rel(f1.grad, ref["g_f1"])
    print(shape, "train" if training else "eval", "skip" if skip else "no-skip", errs, "zeroed share", ref["share"])
    assert errs.pop("out") < PR.TOL_OUT
    for name, e in errs.items():
        assert e < PR.TOL_GRAD, (name, e)
    if training:
        assert PR.rel(bn.running_mean, ref["bn"].running_mean) < PR.TOL_STAT
        assert PR.rel(bn.running_var, ref["bn"].running_var) < PR.TOL_STAT
        assert int(bn.num_batches_tracked) == int(ref["bn"].num_batches_tracked) == before[2] + 1
    else:
        assert torch.equal(bn.running_mean, before[0]) and torch.equal(bn.running_var, before[1])
        assert int(bn.num_batches_tracked) == before[2]


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("shape", PR.DECODER_SHAPES + [PR.RAGGED], ids=lambda s: "x".join(map(str, s)))
def test_hoisted_block_matches_float64_composition(shape, training):
    _check(2, shape, training, True, seed=sum(shape))


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("shape", [PR.DECODER_SHAPES[3], PR.RAGGED], ids=lambda s: "x".join(map(str, s)))
def test_hoisted_block_without_skip_features(shape, training):
    _check(2, shape, training, False, seed=sum(shape) + 7)


def test_weight_slices_follow_the_concatenation_order():
    """[f1 ; up], not [up ; f1]: with f2 = 0 the block is the skip product alone, with f1 = 0 the coarse one alone."""
    from adaptpoint_amd import propagation
    C1, C2, O, n, m = 24, 40, 16, 200, 50
    conv, bn = PR.layer(C1 + C2, O, 3)
    xyz1, xyz2, f1, f2 = PR.inputs(2, C1, C2, n, m, 4)
    f1, f2 = f1.detach(), f2.detach()
    idx, w = PR.nearest_weights(xyz1, xyz2)
    W = conv.weight.detach()
    bnf = lambda y: torch.relu(F.batch_norm(y, None, None, bn.weight, bn.bias, True, 0.1, bn.eps))
    with torch.no_grad():
        only1 = propagation.propagate(f1, torch.zeros_like(f2), idx, w, conv, bn)
        only2 = propagation.propagate(torch.zeros_like(f1), f2, idx, w, conv, bn)
        want1 = bnf(F.conv1d(f1, W[:, :C1]))
        want2 = bnf(F.conv1d(PR.blend64(f2.double(), idx, w).float(), W[:, C1:]))
    torch.testing.assert_close(only1, want1, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(only2, want2, rtol=1e-5, atol=1e-5)


def test_pointnext_feature_propagation_hoisted_meets_reference_goldens(golden_ap, cpu_mirrors, oracle):
    from adaptpoint_amd.pointnext import FeaturePropagation, PointNextDecoder, fill_parameters_by_name
    fp = fill_parameters_by_name(FeaturePropagation([64 + 32, 32, 32], hoisted=True)).train()
    p1 = GI.unit_sphere_cloud(2, 512, seed=141)
    p2 = GI.take_points(p1, oracle.furthest_point_sampling(p1, 128))
    f1 = torch.from_numpy(GI.seeded_normal((2, 32, 512), seed=142)).requires_grad_(True)
    f2 = torch.from_numpy(GI.seeded_normal((2, 64, 128), seed=143)).requires_grad_(True)
    out = fp([torch.from_numpy(p1), f1], [torch.from_numpy(p2), f2])
    (out * torch.from_numpy(GI.seeded_normal(tuple(out.shape), seed=144))).sum().backward()
    np.testing.assert_allclose(out.detach().numpy(), golden_ap["g14_fp_out"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(f1.grad.numpy(), golden_ap["g14_fp_grad_f1"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(f2.grad.numpy(), golden_ap["g14_fp_grad_f2"], rtol=1e-4, atol=1e-5)
    assert tuple(fp.convs[0][0].weight.grad.shape) == (32, 96, 1)
    np.testing.assert_allclose(fp.convs[0][0].weight.grad.numpy(), golden_ap["g14_fp_grad_w0"], rtol=1e-4, atol=1e-5)
    dec = fill_parameters_by_name(PointNextDecoder([32, 64, 128, 256, 512], decoder_layers=2, decoder_stages=4,
                                                   hoisted=True)).train()
    assert sorted(dec.state_dict().keys()) == list(golden_ap["g14_dec_keys"])
    pl = [GI.unit_sphere_cloud(2, 256, seed=146)]
    for m in (128, 64, 32, 16):
        pl.append(GI.take_points(pl[-1], oracle.furthest_point_sampling(pl[-1], m)))
    fl = [torch.from_numpy(GI.seeded_normal((2, c, n), seed=147 + i))
          for i, (c, n) in enumerate(zip((32, 64, 128, 256, 512), (256, 128, 64, 32, 16)))]
    od = dec([torch.from_numpy(q) for q in pl], fl)
    np.testing.assert_allclose(od.detach().numpy(), golden_ap["g14_dec_out"], rtol=1e-4, atol=1e-5)


def test_generator_with_hoisted_decoders_meets_reference_goldens(golden_ap, cpu_mirrors):
    from adaptpoint_amd.augmentor import AdaptPointAugmentor, draw_noise
    from adaptpoint_amd.pointnext import fill_parameters_by_name
    rel = lambda a, ref: float(np.abs(np.asarray(a, np.float64) - np.asarray(ref, np.float64)).max()
                               / max(1e-12, np.abs(np.asarray(ref, np.float64)).max()))
    g = fill_parameters_by_name(AdaptPointAugmentor(fused=False, hoisted=True))
    assert all(d.hoisted for d in g.predict_prob_layer.decode_list)
    assert sum(q.numel() for q in g.parameters()) == 5998062
    g.train()
    x = torch.from_numpy(GI.unit_sphere_cloud(2, 512, seed=91))
    torch.manual_seed(int(golden_ap["g9_seed"]))
    noise = draw_noise(2, 512, 4, with_gumbel=True)
    src, out = g(x, noise)
    (out * torch.from_numpy(GI.seeded_normal((2, 512, 3), seed=92))).sum().backward()
    ref = golden_ap["g9_gen_out"]
    assert np.array_equal(out.detach().abs().sum(-1).numpy() == 0, np.abs(ref).sum(-1) == 0)   # same mask
    assert rel(out.detach().numpy(), ref) < 2e-5
    sac = g.predict_prob_layer
    assert rel(sac.embedding.net[0].weight.grad.numpy(), golden_ap["g9_grad_embed_w"]) < 1e-3
    assert rel(sac.head.prob_head[0].weight.grad.numpy(), golden_ap["g9_grad_prob_head_w"]) < 1e-3
    assert rel(sac.extract_local_feat_masking[0].weight.grad.numpy(), golden_ap["g9_grad_mask_local_w"]) < 1e-3


def test_hoisted_imitator_keeps_the_state_dict():
    from adaptpoint_amd.imitator import SAComponent
    a, b = SAComponent(hoisted=True), SAComponent(hoisted=False)
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa.keys()) == list(sb.keys())
    assert all(sa[k].shape == sb[k].shape for k in sa)
    b.load_state_dict(sa, strict=True)
    a.load_state_dict(b.state_dict(), strict=True)


def test_pointnet2_feature_propagation_hoisted_equals_composed(cpu_mirrors):
    """`FeaturePropagation2(hoisted=True)` against its own composed form with the same state_dict (float32 on the CPU, the
    oracle's three_nn underneath both): outputs, gradients and running statistics within float32 re-association; without
    coarse coordinates (`known is None`: the broadcast variant) the switch changes nothing."""
    from adaptpoint_amd.pointnet2 import FeaturePropagation2
    from adaptpoint_amd.pointnext import fill_parameters_by_name
    a = fill_parameters_by_name(FeaturePropagation2([24 + 40, 32, 16], hoisted=True)).train()
    b = fill_parameters_by_name(FeaturePropagation2([24 + 40, 32, 16])).train()
    assert list(a.state_dict().keys()) == list(b.state_dict().keys())
    unknown = torch.from_numpy(GI.unit_sphere_cloud(2, 200, seed=171))
    known = unknown[:, :50].contiguous()
    res = []
    for mod in (a, b):
        f1 = torch.from_numpy(GI.seeded_normal((2, 24, 200), seed=172)).requires_grad_(True)
        f2 = torch.from_numpy(GI.seeded_normal((2, 40, 50), seed=173)).requires_grad_(True)
        out = mod(unknown, known, f1, f2)
        (out * torch.from_numpy(GI.seeded_normal(tuple(out.shape), seed=174))).sum().backward()
        res.append((out.detach(), f1.grad, f2.grad, mod.convs[0][0].weight.grad, mod.convs[0][1].running_var.clone()))
    for x, y in zip(*res):
        torch.testing.assert_close(x, y, rtol=1e-4, atol=1e-5)
    g = torch.from_numpy(GI.seeded_normal((2, 40, 1), seed=175))
    f1 = torch.from_numpy(GI.seeded_normal((2, 24, 200), seed=172))
    torch.testing.assert_close(a(unknown, None, f1, g), b(unknown, None, f1, g), rtol=1e-5, atol=1e-6)
