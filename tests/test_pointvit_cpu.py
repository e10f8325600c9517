"""CPU suite: the PointViT modules (adaptpoint_amd/pointvit.py) against the REFERENCE's modules captured in
tests/golden/pointvit_golden.npz (tests/golden/make_golden_pointvit.py): names and shapes, the composed mirror in training
and eval mode with both groupers, the float64 restatement the GPU tests compare against, plain-dict arguments, the
fallback reasons of the fused attention on CPU tensors, `forward_seg_feat`, and a reference-named state_dict."""
import os

import numpy as np
import pytest
import torch

import pointvit_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-5          # relative L2 per gradient tensor and buffer, as tests/test_pointmlp_cpu.py holds them; activations: rtol 1e-5


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "pointvit_golden.npz"))


def _narrow(group='knn', fused=False, **over):
    from adaptpoint_amd.pointvit import PointVitClassifier
    from adaptpoint_amd.pointnext import fill_parameters_by_name
    return R.no_dropout(fill_parameters_by_name(PointVitClassifier(fused=fused, **R.narrow(group, **over))))


def _inputs(gold):
    return R.classifier_inputs(R.NARROW_B, R.NARROW_N, int(gold["a/seed"]))


def test_state_dict_names_and_shapes_are_the_references(gold):
    from adaptpoint_amd.pointvit import PointViT
    m = PointViT()
    got = [(n, ",".join(str(s) for s in t.shape)) for n, t in m.state_dict().items()]
    assert got == list(zip(gold["d/vit_names"].tolist(), gold["d/vit_shapes"].tolist()))
    sd = m.state_dict()
    assert sd["blocks.11.attn.qkv.weight"].shape == (1152, 384) and "blocks.0.attn.qkv.bias" not in sd
    assert sd["cls_token"].shape == (1, 1, 384) and sd["pos_embed.0.0.weight"].shape == (128, 3)
    assert m.out_channels == 768 and m.get_num_layers() == 12 and 'cls_token' in m.no_weight_decay()
    assert m.channel_list == [3, 384] and m.global_feat == ['cls', 'max'] and m.add_pos_each_block and m.n_tokens == 1
    assert PointViT(distill=True).n_tokens == 2 and "dist_token" in PointViT(distill=True, depth=1).state_dict()


def _check_training(m, gold, tag, index):
    pos, x, gt = _inputs(gold)
    logits, loss = m.get_logits_loss({'pos': pos, 'x': x}, gt, index=index)
    loss.backward()
    np.testing.assert_allclose(logits.detach().numpy(), gold[f"{tag}/logits"], rtol=1e-5)
    np.testing.assert_allclose(loss.item(), gold[f"{tag}/loss"], rtol=1e-5)
    names = [k[len(f"{tag}/grad/"):] for k in gold.files if k.startswith(f"{tag}/grad/")]
    params = dict(m.named_parameters())
    assert set(names) <= set(params) and (tag != "a" or sorted(names) == sorted(params))
    errs = {}
    for n in names:
        g = params[n].grad.reshape(-1)[torch.from_numpy(R.sample_index(n, params[n].numel()))]
        errs["grad/" + n] = R.rel(g, gold[f"{tag}/grad/" + n])
    buffers = dict(m.named_buffers())
    for k in gold.files:
        if k.startswith(f"{tag}/buf/"):
            n = k[len(f"{tag}/buf/"):]
            if n.endswith("num_batches_tracked"):
                assert int(buffers[n]) == int(gold[k]) == 1, n
            else:
                errs["buf/" + n] = R.rel(buffers[n], gold[k])
    print({k: "%.1e" % v for k, v in errs.items()})
    assert max(errs.values()) < BAR, {k: v for k, v in errs.items() if v >= BAR}


def test_composed_mirror_matches_the_reference_in_training_mode(gold, cpu_mirrors):
    """Logits, loss, every parameter's gradient and the BatchNorm buffers after the step.  On CPU the mirror's sampler is
    the oracle's and its neighbours are the reference's own cdist / topk call."""
    _check_training(_narrow().train(), gold, "a", None)


def test_composed_mirror_matches_the_reference_with_the_ball_query_grouper(gold, cpu_mirrors):
    m = _narrow('ballquery').train()
    pos, _, _ = _inputs(gold)
    idx, nbr = m.encoder.patch_embed.index(pos)
    assert nbr.shape == (R.NARROW_B, 16, 8) and nbr.dtype == torch.int32
    centre = torch.gather(pos, 1, idx.long().unsqueeze(-1).expand(-1, -1, 3))
    assert bool(((pos.unsqueeze(1) - centre.unsqueeze(2)).norm(dim=-1) < R.RADIUS).any(-1).all()), "an empty ball"
    _check_training(m, gold, "c", (idx, nbr))


def test_composed_mirror_matches_the_reference_in_eval_mode(gold, cpu_mirrors):
    m = _narrow().eval()
    pos, x, _ = _inputs(gold)
    with torch.no_grad():
        logits = m({'pos': pos, 'x': x})
        feat = m.encoder.forward_cls_feat(pos, x)
    np.testing.assert_allclose(logits.numpy(), gold["b/logits"], rtol=1e-5)
    assert feat.shape == (R.NARROW_B, 256)


def test_float64_restatement_agrees_with_the_fixture(gold, cpu_mirrors):
    """The restatement the GPU tests compare against, on the fixture's input with the mirror's own index (the fixture's
    err64 records the reference's own distance), for both groupers."""
    pos, x, gt = _inputs(gold)
    for group, tag in (('knn', 'a'), ('ballquery', 'c')):
        m = _narrow(group).train()
        index = m.encoder.patch_embed.index(pos)
        assert index[0].shape == (R.NARROW_B, 16) and index[1].shape == (R.NARROW_B, 16, 8)
        r64 = R.run_classifier64(m, pos, x, index, gt)
        err = R.rel(gold[f"{tag}/logits"], r64['logits'])
        assert err <= 2.0 * float(gold[f"{tag}/err64"][0]) + 1e-6, (group, err)
        err = R.rel(gold[f"{tag}/loss"], r64['loss'])
        assert err <= 2.0 * float(gold[f"{tag}/err64"][1]) + 1e-6, (group, err)


def test_fused_model_on_cpu_tensors_falls_back_counted_and_equals_the_composed(gold, cpu_mirrors):
    from adaptpoint_amd import token_attention as TA
    pos, x, _ = _inputs(gold)
    before = dict(TA.COMPOSED_CALLS)
    with torch.no_grad():
        a = _narrow(fused=None).eval()({'pos': pos, 'x': x})
        assert TA.COMPOSED_CALLS.get("cpu tensor", 0) == before.get("cpu tensor", 0) + 2          # one per block
        b = _narrow(fused=False).eval()({'pos': pos, 'x': x})
        assert TA.COMPOSED_CALLS.get("cpu tensor", 0) == before.get("cpu tensor", 0) + 2          # fused=False is not counted
    assert torch.equal(a, b)
    # attention dropout in training has its own reason; in eval mode it is no reason
    from adaptpoint_amd.pointvit import Attention
    att = Attention(128, num_heads=2, attn_drop=0.25).train()
    att(torch.randn(2, 5, 128))
    reasons = [r for r in TA.COMPOSED_CALLS if "attention dropout 0.25" in r]
    assert len(reasons) == 1
    n = TA.COMPOSED_CALLS[reasons[0]]
    att.eval()(torch.randn(2, 5, 128))
    assert TA.COMPOSED_CALLS[reasons[0]] == n
    assert not TA.supported(torch.empty(2, 5, 3 * 128), 2)
    TA.COMPOSED_CALLS.clear()
    TA.COMPOSED_CALLS.update(before)


def test_plain_dict_arguments_every_feature_type_and_both_reductions(cpu_mirrors):
    """embed_args / norm_args / act_args as plain dicts; all feature types, relative_xyz, normalize_dp, mean / max, both
    groupers, bn norms: the modules build with the reference's parameter names and run."""
    from adaptpoint_amd.pointvit import PointViT, PointPatchEmbed, CHANNEL_MAP
    pos, x, _ = R.classifier_inputs(2, 32, 0)
    for ft in CHANNEL_MAP:
        for group, reduction, norm, ndp, rel_xyz in (('knn', 'max', 'in2d', False, True), ('ballquery', 'mean', 'bn', True, True),
                                                     ('knn', 'avg', 'bn2d', True, False)):
            pe = PointPatchEmbed(sample_ratio=0.25, group_size=4, in_channels=4, embed_dim=16, group=group, radius=0.7,
                                 feature_type=ft, norm_args={'norm': norm}, reduction=reduction, normalize_dp=ndp,
                                 relative_xyz=rel_xyz).eval()
            assert pe.conv1[0][0].in_channels == CHANNEL_MAP[ft](4)
            with torch.no_grad():
                p_list, x_list = pe(pos, x)
            assert p_list[1].shape == (2, 8, 3) and x_list[1].shape == (2, 16, 8) and torch.isfinite(x_list[1]).all(), (ft, group)
    m = PointViT(in_channels=4, embed_dim=64, depth=2, num_heads=1, fused=False,
                 embed_args={'NAME': 'PointPatchEmbed', 'sample_ratio': 0.25, 'group_size': 4, 'group': 'knn',
                             'feature_type': 'dp_df', 'norm_args': {'norm': 'in2d'}},
                 norm_args={'norm': 'ln', 'eps': 1e-6}, act_args={'act': 'gelu'}, drop_path_rate=0.1, global_feat='cls,max,avg')
    assert m.out_channels == 192 and isinstance(m.blocks[0].drop_path, torch.nn.Identity) and m.blocks[1].drop_path.drop_prob > 0
    p_list, x_list = m.eval().forward_seg_feat({'pos': pos, 'x': x})
    assert [t.shape for t in p_list] == [(2, 32, 3), (2, 8, 3)]
    assert x_list[0].shape == (2, 4, 32) and x_list[1].shape == (2, 64, 9)                 # cls + 8 group tokens
    assert m.forward_cls_feat(pos, x).shape == (2, 192)
    torch.manual_seed(0)
    assert m.train().forward_cls_feat(pos, x).shape == (2, 192)                             # DropPath draws


def test_a_reference_named_state_dict_loads_strictly(gold):
    from adaptpoint_amd.pointvit import PointViT
    names, shapes = gold["d/vit_names"].tolist(), gold["d/vit_shapes"].tolist()
    sd = {n: torch.full([int(s) for s in sh.split(",")] if sh else [], 0.5) for n, sh in zip(names, shapes)}
    m = PointViT()
    assert not any(m.load_state_dict(sd, strict=True))
    assert float(m.blocks[3].mlp.fc2.weight.detach()[0, 0]) == 0.5


def test_transformer_encoder_forward_features_picks_the_references_depths():
    from adaptpoint_amd.pointvit import TransformerEncoder
    enc = TransformerEncoder(embed_dim=64, depth=4, num_heads=1, fused=False).eval()
    x, pos = torch.randn(2, 5, 64), torch.randn(2, 5, 64)
    with torch.no_grad():
        outs = enc.forward_features(x, pos, num_outs=2)
        assert len(outs) == 2 and torch.equal(outs[-1], enc(x, pos))
