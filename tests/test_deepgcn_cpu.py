"""CPU suite: the DeepGCN modules (adaptpoint_amd/deepgcn.py) against the REFERENCE's modules captured in
tests/golden/deepgcn_golden.npz (tests/golden/make_golden_deepgcn.py) -- graphs, draws and the generator's position
included --, their refusals, and the argument checks of the new C entries (apn_knn_dilated, apn_ec_out_res,
apn_ec_bwd_prep_act)."""
import os

import numpy as np
import pytest
import torch

import deepgcn_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-5          # relative L2 per gradient tensor and activations at rtol 1e-5, as tests/test_dgcnn_cpu.py holds its golden


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "deepgcn_golden.npz"))


def _narrow(fused=False, **kw):
    from adaptpoint_amd.deepgcn import DeepGcnClassifier
    from adaptpoint_amd.pointnext import fill_parameters_by_name
    return R.no_dropout(fill_parameters_by_name(DeepGcnClassifier(fused=fused, **dict(R.NARROW, **kw))))


def _inputs(gold):
    return R.classifier_inputs(R.NARROW_B, R.NARROW_N, int(gold["a/seed"]))


def _shapes(module):
    return [(n, ",".join(str(s) for s in t.shape)) for n, t in module.state_dict().items()]


def test_state_dict_names_and_shapes_are_the_references(gold):
    from adaptpoint_amd.deepgcn import DeepGCN, DeepGcnClassifier
    assert _shapes(DeepGCN()) == list(zip(gold["d/enc_names"].tolist(), gold["d/enc_shapes"].tolist()))
    assert _shapes(DeepGcnClassifier()) == list(zip(gold["d/cls_names"].tolist(), gold["d/cls_shapes"].tolist()))
    sd = DeepGCN().state_dict()
    assert sd["head.gconv.nn.0.weight"].shape == (64, 6, 1, 1) and sd["backbone.12.body.gconv.nn.0.weight"].shape == (64, 128, 1, 1)
    assert sd["fusion_block.0.weight"].shape == (1024, 896, 1) and not any("slots" in n or n.endswith(".0.bias") for n in sd)
    assert "backbone.0.gconv.nn.1.running_var" in DeepGCN(block='plain', n_blocks=3).state_dict()
    assert DeepGCN().out_channels == 2048 and DeepGCN(is_seg=True).out_channels == 1024
    assert [m.dilation for m in DeepGCN().graph_modules()] == [1] + list(range(1, 14))
    assert [m.dilation for m in DeepGCN(use_dilation=False, n_blocks=4).graph_modules()] == [1, 1, 1, 1]
    plain = DeepGCN(block='plain', n_blocks=3).graph_modules()
    assert [m.stochastic for m in plain] == [True, False, False]          # the head's graph stays stochastic, as in the reference


def test_composed_mirror_matches_the_reference_in_training_mode(gold):
    """With the golden's torch seed the mirror makes the reference's draws: the five graphs are the stored ones
    exactly, and logits, loss, every parameter's gradient, the BatchNorm buffers and the generator's position after
    the step follow."""
    m = _narrow().train()
    pos, x, gt = _inputs(gold)
    torch.manual_seed(int(gold["a/torch_seed"]))
    logits, loss = m.get_logits_loss({'pos': pos, 'x': x}, gt, keep_graphs=True)
    loss.backward()
    assert torch.rand(1).item() == float(gold["a/next_rand"][0])
    graphs = m.encoder.last_graphs
    assert len(graphs) == 5
    random = gold["a/random"].tolist()
    assert any(random) and not all(random)
    for i, g in enumerate(graphs):
        assert g.dtype == torch.int32 and np.array_equal(g.numpy(), gold[f"a/graph/{i}"]), i
    for mod, rnd, d in zip(m.encoder.graph_modules(), random, (1, 1, 2, 3, 4)):
        strided = mod.slots.tolist() == list(range(0, 4 * d, d))
        assert mod.dilation == d and (strided != rnd or d == 1), (d, rnd, mod.slots.tolist())
    np.testing.assert_allclose(logits.detach().numpy(), gold["a/logits"], rtol=1e-5)
    np.testing.assert_allclose(loss.item(), gold["a/loss"], rtol=1e-5)
    names = [k[len("a/grad/"):] for k in gold.files if k.startswith("a/grad/")]
    params = dict(m.named_parameters())
    assert sorted(names) == sorted(params)
    errs = {}
    for n in names:
        g = params[n].grad.reshape(-1)[torch.from_numpy(R.sample_index(n, params[n].numel()))]
        errs["grad/" + n] = R.rel(g, gold["a/grad/" + n])
    buffers = dict(m.named_buffers())
    for k in gold.files:
        if k.startswith("a/buf/"):
            n = k[len("a/buf/"):]
            if n.endswith("num_batches_tracked"):
                assert int(buffers[n]) == int(gold[k]) == 1, n
            else:
                errs["buf/" + n] = R.rel(buffers[n], gold[k])
    print({k: "%.1e" % v for k, v in errs.items()})
    assert max(errs.values()) < BAR, {k: v for k, v in errs.items() if v >= BAR}


def test_composed_mirror_matches_the_reference_in_eval_mode(gold):
    """Eval mode draws torch.rand(1) per graph too (and never the permutation): logits and the generator's position."""
    m = _narrow().eval()
    pos, x, _ = _inputs(gold)
    torch.manual_seed(int(gold["a/torch_seed"]))
    with torch.no_grad():
        logits = m({'pos': pos, 'x': x})
    assert torch.rand(1).item() == float(gold["b/next_rand"][0])
    np.testing.assert_allclose(logits.numpy(), gold["b/logits"], rtol=1e-5)
    assert all(mod.slots.tolist() == list(range(0, 4 * mod.dilation, mod.dilation)) for mod in m.encoder.graph_modules())


def test_plain_blocks_match_the_reference(gold):
    m = _narrow(block='plain').train()
    pos, x, _ = _inputs(gold)
    torch.manual_seed(int(gold["a/torch_seed"]))
    with torch.no_grad():
        logits = m({'pos': pos, 'x': x})
    np.testing.assert_allclose(logits.numpy(), gold["c/logits"], rtol=1e-5)


def test_float64_restatement_agrees_with_the_golden_on_the_stored_graphs(gold):
    """The restatement the GPU tests compare against, on the reference's own graphs: the logits, within the DGCNN
    test's rule (2 x the reference's own recorded distance to float64 + 1e-6)."""
    pos, x, gt = _inputs(gold)
    graphs = [torch.from_numpy(gold[f"a/graph/{i}"]) for i in range(5)]
    r64 = R.run_deepgcn64(_narrow().train(), pos, x, graphs, gt)
    err = R.rel(gold["a/logits"], r64['logits'])
    assert err <= 2.0 * float(gold["a/err64"][0]) + 1e-6, err
    # graphs handed in are the graphs used: nothing is drawn, and nothing is kept unless asked for
    m = _narrow().train()
    torch.manual_seed(7)
    before = torch.get_rng_state()
    with torch.no_grad():
        logits = m({'pos': pos, 'x': x}, graphs=graphs)
    assert torch.equal(torch.get_rng_state(), before) and m.encoder.last_graphs is None
    np.testing.assert_allclose(logits.numpy(), gold["a/logits"], rtol=1e-5)
    with pytest.raises(ValueError):
        m({'pos': pos, 'x': x}, graphs=graphs[:4])


def test_redraw_makes_a_forwards_draws(gold):
    """redraw() moves the generator as one forward does and leaves the tables that forward would use."""
    m = _narrow().train()
    pos, x, _ = _inputs(gold)
    torch.manual_seed(int(gold["a/torch_seed"]))
    m.redraw()
    tables = [mod.slots.clone() for mod in m.encoder.graph_modules()]
    assert torch.rand(1).item() == float(gold["a/next_rand"][0])
    torch.manual_seed(int(gold["a/torch_seed"]))
    with torch.no_grad():
        m({'pos': pos, 'x': x})
    assert all(torch.equal(t, mod.slots) for t, mod in zip(tables, m.encoder.graph_modules()))


def test_refusals():
    from adaptpoint_amd.deepgcn import DeepGCN, DilatedKNN, DynConv, GraphConv, ResDynBlock
    with pytest.raises(NotImplementedError, match="assert"):
        DeepGCN(block='dense')
    for conv in ('mr', 'mrconv'):
        with pytest.raises(NotImplementedError, match="unsequence"):
            DeepGCN(conv=conv)
        with pytest.raises(NotImplementedError, match="unsequence"):
            GraphConv(16, 16, conv)
        with pytest.raises(NotImplementedError, match="unsequence"):
            DynConv(16, 16, conv, 4, 2)
        with pytest.raises(NotImplementedError, match="unsequence"):
            ResDynBlock(16, conv, 4, 2)
    with pytest.raises(ValueError):                                   # k d > N: the reference's topk fails there too
        DilatedKNN(4, 3)(torch.zeros(1, 11, 3))
    assert DilatedKNN(4, 3)(torch.arange(36.).view(1, 12, 3)).shape == (1, 12, 4)
    with pytest.raises(ValueError):
        DeepGCN(in_channels=3, channels=16, emb_dims=32, n_blocks=3, k=4)(torch.zeros(1, 7, 3))


def test_cpu_tensors_are_refused_by_the_operators():
    from adaptpoint_amd import edge_conv, layers
    with pytest.raises(RuntimeError, match="CUDA/HIP"):
        layers.knn_dilated(torch.zeros(1, 8, 3), torch.zeros(1, 8, 3), 2, 2)
    with pytest.raises(RuntimeError, match="CUDA/HIP"):
        edge_conv.edge_index(torch.zeros(1, 8, 4, dtype=torch.int32))
    assert not layers.knn_dilated_covers(torch.zeros(1, 8, 3), torch.zeros(1, 8, 3), 2, 2)
    assert layers.KNN_WIDE_MAX == 256


def test_fused_model_on_cpu_tensors_runs_composed_without_a_fallback_entry(gold):
    from adaptpoint_amd import set_abstraction as SA
    before = dict(SA.FUSED_FALLBACKS)
    m = _narrow(fused=True).eval()
    pos, x, _ = _inputs(gold)
    torch.manual_seed(int(gold["a/torch_seed"]))
    with torch.no_grad():
        logits = m({'pos': pos, 'x': x})
    np.testing.assert_allclose(logits.numpy(), gold["b/logits"], rtol=1e-5)
    assert SA.FUSED_FALLBACKS == before


def test_argument_validation_of_the_new_entries_needs_no_gpu():
    """apn_knn_dilated, apn_ec_out_res and apn_ec_bwd_prep_act reject bad sizes and null pointers before any HIP call,
    and accept empty work (P: a non-null, 16-byte aligned address that is never read).  Nothing launches."""
    from adaptpoint_amd import _lib
    lib = _lib.load()
    EINVAL, P, NAN = -1, 4096, float('nan')

    def knn(b=0, n=300, m=300, c=3, kd=208, k=16, dilation=13, slots=None, support=P, query=P, idx=P, dist2=None):
        return lib.apn_knn_dilated(b, n, m, c, kd, k, dilation, slots, support, query, idx, dist2, None)

    def bad(**kw):          # a refusal must not depend on the work being empty: asked with b = 2 and with b = 0
        return knn(b=2, **kw) == EINVAL and knn(b=0, **kw) == EINVAL
    assert knn() == 0 and knn(b=2, m=0) == 0 and knn(slots=P) == 0 and knn(dist2=P) == 0
    assert knn(support=None, query=None, idx=None) == 0                                     # empty work reads nothing
    assert knn(kd=256, k=64, dilation=4) == 0 and knn(kd=1, k=1, dilation=1) == 0 and knn(n=208) == 0
    assert bad(kd=0, k=1) and bad(kd=257, k=16, dilation=16) and bad(n=207)                 # 1 <= kd <= 256, kd <= n
    assert bad(k=0) and bad(kd=256, k=65, dilation=1) and bad(kd=8, k=9, dilation=1)        # 1 <= k <= 64, k <= kd
    assert bad(dilation=0) and bad(dilation=14) and bad(kd=195)                             # null slots: (k-1) d < kd
    assert knn(dilation=0, slots=P) == 0 and knn(dilation=14, slots=P) == 0                 # (a table replaces the stride)
    assert bad(c=0) and bad(c=129) and bad(n=0, kd=1, k=1, dilation=1)
    assert knn(b=-1) == EINVAL and bad(m=-1) and knn(b=65536, n=256, m=4) == EINVAL
    assert knn(b=1 << 12, n=1 << 12, m=4) == EINVAL and knn(b=1 << 12, m=1 << 12) == EINVAL  # b * max(n, m) >= 2^24
    for name in ("support", "query", "idx"):
        assert knn(b=2, **{name: None}) == EINVAL, name

    def out(b=2, n=16, c=64, ext=P, pack=P, slope=0.0, res=P, o=P):
        return lib.apn_ec_out_res(b, n, c, ext, pack, slope, res, 16 * c, 16, 1, o, None)

    def prep(b=2, n=16, c=64, g=P, ext=P, pack=P, slope=0.0, gsel=P, part_s=P):
        return lib.apn_ec_bwd_prep_act(b, n, c, g, 16 * c, 16, 1, ext, pack, slope, gsel, part_s, None)

    pointers = {out: ["ext", "pack", "o"], prep: ["g", "ext", "pack", "gsel", "part_s"]}
    for entry, names in pointers.items():
        for name in names:
            assert entry(**{name: None}) == EINVAL, (entry.__name__, name)
        assert entry(b=0) == 0 and entry(n=0) == 0, entry.__name__                              # empty work
        assert entry(b=-1) == EINVAL and entry(n=-1) == EINVAL and entry(b=65536, n=1) == EINVAL, entry.__name__
        assert entry(c=96) == EINVAL and entry(c=0) == EINVAL, entry.__name__
        # ReLU (slope 0) and LeakyReLU are accepted -- asked on empty work, so nothing launches --, the rest refused
        assert entry(b=0, slope=0.0) == 0 and entry(b=0, slope=0.2) == 0, entry.__name__
        assert entry(b=0, slope=-0.1) == EINVAL and entry(b=0, slope=NAN) == EINVAL, entry.__name__
        assert entry(slope=-0.1) == EINVAL and entry(slope=NAN) == EINVAL, entry.__name__
    assert out(b=0, res=None) == 0 and out(n=0, res=None) == 0                                  # no residual
    # apn_ec_out / apn_ec_bwd_prep still refuse ReLU
    assert lib.apn_ec_out(0, 16, 64, P, P, 0.0, P, None) == EINVAL
