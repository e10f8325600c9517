"""CPU suite: the DGCNN modules (adaptpoint_amd/dgcnn.py) against the REFERENCE's modules captured in
tests/golden/dgcnn_golden.npz (tests/golden/make_golden_dgcnn.py), their refusals, the argument checks of the new C
entries (apn_knn_query, apn_ec_*) and the plain-value coverage rule of the fused EdgeConv block."""
import os

import numpy as np
import pytest
import torch

import dgcnn_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-5          # relative L2 per gradient tensor, as tests/test_invres_cpu.py holds them; activations: rtol 1e-5


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "dgcnn_golden.npz"))


def _narrow(fused=False):
    from adaptpoint_amd.dgcnn import DgcnnClassifier
    from adaptpoint_amd.pointnext import fill_parameters_by_name
    return R.no_dropout(fill_parameters_by_name(DgcnnClassifier(fused=fused, **R.NARROW)))


def _shapes(module):
    return [(n, ",".join(str(s) for s in t.shape)) for n, t in module.state_dict().items()]


def test_state_dict_names_and_shapes_are_the_references(gold):
    from adaptpoint_amd.dgcnn import DGCNN, DgcnnClassifier
    assert _shapes(DGCNN()) == list(zip(gold["d/enc_names"].tolist(), gold["d/enc_shapes"].tolist()))
    assert _shapes(DgcnnClassifier()) == list(zip(gold["d/cls_names"].tolist(), gold["d/cls_shapes"].tolist()))
    sd = DGCNN().state_dict()
    assert sd["head.gconv.nn.0.weight"].shape == (64, 6, 1, 1) and sd["backbone.2.gconv.nn.0.weight"].shape == (256, 256, 1, 1)
    assert sd["fusion_block.0.weight"].shape == (1024, 512, 1) and "fusion_block.1.running_var" in sd
    assert DGCNN().out_channels == 2048 and DGCNN(is_seg=True).out_channels == 1024


def test_composed_mirror_matches_the_reference_in_training_mode(gold):
    """Logits, loss, every parameter's gradient and the BatchNorm buffers after the step.  On CPU the mirror's graphs
    are the reference's own cdist / topk call on the same activations."""
    m = _narrow().train()
    pos, x, gt = R.classifier_inputs(R.NARROW_B, R.NARROW_N, int(gold["a/seed"]))
    logits, loss = m.get_logits_loss({'pos': pos, 'x': x}, gt)
    loss.backward()
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
    m = _narrow().eval()
    pos, x, _ = R.classifier_inputs(R.NARROW_B, R.NARROW_N, int(gold["a/seed"]))
    with torch.no_grad():
        logits = m({'pos': pos, 'x': x})
    np.testing.assert_allclose(logits.numpy(), gold["b/logits"], rtol=1e-5)


def test_float64_restatement_agrees_with_the_mirror_on_what_rounding_cannot_move(gold):
    """The restatement the GPU tests compare against, on the fixture's input with the mirror's own graphs: the logits
    and the loss (forward values; the fixture's a/err64 records the reference's own distance)."""
    m = _narrow().train()
    pos, x, gt = R.classifier_inputs(R.NARROW_B, R.NARROW_N, int(gold["a/seed"]))
    with torch.no_grad():
        m({'pos': pos, 'x': x}, keep_graphs=True)
    graphs = m.encoder.last_graphs
    assert len(graphs) == 4 and all(g.shape == (R.NARROW_B, R.NARROW_N, R.NARROW['k']) for g in graphs)
    r64 = R.run_classifier64(_narrow().train(), pos, x, graphs, gt)
    err = R.rel(gold["a/logits"], r64['logits'])
    assert err <= 2.0 * float(gold["a/err64"][0]) + 1e-6, err
    # graphs handed in are the graphs used, and nothing is kept unless asked for
    with torch.no_grad():
        again = _narrow().train()
        again({'pos': pos, 'x': x}, graphs=graphs)
    assert again.encoder.last_graphs is None


def test_refusals():
    from adaptpoint_amd.dgcnn import DGCNN, DynConv, GraphConv
    with pytest.raises(NotImplementedError):
        DynConv(16, 16, 'edge', 8, dilation=2)
    with pytest.raises(NotImplementedError):
        DynConv(16, 16, 'edge', 8, stochastic=True, epsilon=0.2)
    with pytest.raises(NotImplementedError):
        GraphConv(16, 16, 'mr')
    with pytest.raises(NotImplementedError):
        DGCNN(conv='mr')
    with pytest.raises(NotImplementedError):
        DGCNN(use_stochastic=True)
    with pytest.raises(NotImplementedError):
        DGCNN(dilation=2)


def test_fused_model_on_cpu_tensors_runs_composed_without_a_fallback_entry(gold):
    from adaptpoint_amd import set_abstraction as SA
    before = dict(SA.FUSED_FALLBACKS)
    m = _narrow(fused=True).eval()
    pos, x, _ = R.classifier_inputs(R.NARROW_B, R.NARROW_N, int(gold["a/seed"]))
    with torch.no_grad():
        logits = m({'pos': pos, 'x': x})
    np.testing.assert_allclose(logits.numpy(), gold["b/logits"], rtol=1e-5)
    assert SA.FUSED_FALLBACKS == before


def test_cpu_tensors_are_refused_by_the_operators():
    from adaptpoint_amd import edge_conv, layers
    with pytest.raises(RuntimeError, match="CUDA/HIP"):
        layers.knn_query(torch.zeros(1, 8, 3), torch.zeros(1, 8, 3), 4)
    with pytest.raises(RuntimeError, match="CUDA/HIP"):
        edge_conv.edge_index(torch.zeros(1, 8, 4, dtype=torch.int32))
    assert not layers.knn_covers(torch.zeros(1, 8, 3), torch.zeros(1, 8, 3), 4)
    # KnnGrouper keeps the cdist / topk line for CPU tensors
    idx = layers.KnnGrouper(3).neighbours(torch.arange(24.).view(1, 8, 3), torch.arange(24.).view(1, 8, 3))
    assert idx.shape == (1, 8, 3) and idx.dtype == torch.int32 and idx[0, :, 0].tolist() == list(range(8))


def test_edge_conv_covers_on_plain_values():
    from adaptpoint_amd.edge_conv import covers
    for H in (64, 128, 256, 512):
        for C in (3, 4, 64, 128, 256):
            for K in (1, 20, 64):
                assert covers(32, 1024, K, C, H)
    assert not covers(32, 1024, 20, 64, 96) and not covers(32, 1024, 20, 5, 64) and not covers(32, 1024, 65, 64, 64)
    assert not covers(32, 1024, 0, 64, 64) and not covers(32, 1024, 20, 64, 64, biased=True)
    assert not covers(32, 1024, 20, 64, 64, momentum=None) and not covers(0, 1024, 20, 64, 64)
    assert not covers(65536, 16, 20, 64, 64) and not covers(1 << 12, 1 << 12, 20, 64, 64)


def test_argument_validation_of_the_new_entries_needs_no_gpu():
    """apn_knn_query and the apn_ec_* entries reject bad sizes and null pointers before any HIP call, and accept empty
    work (P: a non-null, 16-byte aligned address that is never read)."""
    from adaptpoint_amd import _lib
    lib = _lib.load()
    EINVAL, P = -1, 4096

    def knn(b=2, n=16, m=16, c=3, k=4, support=P, query=P, idx=P, dist2=None):
        return lib.apn_knn_query(b, n, m, c, k, support, query, idx, dist2, None)
    assert knn(b=0) == 0 and knn(m=0) == 0 and knn(b=0, support=None, query=None, idx=None) == 0
    assert knn(k=17) == EINVAL and knn(n=100, k=65) == EINVAL and knn(k=0) == EINVAL          # k > n, k > 64, k < 1
    assert knn(c=129) == EINVAL and knn(c=0) == EINVAL and knn(n=0, k=1) == EINVAL
    assert knn(b=-1) == EINVAL and knn(m=-1) == EINVAL and knn(b=65536, n=4, m=4) == EINVAL
    assert knn(b=1 << 12, n=1 << 12) == EINVAL and knn(b=1 << 12, m=1 << 12) == EINVAL        # b * max(n, m) >= 2^24
    assert knn(support=None) == EINVAL and knn(query=None) == EINVAL and knn(idx=None) == EINVAL

    assert lib.apn_ec_pool_rows(2, 100) == 4 and lib.apn_ec_pool_rows(0, 100) == 0
    assert lib.apn_ec_bwd_prep_rows(3, 65) == 6 and lib.apn_ec_bwd_prep_rows(3, 0) == 0

    def fwd(b=2, n=16, c=64, k=4, uv=P, ld=128, idx=P, gamma=None, ext=P, sel=P, ysum=P, part=P):
        return lib.apn_ec_pool_fwd(b, n, c, k, uv, ld, idx, gamma, ext, sel, ysum, part, None)

    def out(b=2, n=16, c=64, ext=P, pack=P, slope=0.2, o=P):
        return lib.apn_ec_out(b, n, c, ext, pack, slope, o, None)

    def prep(b=2, n=16, c=64, g=P, ext=P, pack=P, slope=0.2, gsel=P, part_s=P):
        return lib.apn_ec_bwd_prep(b, n, c, g, 16 * c, 16, 1, ext, pack, slope, gsel, part_s, None)

    def csr(b=2, n=16, k=4, idx=P, pcnt_poff=P, plist=P, scratch=P):
        return lib.apn_ec_csr(b, n, k, idx, pcnt_poff, plist, scratch, None)

    def bwd(b=2, n=16, c=64, k=4, gsel=P, sel=P, pcnt_poff=P, plist=P, uv=P, ld=128, ysum=None, de=P, duv=P):
        return lib.apn_ec_pool_bwd(b, n, c, k, gsel, sel, pcnt_poff, plist, uv, ld, ysum, de, duv, None)

    pointers = {fwd: ["uv", "idx", "ext", "sel"], out: ["ext", "pack", "o"], prep: ["g", "ext", "pack", "gsel", "part_s"],
                csr: ["idx", "pcnt_poff", "plist", "scratch"], bwd: ["gsel", "sel", "pcnt_poff", "plist", "uv", "de", "duv"]}
    for entry, names in pointers.items():
        for name in names:
            assert entry(**{name: None}) == EINVAL, (entry.__name__, name)
        assert entry(b=0) == 0 and entry(n=0) == 0, entry.__name__                              # empty work
        assert entry(b=-1) == EINVAL and entry(n=-1) == EINVAL and entry(b=65536, n=1) == EINVAL, entry.__name__
    for entry in (fwd, csr, bwd):
        assert entry(k=0) == EINVAL and entry(k=65) == EINVAL, entry.__name__
        assert entry(b=1 << 12, n=1 << 12) == EINVAL, entry.__name__                            # b * n >= 2^24
    for entry in (fwd, bwd):
        assert entry(c=96) == EINVAL and entry(c=1024) == EINVAL and entry(c=0) == EINVAL, entry.__name__
        assert entry(ld=127) == EINVAL and entry(ld=130) == EINVAL, entry.__name__              # ld >= 2c, ld % 4 == 0
    assert fwd(ysum=None) == EINVAL and fwd(part=None) == EINVAL                                # both or neither
    for entry in (out, prep):
        assert entry(c=96) == EINVAL and entry(c=0) == EINVAL, entry.__name__
        assert entry(slope=0.0) == EINVAL and entry(slope=-0.1) == EINVAL, entry.__name__
