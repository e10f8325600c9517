"""CPU suite: the PointMLP modules (adaptpoint_amd/pointmlp.py) against the REFERENCE's modules captured in
tests/golden/pointmlp_golden.npz (tests/golden/make_golden_pointmlp.py), the hoisted algebra of
adaptpoint_amd/affine_group.py against the composed one in float64, the plain-value coverage rule of the fused stage and
the argument checks of the new C entries (apn_ag_*)."""
import os

import numpy as np
import pytest
import torch

import pointmlp_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-5          # relative L2 per gradient tensor and buffer, as tests/test_dgcnn_cpu.py holds them; activations: rtol 1e-5


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "pointmlp_golden.npz"))


def _narrow(fused=False):
    from adaptpoint_amd.pointmlp import PointMlpClassifier
    from adaptpoint_amd.pointnext import fill_parameters_by_name
    return R.no_dropout(fill_parameters_by_name(PointMlpClassifier(fused=fused, **R.NARROW)))


def _shapes(module):
    return [(n, ",".join(str(s) for s in t.shape)) for n, t in module.state_dict().items()]


def test_state_dict_names_and_shapes_are_the_references(gold):
    from adaptpoint_amd.pointmlp import PointMLP, PointMLPEncoder, pointMLP, pointMLPElite
    for tag, model in (("enc", PointMLPEncoder()), ("cls", PointMLP()), ("elite", pointMLPElite())):
        assert _shapes(model) == list(zip(gold[f"d/{tag}_names"].tolist(), gold[f"d/{tag}_shapes"].tolist())), tag
    assert _shapes(pointMLP()) == _shapes(PointMLPEncoder())
    sd = PointMLP().state_dict()
    assert sd["local_grouper_list.0.affine_alpha"].shape == (1, 1, 1, 64)
    assert sd["pre_blocks_list.0.transfer.net.0.weight"].shape == (128, 128, 1)
    assert sd["pos_blocks_list.3.operation.1.net2.0.weight"].shape == (1024, 1024, 1) and "classifier.8.bias" in sd
    assert PointMLPEncoder().out_channels == 1024 and pointMLPElite().out_channels == 256


def test_composed_mirror_matches_the_reference_in_training_mode(gold, cpu_mirrors):
    """Logits, loss, every parameter's gradient and the BatchNorm buffers after the step.  On CPU the mirror's sampler
    is the oracle's and its neighbours are the reference's own square_distance / topk call."""
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


def test_composed_mirror_matches_the_reference_in_eval_mode(gold, cpu_mirrors):
    m = _narrow().eval()
    pos, x, _ = R.classifier_inputs(R.NARROW_B, R.NARROW_N, int(gold["a/seed"]))
    with torch.no_grad():
        logits = m({'pos': pos, 'x': x})
        feat = m.encoder.forward_cls_feat(pos, x)                  # tensors or the reference's dict
    np.testing.assert_allclose(logits.numpy(), gold["b/logits"], rtol=1e-5)
    assert torch.equal(feat, logits)


def test_float64_restatement_agrees_with_the_fixture(gold, cpu_mirrors):
    """The restatement the GPU tests compare against, on the fixture's input with the mirror's own graphs (the
    fixture's a/err64 records the reference's own distance); graphs handed in are the graphs used."""
    m = _narrow().train()
    pos, x, gt = R.classifier_inputs(R.NARROW_B, R.NARROW_N, int(gold["a/seed"]))
    graphs = m.encoder.index(pos)
    assert len(graphs) == 4
    for i, g in enumerate(graphs):
        S = R.NARROW_N >> (i + 1)
        assert g.idx.shape == (R.NARROW_B, S, 8) and g.fps_idx.shape == (R.NARROW_B, S) and g.new_xyz.shape == (R.NARROW_B, S, 3)
        assert g.idx.dtype == g.fps_idx.dtype == torch.int32 and g.nbr_list is None
    r64 = R.run_classifier64(_narrow().train(), pos, x, graphs, gt)
    err = R.rel(gold["a/logits"], r64['logits'])
    assert err <= 2.0 * float(gold["a/err64"][0]) + 1e-6, err
    with torch.no_grad():
        a = m({'pos': pos, 'x': x}, graphs=graphs, keep_graphs=True)
        assert all(u is v for u, v in zip(m.encoder.last_graphs, graphs))
        b = _narrow().train()({'pos': pos, 'x': x})
        assert m.encoder.last_graphs is not None and torch.equal(a, b)
        m({'pos': pos, 'x': x})
    assert m.encoder.last_graphs is None
    with pytest.raises(ValueError):
        m({'pos': pos, 'x': x}, graphs=graphs[:3])


def _stage_case(B, N, S, K, C, O, seed):
    g = torch.Generator().manual_seed(seed)
    pts = torch.randn(B, N, C, generator=g, dtype=torch.float64)
    idx = torch.randint(0, N, (B, S, K), generator=g)
    fps = torch.randint(0, N, (B, S), generator=g)               # (anchors may repeat)
    alpha = 1 + 0.3 * torch.randn(C, generator=g, dtype=torch.float64)
    beta = 0.3 * torch.randn(C, generator=g, dtype=torch.float64)
    w = torch.randn(O, 2 * C, 1, generator=g, dtype=torch.float64) / (2 * C) ** 0.5
    gy = torch.randn(B, O, S * K, generator=g, dtype=torch.float64)
    return pts, idx, fps, alpha, beta, w, gy


@pytest.mark.parametrize("shape", [(2, 20, 7, 5, 6, 9), (4, 64, 32, 8, 16, 32), (1, 8, 1, 1, 2, 3)])
def test_hoisted_formula_equals_the_composed_one_in_float64(shape):
    """Forward, and the hand-written backward pass (what the kernels compute) against autograd of the composed form:
    dx with its sigma path, the gradients of Wa, W2 and c0 chained to W, alpha and beta."""
    pts, idx, fps, alpha, beta, w, gy = _stage_case(*shape, seed=5)
    leaves = [t.clone().requires_grad_(True) for t in (pts, alpha, beta, w)]
    y = R.composed_first_layer(leaves[0], idx, fps, leaves[1], leaves[2], leaves[3])
    gx, galpha, gbeta, gw = torch.autograd.grad(y, leaves, gy)
    yh, saved = R.hoisted_forward(pts, idx, fps, alpha, beta, w)
    assert R.rel(yh, y) < 1e-12
    res = R.hoisted_backward(gy, pts, idx, fps, saved)
    assert R.rel(res['dx'], gx) < 1e-12
    C = pts.shape[2]
    w1 = w.reshape(w.shape[0], 2 * C)[:, :C]
    gw1 = res['dwa'] * alpha.view(1, C) + res['dc0'].view(-1, 1) * beta.view(1, C)
    assert R.rel(torch.cat([gw1, res['dw2']], 1), gw.reshape(-1, 2 * C)) < 1e-12
    assert R.rel((res['dwa'] * w1).sum(0), galpha) < 1e-12 and R.rel(w1.t() @ res['dc0'], gbeta) < 1e-12
    # and the sigma path is a real part of dx
    no_sigma = R.hoisted_backward(gy, pts, idx, fps, saved, sigma_path=False)['dx']
    y2 = R.composed_first_layer(leaves[0], idx, fps, leaves[1], leaves[2], leaves[3], detach_sigma=True)
    assert R.rel(no_sigma, torch.autograd.grad(y2, leaves[0], gy)[0]) < 1e-12
    if shape[2] * shape[3] > 1:
        assert R.rel(no_sigma, gx) > 1e-4


def test_the_sigma_path_case_of_the_gpu_suite_separates_the_two_gradients():
    """tests/test_gpu_pointmlp.py's sigma-path case: its two float64 reference gradients differ by more than 1e-2."""
    import test_gpu_pointmlp as G
    pts, idx, fps, alpha, beta, w, gy = G.sigma_case()
    _, saved = R.hoisted_forward(pts.double(), idx, fps, alpha.double(), beta.double(), w.double())
    full = R.hoisted_backward(gy.double(), pts.double(), idx, fps, saved)['dx']
    detached = R.hoisted_backward(gy.double(), pts.double(), idx, fps, saved, sigma_path=False)['dx']
    assert R.rel(detached, full) > 1e-2


def test_covers_on_plain_values():
    from adaptpoint_amd.affine_group import covers
    B, N = 32, 1024
    for C0, O_of in ((64, lambda c, i: 2 * c), (32, lambda c, i: 2 * c if i < 3 else c), (16, lambda c, i: 2 * c)):
        c, n = C0, N
        for i in range(4):
            o = O_of(c, i)
            for K in (8, 24):
                assert covers(B, n, n // 2, K, c, o), (c, o, n)
            c, n = o, n // 2
    assert covers(4, 64, 32, 8, 16, 32) and covers(1, 8, 1, 1, 16, 32) and covers(2, 70, 33, 64, 64, 128)
    ok = dict(B=32, N=1024, S=512, K=24, C=64, O=128)
    assert covers(**ok)
    assert not covers(**{**ok, 'K': 65}) and not covers(**{**ok, 'K': 0}) and not covers(**{**ok, 'N': 16, 'S': 8})
    assert not covers(**ok, groups=2) and not covers(**ok, bias=True) and not covers(**ok, use_xyz=True)
    assert not covers(**ok, normalize="center") and not covers(**ok, normalize=None) and not covers(**ok, activation="gelu")
    assert not covers(**{**ok, 'B': 65536, 'N': 64, 'S': 32}) and not covers(**{**ok, 'B': 1 << 12, 'N': 1 << 12})
    assert not covers(1, 1, 1, 1, 1, 4) and not covers(**{**ok, 'B': 0})           # S K C >= 2


def test_uncovered_configurations_run_composed(cpu_mirrors):
    """normalize in {center, anchor, None}, use_xyz, groups > 1, bias=True and the other activations all build and run
    (composed) with the reference's parameter names."""
    from adaptpoint_amd.pointmlp import PointMLP
    pos, x, _ = R.classifier_inputs(2, 32, 0)
    for over in (dict(normalize="center"), dict(normalize=None), dict(use_xyz=True), dict(groups=2), dict(bias=True),
                 dict(activation="gelu"), dict(activation="leakyrelu"), dict(pre_blocks=[0, 1], pos_blocks=[1, 0])):
        args = dict(in_channels=4, embed_dim=8, dim_expansion=[2, 2], pre_blocks=[1, 1], pos_blocks=[1, 1],
                    k_neighbors=[4, 4], reducers=[2, 2], fused=True)
        args.update(over)
        m = PointMLP(**args).eval()
        with torch.no_grad():
            out = m({'pos': pos, 'x': x})
        assert out.shape == (2, 15) and torch.isfinite(out).all(), over
        assert ("local_grouper_list.0.affine_alpha" in m.state_dict()) == (args.get('normalize', 'anchor') is not None)


def test_fused_model_on_cpu_tensors_runs_composed_without_a_fallback_entry(gold, cpu_mirrors):
    from adaptpoint_amd import set_abstraction as SA
    before = dict(SA.FUSED_FALLBACKS)
    m = _narrow(fused=True).eval()
    pos, x, _ = R.classifier_inputs(R.NARROW_B, R.NARROW_N, int(gold["a/seed"]))
    with torch.no_grad():
        logits = m({'pos': pos, 'x': x})
    np.testing.assert_allclose(logits.numpy(), gold["b/logits"], rtol=1e-5)
    assert SA.FUSED_FALLBACKS == before


def test_a_graph_without_reverse_lists_has_its_own_fallback_reason(cpu_mirrors):
    """A GroupIndex built from CPU tensors carries no lists: the fused stage names that, not the configuration."""
    m = _narrow(fused=True)
    pos, x, _ = R.classifier_inputs(R.NARROW_B, R.NARROW_N, 0)
    graphs = m.encoder.index(pos)
    reason = m.encoder._uncovered(0, torch.zeros(R.NARROW_B, 16, R.NARROW_N), graphs[0])
    assert reason is not None and "no reverse lists" in reason and "no fused kernel" not in reason


def test_cpu_tensors_are_refused_by_the_operators():
    from adaptpoint_amd import affine_group as AG
    g = AG.group_index(torch.zeros(1, 2, dtype=torch.int32), torch.zeros(1, 2, 3), torch.zeros(1, 2, 2, dtype=torch.int32), 4)
    with pytest.raises(RuntimeError, match="CUDA/HIP"):
        AG.affine_group_linear(torch.zeros(1, 4, 2), g, torch.ones(2), torch.zeros(2), torch.zeros(3, 4, 1))
    with pytest.raises(RuntimeError, match="CUDA/HIP"):
        AG.res_relu_max(torch.zeros(1, 2, 4), torch.zeros(1, 2, 4), 2)


def test_argument_validation_of_the_new_entries_needs_no_gpu():
    """Every apn_ag_* entry rejects null pointers, K = 0, K > 64, K > N and B N >= 2^24 before any HIP call, and accepts
    empty work (P: a non-null, aligned address that is never read)."""
    from adaptpoint_amd import _lib
    lib = _lib.load()
    EINVAL, P = -1, 4096

    def mom(b=2, n=16, s=8, k=4, o=8, x=P, idx=P, fps_idx=P, part=P):
        return lib.apn_ag_moments(b, n, s, k, o, x, idx, fps_idx, part, None)

    def fwd(b=2, n=16, s=8, k=4, o=8, pq=P, idx=P, fps_idx=P, r=P, c0=P, y=P, part=P, training=1, rm=None, rv=None, out=None):
        return lib.apn_ag_combine_fwd(b, n, s, k, o, pq, idx, fps_idx, r, c0, y, part, training, None, None, rm, rv, 1e-5, 1,
                                      None, out, None)

    def bwd(b=2, n=16, s=8, k=4, o=8, gyt=P, r=P, pq=P, ci=P, li=P, ca=P, la=P, dpq=P, part_dr=P, part_c0=P):
        return lib.apn_ag_combine_bwd(b, n, s, k, o, gyt, r, pq, ci, li, ca, la, dpq, part_dr, part_c0, None)

    def sig(b=2, n=16, s=8, k=4, o=8, x=P, idx=P, fps_idx=P, kappa=P, mu=P, ci=P, li=P, ca=P, la=P, dx=P):
        return lib.apn_ag_sigma_bwd(b, n, s, k, o, x, idx, fps_idx, kappa, mu, ci, li, ca, la, dx, None)

    def pool(b=2, o=8, s=8, k=4, z=P, h=P, out=P, sel=P):
        return lib.apn_ag_res_relu_max(b, o, s, k, z, h, out, sel, None)

    def pool_grad(b=2, o=8, s=8, k=4, g=P, out=P, sel=P, gz=P):
        return lib.apn_ag_res_relu_max_grad(b, o, s, k, g, out, sel, gz, None, None)

    def fold(rows=4, ncol=8, part=P, out=P):
        return lib.apn_ag_fold(rows, ncol, part, out, None)

    pointers = {mom: ["x", "idx", "fps_idx", "part"], fwd: ["pq", "idx", "fps_idx", "r", "c0", "y", "part"],
                bwd: ["gyt", "r", "pq", "ci", "li", "ca", "la", "dpq", "part_dr", "part_c0"],
                sig: ["x", "idx", "fps_idx", "kappa", "mu", "ci", "li", "ca", "la", "dx"],
                pool: ["z", "h", "out", "sel"], pool_grad: ["g", "out", "sel", "gz"], fold: ["part", "out"]}
    for entry, names in pointers.items():
        for name in names:
            assert entry(**{name: None}) == EINVAL, (entry.__name__, name)
    for entry in (mom, fwd, bwd, sig, pool, pool_grad):
        assert entry(b=0) == 0, entry.__name__                                                  # empty work
        assert entry(k=0) == EINVAL and entry(k=65) == EINVAL and entry(b=-1) == EINVAL, entry.__name__
        assert entry(b=65536) == EINVAL and entry(s=-1) == EINVAL, entry.__name__
    for entry in (mom, fwd, bwd, sig):
        assert entry(n=3) == EINVAL and entry(n=64, k=65) == EINVAL, entry.__name__             # K > N, K > 64
        assert entry(b=1 << 12, n=1 << 12) == EINVAL and entry(n=-1) == EINVAL, entry.__name__  # B N >= 2^24
        assert entry(o=-1) == EINVAL, entry.__name__
    assert mom(s=0) == 0 and fwd(s=0) == 0 and mom(o=0) == 0 and fwd(o=0) == 0 and pool(s=0) == 0 and pool_grad(o=0) == 0
    assert fwd(training=0) == EINVAL and fwd(training=0, rm=P, rv=P) == EINVAL                  # eval mode needs out
    assert fold(ncol=0) == 0 and fold(rows=-1) == EINVAL and fold(ncol=-1) == EINVAL
    assert lib.apn_ag_moment_rows(0) == 0 and lib.apn_ag_moment_rows(5) == 2 and lib.apn_ag_moment_rows(4096) == 64
    assert lib.apn_ag_point_rows(0) == 0 and lib.apn_ag_point_rows(17) == 2


def test_library_exports_every_declared_affine_group_symbol():
    import re
    from adaptpoint_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "adaptpoint_amd.h")).read()
    names = sorted(set(re.findall(r"\b(apn_ag_\w+)\s*\(", header)))
    assert len(names) == 9, names
    for name in names:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
