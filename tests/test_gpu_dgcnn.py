"""GPU suite: the DGCNN classifier (adaptpoint_amd/dgcnn.py) with its EdgeConv blocks on csrc/edge_conv.hip and its
graphs from csrc/knn.hip, against the float64 restatement (tests/dgcnn_reference.py) with the composed fp32 model
measured beside it -- the bar of tests/test_gpu_edge_conv.py: per tensor at most 4 x the composed model's relative L2
distance to float64, floor 2e-6 -- and inside the training and evaluation steps it has to drop into.

The fused model runs once and keeps its four graphs; the composed model and the restatement run on those same graphs
(a neighbour that rounding swaps is a different function, not an arithmetic error)."""
import numpy as np
import pytest
import torch

import dgcnn_reference as R

pytestmark = pytest.mark.gpu
B, N = 4, 256


def _model(dev, fused, **over):
    from adaptpoint_amd.dgcnn import DgcnnClassifier
    from adaptpoint_amd.pointnext import fill_parameters_by_name
    return R.no_dropout(fill_parameters_by_name(DgcnnClassifier(fused=fused, **over))).to(dev)


def _within(fused, composed, what):
    rows = {k: (fused[k], composed[k]) for k in composed}
    print(what, "(fused, composed) distance to float64:", {k: "%.1e / %.1e" % v for k, v in rows.items()})
    bad = {k: v for k, v in rows.items() if not v[0] <= max(4.0 * v[1], 2e-6)}
    assert not bad, (what, bad)


def _train_step(model, pos, x, gt, **kw):
    model.zero_grad(set_to_none=True)
    logits, loss = model.get_logits_loss({'pos': pos, 'x': x}, gt, **kw)
    loss.backward()
    return {'logits': logits.detach(), 'loss': loss.detach(),
            'grads': {n: q.grad for n, q in model.named_parameters() if q.grad is not None}}


def _errors(res, ref):
    errs = {'logits': R.rel(res['logits'], ref['logits']), 'loss': R.rel(res['loss'], ref['loss'])}
    for n, g in ref['grads'].items():
        errs['grad/' + n] = R.rel(res['grads'][n], g)
    return errs


@pytest.fixture(scope="module")
def step(dev):
    """One training step of the default classifier at B = 4, N = 256, dropout 0: fused (keeping its graphs), composed
    and float64 on the same graphs.  Of 8 seeded inputs, the one with the largest float64 decision margin on the fused
    model's graphs."""
    from adaptpoint_amd import set_abstraction as SA
    before = dict(SA.FUSED_FALLBACKS)
    best = None
    for seed in range(8):
        pos, x, gt = (t.to(dev) for t in R.classifier_inputs(B, N, seed))
        fused = _model(dev, True).train()
        res = _train_step(fused, pos, x, gt, keep_graphs=True)
        graphs = fused.encoder.last_graphs
        ref = R.run_classifier64(_model(dev, False).train(), pos, x, graphs, gt)
        if best is None or ref['margin'] > best['ref']['margin']:
            best = dict(seed=seed, pos=pos, x=x, gt=gt, fused=res, graphs=graphs, ref=ref)
    assert SA.FUSED_FALLBACKS == before, "a fused EdgeConv block fell back"
    print(f"input seed {best['seed']} of 8, decision margin {best['ref']['margin']:.1e}")
    best['composed'] = _train_step(_model(dev, False).train(), best['pos'], best['x'], best['gt'], graphs=best['graphs'])
    return best


def test_classifier_against_float64(step):
    assert step['fused']['logits'].shape == (B, 15) and len(step['graphs']) == 4
    assert sorted(step['fused']['grads']) == sorted(step['ref']['grads']) == sorted(step['composed']['grads'])
    _within(_errors(step['fused'], step['ref']), _errors(step['composed'], step['ref']), "DgcnnClassifier, training mode")


def test_no_systematic_error_along_the_true_gradient(step):
    """The projection check of tests/test_gpu_pointnext.py: <g - g_ref, g_ref> / |g_ref|^2 <= 1e-3 on every tensor of
    8192 entries or more -- a backward kernel that drops or mis-scales a term fails here."""
    proj = lambda a, b: float(((a.double() - b) * b).sum() / (b * b).sum().clamp_min(1e-300))
    rows = {n: (proj(step['fused']['grads'][n], g), proj(step['composed']['grads'][n], g))
            for n, g in step['ref']['grads'].items() if g.numel() >= 8192}
    print("projection on the float64 gradient (fused, composed):", {k: "%.1e / %.1e" % v for k, v in rows.items()})
    assert len(rows) >= 6
    assert all(abs(v[0]) <= 1e-3 for v in rows.values()), {k: v for k, v in rows.items() if abs(v[0]) > 1e-3}


def test_the_dynamic_graph_is_the_kernels(dev, step):
    """Each kept graph equals knn_query of that layer's recorded input, bit for bit."""
    from adaptpoint_amd.layers import knn_query
    fused = _model(dev, True).train()
    inputs = []
    hooks = [blk.register_forward_pre_hook(lambda m, args: inputs.append(args[0].detach().squeeze(-1).transpose(1, 2).contiguous()))
             for blk in fused.encoder.backbone]
    with torch.no_grad():
        fused({'pos': step['pos'], 'x': step['x']}, keep_graphs=True)
    for h in hooks:
        h.remove()
    graphs = fused.encoder.last_graphs
    assert len(inputs) == 3 and len(graphs) == 4
    assert torch.equal(graphs[0], knn_query(step['pos'], step['pos'], 20))
    for g, rows in zip(graphs[1:], inputs):
        assert g.dtype == torch.int32 and g.shape == (B, N, 20)
        assert torch.equal(g, knn_query(rows, rows, 20))
    for g, kept in zip(graphs, step['graphs']):                     # and the training step above used the same ones
        assert torch.equal(g, kept)


def test_plugs_into_the_classifier_step(dev, step):
    """One `ClassifierStep` iteration with the fused model: finite, and its loss and logits agree with the composed
    model on the graphs it used within the bar above (both measured against float64)."""
    from adaptpoint_amd import set_abstraction as SA
    from adaptpoint_amd.gan import ClassifierStep
    before = dict(SA.FUSED_FALLBACKS)
    pos, x, gt = step['pos'], step['x'], step['gt']
    points = x.transpose(1, 2).contiguous()                          # (B, N, 4): N <= npoints, nothing is resampled
    fused = _model(dev, True)
    fused.encoder.keep_graphs = True
    weights = {n: q.detach().clone() for n, q in fused.named_parameters()}
    logits, loss = ClassifierStep(fused)(points, gt)
    graphs = fused.encoder.last_graphs
    assert torch.isfinite(logits).all() and torch.isfinite(loss) and SA.FUSED_FALLBACKS == before
    assert all(torch.isfinite(q).all() for q in fused.parameters())
    assert any(not torch.equal(q, weights[n]) for n, q in fused.named_parameters())       # the optimizer stepped
    composed = _train_step(_model(dev, False).train(), pos, x, gt, graphs=graphs)
    ref = R.run_classifier64(_model(dev, False).train(), pos, x, graphs, gt)
    err = lambda r: {'logits': R.rel(r['logits'], ref['logits']), 'loss': R.rel(r['loss'], ref['loss'])}
    _within(err({'logits': logits, 'loss': loss}), err(composed), "ClassifierStep")


def test_plugs_into_the_evaluator(dev, step):
    """One `Evaluator` batch with the fused model: finite counts, and the predictions of the composed model on the same
    input and graphs wherever its two best logits are farther apart than rounding can move them."""
    from adaptpoint_amd import evaluate as E
    from adaptpoint_amd.synthetic import unit_sphere_cloud
    from adaptpoint_amd.transforms import CloudTransform
    S = 8
    points = torch.from_numpy(unit_sphere_cloud(S, N, 77)).to(dev)
    labels = torch.randint(0, 15, (S,), generator=torch.Generator().manual_seed(77)).to(dev)
    fused = _model(dev, True)
    fused.encoder.keep_graphs = True
    seen = []
    hook = fused.register_forward_pre_hook(lambda m, args: seen.append(args[0]))
    ev = E.Evaluator(fused, CloudTransform(['PointsToTensor', 'PointCloudCenterAndNormalize'], 'val', gravity_dim=1),
                     batch_size=S, num_points=N, capture=False, keep_pred=True)
    macc, oa, accs, cm = ev.validate(points, labels)
    hook.remove()
    assert np.isfinite(macc) and np.isfinite(oa) and int(cm.value.sum()) == S and len(seen) == 1
    with torch.no_grad():
        logits = _model(dev, False).eval()(seen[0], graphs=fused.encoder.last_graphs)
    top = logits.topk(2, dim=1).values
    clear = (top[:, 0] - top[:, 1]) > 1e-4 * logits.abs().max()
    assert clear.sum() >= S - 1
    pred = ev.pred.reshape(-1)[:S].long()
    assert torch.equal(pred[clear], logits.argmax(1)[clear])
