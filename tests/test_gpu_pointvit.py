"""PointViT on the GPU (adaptpoint_amd/pointvit.py): the fixture's narrow model (dim 128, depth 2, 2 heads of 64, T = 17) with
`fused=True` (csrc/token_attention.hip) and `fused=False` (the reference's composition) on the SAME index tensors, each
against the float64 restatement of tests/pointvit_reference.py:

    || fused - f64 || <= 4 || composed - f64 || + 2e-6 || f64 ||        logits, loss, every weight gradient

with no call falling back; eval mode and `forward_seg_feat`; `PointVitClassifier` through one `ClassifierStep` iteration
and one `Evaluator` batch; a captured training step replayed twice gives the same bits."""
import gc

import numpy as np
import pytest
import torch

import pointvit_reference as R

pytestmark = pytest.mark.gpu
N = R.NARROW_N


def _model(dev, fused, group='knn'):
    from adaptpoint_amd.pointvit import PointVitClassifier
    from adaptpoint_amd.pointnext import fill_parameters_by_name
    return R.no_dropout(fill_parameters_by_name(PointVitClassifier(fused=fused, **R.narrow(group)))).to(dev)


def _train_step(m, pos, x, gt, index):
    m.zero_grad(set_to_none=True)
    logits, loss = m.get_logits_loss({'pos': pos, 'x': x}, gt, index=index)
    loss.backward()
    return {'logits': logits.detach(), 'loss': loss.detach(), 'grads': {n: q.grad for n, q in m.named_parameters()}}


def _fallbacks():
    from adaptpoint_amd import token_attention as TA
    return dict(TA.COMPOSED_CALLS)


@pytest.fixture(scope="module", params=['knn', 'ballquery'])
def step(request, dev):
    """One training step of the fused and of the composed model on the kernels' own index, and the float64 restatement."""
    group = request.param
    pos, x, gt = (t.to(dev) for t in R.classifier_inputs(R.NARROW_B, N, 3))
    before = _fallbacks()
    fused = _model(dev, True, group).train()
    index = fused.encoder.patch_embed.index(pos)
    res = dict(group=group, pos=pos, x=x, gt=gt, index=index)
    res['fused'] = _train_step(fused, pos, x, gt, index)
    res['fell_back'] = _fallbacks() != before
    res['composed'] = _train_step(_model(dev, False, group).train(), pos, x, gt, index)
    res['ref'] = R.run_classifier64(_model(dev, False, group).train(), pos, x, index, gt)
    return res


def _within(fused_err, composed_err, norm, what):
    assert fused_err <= 4 * composed_err + 2e-6 * norm, (what, fused_err, composed_err, norm)


def test_classifier_against_float64(step):
    ref, fused, comp = step['ref'], step['fused'], step['composed']
    assert not step['fell_back']
    assert step['index'][0].shape == (R.NARROW_B, 16) and step['index'][1].shape == (R.NARROW_B, 16, 8)
    worst = 0.0
    for name in ('logits', 'loss'):
        f, c = (float((r[name].double() - ref[name]).norm()) for r in (fused, comp))
        _within(f, c, float(ref[name].norm()), name)
    for n, g64 in ref['grads'].items():
        f, c = (float((r['grads'][n].double() - g64).norm()) for r in (fused, comp))
        _within(f, c, float(g64.norm()), n)
        worst = max(worst, f / max(c, 1e-300))
    print(f"{step['group']}: worst fused / composed error ratio over the gradients {worst:.2f}; logits fused "
          f"{R.rel(fused['logits'], ref['logits']):.2e} composed {R.rel(comp['logits'], ref['logits']):.2e}")
    assert sorted(ref['grads']) == sorted(fused['grads'])


def test_eval_mode_and_seg_feat(dev, step):
    pos, x, index = step['pos'], step['x'], step['index']
    before = _fallbacks()
    fused, comp = _model(dev, True, step['group']).eval(), _model(dev, False, step['group']).eval()
    with torch.no_grad():
        a, b = fused({'pos': pos, 'x': x}, index=index), comp({'pos': pos, 'x': x}, index=index)
        own = fused({'pos': pos, 'x': x})                                   # its own index: the same kernels, the same bits
        p_list, x_list = fused.encoder.forward_seg_feat(pos, x, index=index)
    ref = R.run_classifier64(comp, pos, x, index, training=False)['logits']
    _within(float((a.double() - ref).norm()), float((b.double() - ref).norm()), float(ref.norm()), "eval logits")
    assert torch.equal(own, a) and _fallbacks() == before
    assert [tuple(t.shape) for t in p_list] == [(R.NARROW_B, N, 3), (R.NARROW_B, 16, 3)]
    assert tuple(x_list[0].shape) == (R.NARROW_B, 4, N) and tuple(x_list[1].shape) == (R.NARROW_B, 128, 17)


def test_two_training_steps_from_the_same_state_are_bit_identical(dev, step):
    again = _train_step(_model(dev, True, step['group']).train(), step['pos'], step['x'], step['gt'], step['index'])
    assert torch.equal(again['logits'], step['fused']['logits'])
    differ = [n for n, g in again['grads'].items() if not torch.equal(g, step['fused']['grads'][n])]
    assert not differ, differ


def test_training_step_captures_and_replays_the_same_bits(dev):
    from adaptpoint_amd import graphs
    before = _fallbacks()
    pos, x, gt = (t.to(dev) for t in R.classifier_inputs(R.NARROW_B, N, 0))
    m = _model(dev, True).train()
    index = m.encoder.patch_embed.index(pos)
    params = [q for q in m.parameters() if q.requires_grad]

    def run():
        logits, loss = m.get_logits_loss({'pos': pos, 'x': x}, gt, index=index)
        grads = torch.autograd.grad(loss, params, allow_unused=True)
        return [logits.detach(), loss.detach()] + [g for g in grads if g is not None]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                       # warm-up: allocator pools, lazy initialisation
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    gc.collect()
    graph, captured, census = graphs.capture(run, leaves=params, what="the PointViT training step")
    print("PointViT step graph:", census)
    assert _fallbacks() == before
    first = None
    for _ in range(2):
        for t in captured:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.isfinite(t).all() for t in captured)
        if first is None:
            first = [t.clone() for t in captured]
        else:
            assert all(torch.equal(a, b) for a, b in zip(first, captured))


def test_plugs_into_the_classifier_step(dev):
    from adaptpoint_amd.gan import ClassifierStep
    before = _fallbacks()
    pos, x, gt = (t.to(dev) for t in R.classifier_inputs(R.NARROW_B, N, 3))
    points = x.transpose(1, 2).contiguous()                          # (B, N, 4): N <= npoints, nothing is resampled
    fused = _model(dev, True)
    weights = {n: q.detach().clone() for n, q in fused.named_parameters()}
    logits, loss = ClassifierStep(fused)(points, gt)
    assert torch.isfinite(logits).all() and torch.isfinite(loss) and _fallbacks() == before
    assert all(torch.isfinite(q).all() for q in fused.parameters())
    assert any(not torch.equal(q, weights[n]) for n, q in fused.named_parameters())       # the optimizer stepped
    comp = _model(dev, False).train()
    index = comp.encoder.patch_embed.index(pos)
    composed = _train_step(comp, pos, x, gt, index)
    ref = R.run_classifier64(_model(dev, False).train(), pos, x, index, gt)
    for name, got in (('logits', logits), ('loss', loss)):
        _within(float((got.double() - ref[name]).norm()), float((composed[name].double() - ref[name]).norm()),
                float(ref[name].norm()), "ClassifierStep " + name)


def test_plugs_into_the_evaluator(dev):
    from adaptpoint_amd import evaluate as E
    from adaptpoint_amd.synthetic import unit_sphere_cloud
    from adaptpoint_amd.transforms import CloudTransform
    S = 8
    points = torch.from_numpy(unit_sphere_cloud(S, N, 77)).to(dev)
    labels = torch.randint(0, 15, (S,), generator=torch.Generator().manual_seed(77)).to(dev)
    before = _fallbacks()
    fused = _model(dev, True)
    seen = []
    hook = fused.register_forward_pre_hook(lambda m, args: seen.append(args[0]))
    ev = E.Evaluator(fused, CloudTransform(['PointsToTensor', 'PointCloudCenterAndNormalize'], 'val', gravity_dim=1),
                     batch_size=S, num_points=N, capture=False, keep_pred=True)
    macc, oa, accs, cm = ev.validate(points, labels)
    hook.remove()
    assert np.isfinite(macc) and np.isfinite(oa) and int(cm.value.sum()) == S and len(seen) == 1 and _fallbacks() == before
    with torch.no_grad():
        logits = _model(dev, False).eval()(seen[0])
    top = logits.topk(2, dim=1).values
    clear = (top[:, 0] - top[:, 1]) > 1e-4 * logits.abs().max()
    assert clear.sum() >= S - 1
    pred = ev.pred.reshape(-1)[:S].long()
    assert torch.equal(pred[clear], logits.argmax(1)[clear])
