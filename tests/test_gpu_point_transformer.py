"""GPU suite of the Point Transformer model (adaptpoint_amd/point_transformer.py): PTSeg(width 32, two blocks per stage)
on three clouds of 1100, 700 and 1300 points -- fused, composed and float64 (tests/point_transformer_reference.py) on
the fused model's kept graphs and sampled indices, the bar of tests/test_gpu_dgcnn.py (fused distance to float64 at
most max(4 x the composed path's, 2e-6) per tensor) --, the kNN launch count, and the reference's narrow model of
tests/golden/point_transformer_golden.npz on the GPU's composed path."""
import os

import numpy as np
import pytest
import torch

import point_transformer_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1100, 700, 1300)
CFG = dict(width=32, blocks=[2, 2, 2, 2, 2])
ATOL = 16 * 2.0 ** -22         # the golden comparison's absolute term: 16 ulps of a logit of 2 .. 4


def _model(dev, fused, **cfg):
    from adaptpoint_amd.point_transformer import PTSeg
    from adaptpoint_amd.pointnext import fill_parameters_by_name
    return fill_parameters_by_name(PTSeg('PointTransformerBlock', fused=fused, **(cfg or CFG))).to(dev)


def _train_step(model, p, x, o, w, **kw):
    model.zero_grad(set_to_none=True)
    logits = model(p, x, o, **kw)
    (logits * w).sum().backward()
    return {'logits': logits.detach(), 'grads': {n: q.grad for n, q in model.named_parameters()}}


def _errors(res, ref):
    errs = {'logits': R.rel(res['logits'], ref['logits'])}
    for n, g in ref['grads'].items():
        errs['grad/' + n] = R.rel(res['grads'][n], g)
    return errs


def _within(fused, composed, what):
    rows = {k: (fused[k], composed[k]) for k in composed}
    worst = sorted(rows.items(), key=lambda kv: -kv[1][0])[:8]
    print(what, "(fused, composed) distance to float64, the 8 largest:", {k: "%.1e / %.1e" % v for k, v in worst})
    bad = {k: v for k, v in rows.items() if not v[0] <= max(4.0 * v[1], 2e-6)}
    assert not bad, (what, bad)


@pytest.fixture(scope="module")
def step(dev):
    """One training step: fused (keeping its graphs), composed and float64 on the same graphs.  Of 8 seeded inputs, the
    one with the largest float64 decision margin on the fused model's graphs."""
    from adaptpoint_amd import point_transformer as PT, set_abstraction as SA
    before = dict(SA.FUSED_FALLBACKS)
    best = None
    for seed in range(8):
        p, x, o, w = (t.to(dev) for t in R.model_inputs(SIZES, seed))
        fused = _model(dev, True).train()
        calls = []
        PT.knn_hook = lambda who, k, n, m: calls.append(who)
        try:
            res = _train_step(fused, p, x, o, w, keep_graphs=True)
        finally:
            PT.knn_hook = None
        graphs = fused.last_graphs
        ref = R.run_model64(_model(dev, False), p, x, o, graphs, w)
        if best is None or ref['margin'] > best['ref']['margin']:
            best = dict(seed=seed, p=p, x=x, o=o, w=w, fused=res, graphs=graphs, ref=ref, calls=calls)
    assert SA.FUSED_FALLBACKS == before, "a fused layer fell back"
    print(f"input seed {best['seed']} of 8, decision margin {best['ref']['margin']:.1e}")
    best['composed'] = _train_step(_model(dev, False).train(), best['p'], best['x'], best['o'], best['w'],
                                   graphs=best['graphs'])
    return best


def test_training_step_against_float64(step):
    n = sum(SIZES)
    assert step['fused']['logits'].shape == (n, 13)
    rows, sizes = [], SIZES
    for _ in range(5):                                           # every cloud keeps a quarter of its points per level
        rows.append(sum(sizes))
        sizes = [s // 4 for s in sizes]
    assert rows == [3100, 775, 192, 47, 11]                      # the deepest clouds hold 4, 2 and 5 points: fewer than k
    assert [tuple(g.shape) for g in step['graphs']['stage']] == list(zip(rows, [8, 16, 16, 16, 16]))
    assert sorted(step['fused']['grads']) == sorted(step['ref']['grads']) == sorted(step['composed']['grads'])
    _within(_errors(step['fused'], step['ref']), _errors(step['composed'], step['ref']), "PTSeg, training mode")


def test_five_knn_queries_serve_the_eighteen_layer_calls(step):
    """Through the module's call hook: one query per level for the layers (the reference issues two per layer), one per
    strided TransitionDown; with keep_graphs one more per TransitionUp to record what the interpolation kernel used."""
    assert step['calls'].count('stage') == 5 and step['calls'].count('down') == 4


def test_eval_logits_against_float64(dev, step):
    p, x, o = step['p'], step['x'], step['o']
    with torch.no_grad():
        fused = _model(dev, True).eval()(p, x, o, graphs=step['graphs'])
        comp = _model(dev, False).eval()(p, x, o, graphs=step['graphs'])
    ref = R.run_model64(_model(dev, False), p, x, o, step['graphs'], training=False)['logits']
    _within({'logits': R.rel(fused, ref)}, {'logits': R.rel(comp, ref)}, "PTSeg, eval mode")


def test_graphs_are_the_kernels(dev, step):
    """The kept stage graphs equal the kNN kernel's answer on the kept levels' points, and a second forward on the
    kept graphs issues no query at all."""
    from adaptpoint_amd import point_transformer as PT, pointops as PO
    p, o = step['p'], step['o']
    idx, _ = PO.knnquery(8, p, p, o, o)
    assert torch.equal(idx, step['graphs']['stage'][0])
    calls = []
    PT.knn_hook = lambda who, k, n, m: calls.append(who)
    try:
        with torch.no_grad():
            _model(dev, True).eval()(p, step['x'], o, graphs=step['graphs'])
    finally:
        PT.knn_hook = None
    assert calls == []


def test_the_goldens_narrow_model_on_the_composed_gpu_path(dev):
    """The reference's PTSeg (width 8) as the fixture recorded it on CPU statements: the GPU operators choose the same
    indices at every level and the composed path reproduces the logits."""
    gold = np.load(os.path.join(ROOT, "tests", "golden", "point_transformer_golden.npz"))
    p, x, o, _ = (t.to(dev) for t in R.model_inputs(R.NARROW_SIZES, int(gold["a/seed"])))
    m = _model(dev, False, **R.NARROW).eval()
    with torch.no_grad():
        logits = m(p, x, o, keep_graphs=True)
    graphs = m.last_graphs
    for lv in range(5):
        assert np.array_equal(graphs['stage'][lv].cpu().numpy(), gold[f"a/graph/stage{lv + 1}"]), lv
    for lv in range(4):
        assert np.array_equal(graphs['down'][lv][0].cpu().numpy(), gold[f"a/graph/fps{lv + 2}"]), lv
        assert np.array_equal(graphs['down'][lv][1].cpu().numpy(), gold[f"a/graph/down{lv + 2}"]), lv
        assert np.array_equal(graphs['up'][lv].cpu().numpy(), gold[f"a/graph/up{lv + 1}"]), lv
    # elementwise rtol 1e-5, with an absolute term of 16 ulps of the logit scale (2.5: 16 x 2^-22 = 3.8e-6).  Without one
    # the check asks the impossible of the logits near zero: the smallest of the 14 001 is 6.6e-5, where rtol 1e-5 is 7e-10,
    # far below one fp32 rounding of the last Linear's sum at this scale -- the CPU mirror itself (relative L2 2.5e-7,
    # largest difference 1.9e-6) misses it on 186 elements.  16 ulps still catches a single wrong logit
    got, want = logits.cpu().numpy(), gold["b/logits"]
    diff = np.abs(got - want)
    print("eval logits: relative L2 %.1e, largest absolute difference %.1e, largest share of the elementwise bound %.2f"
          % (R.rel(got, want), diff.max(), (diff / (ATOL + 1e-5 * np.abs(want))).max()))
    assert 2.0 < np.abs(want).max() < 4.0                        # the scale ATOL is stated for
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=ATOL)
    assert R.rel(got, want) <= 1e-5
