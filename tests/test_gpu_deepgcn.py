"""GPU suite: the DeepGCN classifier (adaptpoint_amd/deepgcn.py) with its blocks on csrc/edge_conv.hip (ReLU, the residual
in the output kernel) and its dilated, stochastic graphs from csrc/knn.hip, against the float64 restatement
(tests/deepgcn_reference.py) with the composed fp32 model measured beside it -- the bar of tests/test_gpu_edge_conv.py:
per tensor at most 4 x the composed model's relative L2 distance to float64, floor 2e-6 -- and inside the training and
evaluation steps it has to drop into.

The model: the default model's widths at small depth -- channels 64, emb_dims 256, n_blocks 6 (dilations 1..5, so the
widest graph searches 80 neighbours), k = 16, epsilon 0.2 under a fixed torch.manual_seed, B = 4, N = 256, dropout 0.
The fused model runs once and keeps its six graphs; the composed model and the restatement run on those same graphs
(a neighbour that rounding swaps is a different function, not an arithmetic error)."""
import gc

import pytest
import torch

import deepgcn_reference as R

pytestmark = pytest.mark.gpu
B, N = 4, 256
MODEL = dict(channels=64, emb_dims=256, n_blocks=6, k=16, epsilon=0.2)
SEED = 0          # torch.manual_seed before a forward: with it the six draws take both branches (asserted below)


def _model(dev, fused, **over):
    from adaptpoint_amd.deepgcn import DeepGcnClassifier
    from adaptpoint_amd.pointnext import fill_parameters_by_name
    return R.no_dropout(fill_parameters_by_name(DeepGcnClassifier(fused=fused, **dict(MODEL, **over)))).to(dev)


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


def _tables(model):
    return [m.slots.tolist() for m in model.encoder.graph_modules()]


def _strided(model):
    return [list(range(0, m.k * m.dilation, m.dilation)) for m in model.encoder.graph_modules()]


@pytest.fixture(scope="module")
def step(dev):
    """One training step at B = 4, N = 256, dropout 0: fused (keeping its graphs), composed and float64 on the same
    graphs.  Of 8 seeded inputs, the one with the largest float64 decision margin on the fused model's graphs."""
    from adaptpoint_amd import set_abstraction as SA
    before = dict(SA.FUSED_FALLBACKS)
    best = None
    for seed in range(8):
        pos, x, gt = (t.to(dev) for t in R.classifier_inputs(B, N, seed))
        fused = _model(dev, True).train()
        torch.manual_seed(SEED)
        res = _train_step(fused, pos, x, gt, keep_graphs=True)
        graphs = fused.encoder.last_graphs
        ref = R.run_deepgcn64(_model(dev, False).train(), pos, x, graphs, gt)
        if best is None or ref['margin'] > best['ref']['margin']:
            best = dict(seed=seed, pos=pos, x=x, gt=gt, fused=res, graphs=graphs, ref=ref, tables=_tables(fused))
    assert SA.FUSED_FALLBACKS == before, "a fused block fell back"
    print(f"input seed {best['seed']} of 8, decision margin {best['ref']['margin']:.1e}; slot tables {best['tables']}")
    best['composed'] = _train_step(_model(dev, False).train(), best['pos'], best['x'], best['gt'], graphs=best['graphs'])
    return best


def test_classifier_against_float64(dev, step):
    assert step['fused']['logits'].shape == (B, 15) and len(step['graphs']) == 6
    strided = _strided(_model(dev, False))
    hit = [t != s for t, s in zip(step['tables'], strided)]
    assert any(hit[1:]) and not all(hit), hit                        # both the random and the strided branch were taken
    assert sorted(step['fused']['grads']) == sorted(step['ref']['grads']) == sorted(step['composed']['grads'])
    _within(_errors(step['fused'], step['ref']), _errors(step['composed'], step['ref']), "DeepGcnClassifier, training mode")


def test_no_systematic_error_along_the_true_gradient(step):
    """The projection check of tests/test_gpu_pointnext.py: <g - g_ref, g_ref> / |g_ref|^2 <= 1e-3 on every tensor of
    8192 entries or more -- a backward kernel that drops or mis-scales a term (the residual's g, say) fails here."""
    proj = lambda a, b: float(((a.double() - b) * b).sum() / (b * b).sum().clamp_min(1e-300))
    rows = {n: (proj(step['fused']['grads'][n], g), proj(step['composed']['grads'][n], g))
            for n, g in step['ref']['grads'].items() if g.numel() >= 8192}
    print("projection on the float64 gradient (fused, composed):", {k: "%.1e / %.1e" % v for k, v in rows.items()})
    assert len(rows) >= 6
    assert all(abs(v[0]) <= 1e-3 for v in rows.values()), {k: v for k, v in rows.items() if abs(v[0]) > 1e-3}


def test_the_dynamic_graphs_are_the_kernels(dev, step):
    """Each kept graph equals knn_dilated of that layer's recorded input with that module's slot table, bit for bit."""
    from adaptpoint_amd.layers import knn_dilated
    fused = _model(dev, True).train()
    inputs = []
    hooks = [blk.register_forward_pre_hook(lambda m, args: inputs.append(args[0].detach().squeeze(-1).transpose(1, 2).contiguous()))
             for blk in fused.encoder.backbone]
    torch.manual_seed(SEED)
    with torch.no_grad():
        fused({'pos': step['pos'], 'x': step['x']}, keep_graphs=True)
    for h in hooks:
        h.remove()
    graphs = fused.encoder.last_graphs
    mods = fused.encoder.graph_modules()
    assert len(inputs) == 5 and len(graphs) == 6 and _tables(fused) == step['tables']
    for g, rows, m in zip(graphs, [step['pos']] + inputs, mods):
        assert g.dtype == torch.int32 and g.shape == (B, N, 16)
        assert torch.equal(g, knn_dilated(rows, rows, 16, m.dilation, slots=m.slots))
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
    torch.manual_seed(SEED)
    logits, loss = ClassifierStep(fused)(points, gt)
    graphs = fused.encoder.last_graphs
    assert torch.isfinite(logits).all() and torch.isfinite(loss) and SA.FUSED_FALLBACKS == before
    assert all(torch.isfinite(q).all() for q in fused.parameters())
    assert any(not torch.equal(q, weights[n]) for n, q in fused.named_parameters())       # the optimizer stepped
    composed = _train_step(_model(dev, False).train(), pos, x, gt, graphs=graphs)
    ref = R.run_deepgcn64(_model(dev, False).train(), pos, x, graphs, gt)
    err = lambda r: {'logits': R.rel(r['logits'], ref['logits']), 'loss': R.rel(r['loss'], ref['loss'])}
    _within(err({'logits': logits, 'loss': loss}), err(composed), "ClassifierStep")


def test_plugs_into_the_evaluator(dev):
    """One `Evaluator` batch with the fused model: finite counts, and the predictions of the composed model on the same
    input and graphs wherever its two best logits are farther apart than rounding can move them."""
    import numpy as np
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
    assert _tables(fused) == _strided(fused)                         # eval mode: every graph strided
    with torch.no_grad():
        logits = _model(dev, False).eval()(seen[0], graphs=fused.encoder.last_graphs)
    top = logits.topk(2, dim=1).values
    clear = (top[:, 0] - top[:, 1]) > 1e-4 * logits.abs().max()
    assert clear.sum() >= S - 1
    pred = ev.pred.reshape(-1)[:S].long()
    assert torch.equal(pred[clear], logits.argmax(1)[clear])


def test_captured_step_follows_redraw_between_replays(dev, step):
    """Forward + backward captured once; under capture nothing is drawn or copied, `redraw()` between replays makes the
    draws: each replay equals the eager step made under the same torch seed, bit for bit; no memset node."""
    from adaptpoint_amd import graphs
    pos, x, gt = step['pos'], step['x'], step['gt']
    model = _model(dev, True).train()
    params = list(model.parameters())
    data = {'pos': pos, 'x': x}

    def run():
        logits, loss = model.get_logits_loss(data, gt)
        return [logits.detach(), loss.detach()] + list(torch.autograd.grad(loss, params))
    # two torch seeds whose draws differ, the second with a random table
    seeds, seen = [], []
    for s in range(40):
        torch.manual_seed(s)
        model.redraw()
        t = _tables(model)
        if (not seeds and t == _strided(model)) or (len(seeds) == 1 and t != _strided(model)):
            seeds.append(s)
            seen.append(t)
        if len(seeds) == 2:
            break
    assert len(seeds) == 2 and seen[0] != seen[1]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                       # warm-up: allocator pools, lazy initialisation
        for _ in range(2):
            run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    eager = {}
    for s in seeds:
        torch.manual_seed(s)
        eager[s] = [t.clone() for t in run()]
    assert not torch.equal(eager[seeds[0]][0], eager[seeds[1]][0])
    counter = model.encoder.head.gconv.nn[1].num_batches_tracked
    torch.cuda.synchronize()
    gc.collect()
    torch.manual_seed(99)
    state = torch.get_rng_state()
    tables = _tables(model)
    graph, captured, census = graphs.capture(run, leaves=params, what="the DeepGCN step's graph")
    print("DeepGCN step graph:", census)
    assert not census.get("memset", 0)
    assert torch.equal(torch.get_rng_state(), state) and _tables(model) == tables       # nothing drawn, nothing copied
    n0 = int(counter)
    for s in (seeds[0], seeds[1], seeds[0]):
        torch.manual_seed(s)
        model.redraw()
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(eager[s], captured):
            assert torch.equal(a, b), s
    assert int(counter) == n0 + 3


def test_widest_graph_block(dev):
    """`DynConv` at d = 13, k = 16: the default model's widest graph (208 neighbours searched) at N = 256, fused against
    float64 with the composed block beside it, on the graph the fused block made."""
    from adaptpoint_amd import set_abstraction as SA
    from adaptpoint_amd.deepgcn import DynConv
    from adaptpoint_amd.layers import knn_dilated
    from adaptpoint_amd.pointnext import fill_parameters_by_name
    before = dict(SA.FUSED_FALLBACKS)

    def blk(fused):
        return fill_parameters_by_name(DynConv(64, 64, 'edge', 16, 13, norm_args={'norm': 'bn'}, act_args={'act': 'relu'},
                                               fused=fused)).to(dev).train()
    x, w = (t.to(dev) for t in R.block_inputs(2, 256, 64, 64, 5))
    res = {}
    xin = x.clone().requires_grad_(True)
    f = blk(True)
    out = f(xin.unsqueeze(-1)).squeeze(-1)
    (out * w).sum().backward()
    idx = f.last_graph
    rows = x.transpose(1, 2).contiguous()
    assert idx.shape == (2, 256, 16) and torch.equal(idx, knn_dilated(rows, rows, 16, 13))
    assert torch.equal(idx[:, :, 0].long(), torch.arange(256, device=dev).expand(2, -1))
    res[True] = {'out': out.detach(), 'dx': xin.grad, 'grads': {n: q.grad for n, q in f.named_parameters()}}
    c = blk(False)
    xc = x.clone().requires_grad_(True)
    oc = c(xc.unsqueeze(-1), idx).squeeze(-1)
    (oc * w).sum().backward()
    res[False] = {'out': oc.detach(), 'dx': xc.grad, 'grads': {n: q.grad for n, q in c.named_parameters()}}
    ref = R.run_res64(blk(False), x, idx, w)
    errs = {k: {'out': R.rel(r['out'], ref['out']), 'dx': R.rel(r['dx'], ref['dx']),
                **{'grad/' + n: R.rel(r['grads'][n], g) for n, g in ref['grads'].items()}} for k, r in res.items()}
    _within(errs[True], errs[False], "DynConv k=16 d=13")
    assert SA.FUSED_FALLBACKS == before


def test_more_than_256_searched_neighbours_take_the_composed_lines_with_a_recorded_fallback(dev):
    from adaptpoint_amd import set_abstraction as SA
    from adaptpoint_amd.deepgcn import DilatedKNN
    x = R.block_inputs(2, 300, 8, 8, 6)[0].transpose(1, 2).contiguous().to(dev)          # (2, 300, 8)
    before = sum(SA.FUSED_FALLBACKS.values())
    idx = DilatedKNN(20, 13).to(dev)(x)                                                    # 260 neighbours searched
    assert sum(SA.FUSED_FALLBACKS.values()) == before + 1
    assert any("DilatedKNN" in k and "d=13" in k for k in SA.FUSED_FALLBACKS)
    want = torch.cdist(x, x).topk(k=260, dim=-1, largest=False, sorted=True).indices[..., ::13].int()
    assert idx.dtype == torch.int32 and idx.is_contiguous() and torch.equal(idx, want)
    assert sum(SA.FUSED_FALLBACKS.values()) == before + 1
    DilatedKNN(16, 13).to(dev)(x)                                                          # 208: the kernel, no entry
    assert sum(SA.FUSED_FALLBACKS.values()) == before + 1
