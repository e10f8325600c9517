"""GPU suite of the RandLA-Net model (adaptpoint_amd/randla.py) at the golden's configuration
(tests/golden/randla_golden.npz: the REFERENCE's model on the CPU over our kNN stand-in), fused and composed: the graphs
of every level bit for bit, logits and gradients within 8 x the reference's own recorded distance to float64 (err64; the
layer suite's margin, for the same reasons), capture and replay of a training step, the state_dict, the fallback.

MEASURED (MI355X): the worst ratio to err64 over all tensors, per path (documentation; the test asserts the bar)."""
import gc
import os

import numpy as np
import pytest
import torch

import randla_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 8.0
NOISE = 1e-4        # a gradient that is an analytic zero (err64 > 0.5): its norm relative to the layer's weight gradient

# err64 of the logits is 1.7e-6 (median over all tensors 1.2e-6)
MEASURED = dict(fused_worst="1.95 (buf/encoder.1.pool2.mlp.batch_norm.running_var); gradients: 1.71 (fc_end.1.batch_norm.bias)",
                composed_worst="2.0 (grad/fc_end.3.conv.bias; varies run to run with the framework's reductions)",
                eval_logits="fused 1.0e-6, composed 8e-7 against 8 x 1.7e-6",
                step_graph="561 kernel + 56 memcpy nodes, no memset")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "randla_golden.npz"))


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _model(fused, **kw):
    from adaptpoint_amd.pointnext import fill_parameters_by_name
    from adaptpoint_amd.randla import RandLANet
    m = fill_parameters_by_name(RandLANet(device=_dev(), fused=fused, **dict(R.MODEL, **kw)))
    m.fc_end[2].p = 0.0
    return m


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "composed"])
def test_training_step_matches_the_reference(gold, fused):
    from adaptpoint_amd import set_abstraction as SA
    dev = _dev()
    before = dict(SA.FUSED_FALLBACKS)
    m = _model(fused).train()
    x, labels = (t.to(dev) for t in R.model_inputs())
    perm = torch.from_numpy(gold["train/perm"]).to(dev)
    logits = m(x, permutation=perm, keep_graphs=True)
    R.model_loss(logits, labels).backward()
    assert SA.FUSED_FALLBACKS == before, "a fused layer fell back"
    for i, (idx, d2) in enumerate(m.last_graphs['encoder']):
        assert np.array_equal(idx.cpu().numpy(), gold[f"train/graph/encoder{i}"]), i
    for i, idx in enumerate(m.last_graphs['decoder']):
        assert np.array_equal(idx.cpu().numpy(), gold[f"train/graph/decoder{i}"]), i
    ratios = {"logits": R.rel(logits, gold["train/logits"]) / float(gold["train/err64/logits"])}
    params, buffers = dict(m.named_parameters()), dict(m.named_buffers())
    for n, p in params.items():
        g = p.grad.reshape(-1).cpu()[torch.from_numpy(R.sample_index(n, p.numel()))]
        err64 = float(gold["train/err64/grad/" + n])
        if err64 > 0.5:
            assert g.norm().item() <= NOISE * params[n[:-len("bias")] + "weight"].grad.norm().item(), n
        elif n.endswith("score_fn.0.weight"):
            C = p.shape[0] // 2
            ratios["grad/" + n] = R.rel(g, gold["train/grad/" + n]) / err64
            if fused:
                assert not p.grad[:C, C:].any() and not p.grad[C:, :C].any() and not p.grad[C:, C:].any(), n
        else:
            ratios["grad/" + n] = R.rel(g, gold["train/grad/" + n]) / err64
    for n, b in buffers.items():
        if n.endswith("num_batches_tracked"):
            assert int(b) == 1, n
        else:
            ratios["buf/" + n] = R.rel(b, gold["train/buf/" + n]) / max(float(gold["train/err64/buf/" + n]), 1e-7)
    worst = sorted(ratios.items(), key=lambda kv: -kv[1])[:5]
    print("fused" if fused else "composed", "worst ratios to err64:", [(k, "%.2f" % v) for k, v in worst])
    bad = {k: v for k, v in ratios.items() if not v <= MARGIN}
    assert not bad, bad


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "composed"])
def test_eval_logits_match_the_reference(gold, fused):
    m = _model(fused).eval()
    x, _ = R.model_inputs()
    with torch.no_grad():
        logits = m(x.to(_dev()), permutation=torch.from_numpy(gold["eval/perm"]).to(_dev()))
    err = R.rel(logits, gold["eval/logits"])
    print("eval", "fused" if fused else "composed", "%.1e" % err, "err64 %.1e" % float(gold["train/err64/logits"]))
    assert err <= MARGIN * float(gold["train/err64/logits"])


def test_training_step_captures_without_a_memset_and_replays_to_the_eager_bits(gold):
    from adaptpoint_amd import graphs
    dev = _dev()
    m = _model(True).train()
    x, labels = (t.to(dev) for t in R.model_inputs())
    perm = torch.from_numpy(gold["train/perm"]).to(dev)
    params = list(m.parameters())

    def step():
        logits = m(x, permutation=perm)
        grads = torch.autograd.grad(R.model_loss(logits, labels), params)
        return [logits.detach()] + list(grads)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                       # warm-up: allocator pools, lazy initialisation
        step()
    torch.cuda.current_stream().wait_stream(side)
    eager = [t.clone() for t in step()]
    torch.cuda.synchronize()
    gc.collect()
    graph, captured, census = graphs.capture(step, leaves=params, what="the RandLA-Net training step")
    print("RandLA-Net step graph:", census)
    graphs.assert_replayable(graph, "the RandLA-Net training step")
    for _ in range(2):
        for t in captured:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(eager, captured))


def test_reference_named_state_dict_round_trips(gold):
    m = _model(True)
    sd = {n: torch.full([int(s) for s in shape.split(",") if s], 0.25) if not n.endswith("num_batches_tracked")
          else torch.tensor(3) for n, shape in zip(gold["names"].tolist(), gold["shapes"].tolist())}
    m.load_state_dict(sd, strict=True)
    back = m.state_dict()
    assert list(back) == gold["names"].tolist()
    assert all(torch.equal(v.cpu().float(), sd[n].float()) for n, v in back.items())


def test_forty_neighbours_take_the_composed_path_and_say_so():
    from adaptpoint_amd import set_abstraction as SA
    from adaptpoint_amd.randla import LocalFeatureAggregation
    dev = _dev()
    torch.manual_seed(3)
    fused = LocalFeatureAggregation(8, 16, 40, dev, fused=True).to(dev).train()
    composed = LocalFeatureAggregation(8, 16, 40, dev, fused=False).to(dev).train()
    composed.load_state_dict(fused.state_dict())
    coords, feats = torch.rand(2, 96, 3, device=dev), torch.randn(2, 8, 96, 1, device=dev)
    before = sum(v for k, v in SA.FUSED_FALLBACKS.items() if "K = 40" in k)
    out = fused(coords, feats)
    assert sum(v for k, v in SA.FUSED_FALLBACKS.items() if "K = 40" in k) == before + 1
    torch.testing.assert_close(out, composed(coords, feats), rtol=1e-4, atol=1e-5)
