"""CPU suite of RandLA-Net (adaptpoint_amd/randla.py): the composed modules against the REFERENCE's captured in
tests/golden/randla_golden.npz (tests/golden/make_golden_randla.py) at the bars of tests/test_deepgcn_cpu.py, the two
identities the fused layer rests on in float64 (tests/randla_reference.py), and the argument checks of the apn_rl_*
entries (no launch is reached)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import randla_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-5          # relative L2 per gradient tensor / buffer, logits at rtol 1e-5: tests/test_deepgcn_cpu.py's
NOISE = 1e-4        # a gradient that is an analytic zero (the golden's err64 > 0.5): its norm relative to the layer's weight gradient


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "randla_golden.npz"))


def _model(fused=False, **kw):
    from adaptpoint_amd.pointnext import fill_parameters_by_name
    from adaptpoint_amd.randla import RandLANet
    m = fill_parameters_by_name(RandLANet(device=torch.device('cpu'), fused=fused, **dict(R.MODEL, **kw)))
    m.fc_end[2].p = 0.0
    return m


def test_state_dict_names_and_shapes_are_the_references(gold):
    sd = _model().state_dict()
    assert [(n, ",".join(str(s) for s in t.shape)) for n, t in sd.items()] == \
        list(zip(gold["names"].tolist(), gold["shapes"].tolist()))
    assert sd["decoder.0.conv.weight"].shape == (1024, 256, 1, 1)          # ConvTranspose2d: (in, out, 1, 1)
    assert sd["encoder.1.pool1.score_fn.0.weight"].shape == (64, 64)       # the full 2C x 2C score weight
    assert sd["encoder.0.lse1.mlp.conv.weight"].shape == (8, 10, 1, 1)


def test_composed_model_matches_the_reference_in_training_mode(gold):
    """With the golden's seed the forward draws the reference's permutation at the reference's place in the host stream;
    graphs, logits, buffers and gradients follow."""
    m = _model().train()
    x, labels = R.model_inputs()
    torch.manual_seed(R.MODEL_SEED)
    logits = m(x, keep_graphs=True)
    R.model_loss(logits, labels).backward()
    assert torch.rand(1).item() == float(gold["train/next_rand"])
    for i, (idx, _) in enumerate(m.last_graphs['encoder']):
        assert idx.dtype == torch.int32 and np.array_equal(idx.numpy(), gold[f"train/graph/encoder{i}"]), i
    for i, idx in enumerate(m.last_graphs['decoder']):
        assert np.array_equal(idx.numpy(), gold[f"train/graph/decoder{i}"]), i
    np.testing.assert_allclose(logits.detach().numpy(), gold["train/logits"], rtol=1e-5)
    params, buffers = dict(m.named_parameters()), dict(m.named_buffers())
    names = [k[len("train/grad/"):] for k in gold.files if k.startswith("train/grad/")]
    assert sorted(names) == sorted(params)
    errs = {}
    for n in names:
        g = params[n].grad.reshape(-1)[torch.from_numpy(R.sample_index(n, params[n].numel()))]
        if float(gold["train/err64/grad/" + n]) > 0.5:
            companion = params[n[:-len("bias")] + "weight"].grad.norm().item()
            assert g.norm().item() <= NOISE * companion, n
        else:
            errs["grad/" + n] = R.rel(g, gold["train/grad/" + n])
    for k in gold.files:
        if k.startswith("train/buf/"):
            n = k[len("train/buf/"):]
            if n.endswith("num_batches_tracked"):
                assert int(buffers[n]) == int(gold[k]) == 1, n
            else:
                errs["buf/" + n] = R.rel(buffers[n], gold[k])
    assert max(errs.values()) < BAR, {k: v for k, v in errs.items() if v >= BAR}


def test_composed_model_matches_the_reference_in_eval_mode(gold):
    m = _model().eval()
    x, _ = R.model_inputs()
    with torch.no_grad():
        logits = m(x, permutation=torch.from_numpy(gold["eval/perm"]))
        torch.manual_seed(R.MODEL_SEED)
        drawn = m(x)
    np.testing.assert_allclose(logits.numpy(), gold["eval/logits"], rtol=1e-5)
    assert torch.equal(logits, drawn)            # a supplied permutation is the drawn one's equal


def test_reference_state_dict_round_trips(gold):
    m = _model()
    sd = {n: torch.full([int(s) for s in shape.split(",") if s], 0.25) if not n.endswith("num_batches_tracked")
          else torch.tensor(3) for n, shape in zip(gold["names"].tolist(), gold["shapes"].tolist())}
    m.load_state_dict(sd, strict=True)
    assert all(torch.equal(v.float(), sd[n].float()) for n, v in m.state_dict().items())


def test_limits_are_refused_loudly():
    m = _model()
    with pytest.raises(ValueError, match="points"):
        m(torch.zeros(1, 24, 6))                 # 24 points do not divide into four levels of decimation 2
    from adaptpoint_amd.randla import LocalFeatureAggregation
    with pytest.raises(ValueError, match="dist"):
        LocalFeatureAggregation(8, 16, 4, torch.device('cpu'), dist='manhattan')


@pytest.mark.parametrize("case", [(2, 64, 16, 32), (1, 37, 3, 8)])
def test_batchnorm_statistics_follow_from_the_encodings_moments(case):
    """mean_c = w_c . mu + b_c and var_c = w_c^T Sigma w_c against the direct statistics over (B,C,N,K), in float64."""
    t = R.tensors(R.layer_inputs(*case, seed=3), 'cpu', torch.float64)
    e = R.encoding(t['coords'], t['idx'], t['dist'])
    _, mean, var = R.hidden(e, t['w'], t['b'], t['gamma'], t['beta'])
    mean_m, var_m = R.moment_statistics(e, t['w'], t['b'])
    assert R.rel(mean_m, mean) < 1e-12 and R.rel(var_m, var) < 1e-12


@pytest.mark.parametrize("case", [(2, 64, 16, 32), (1, 37, 3, 8)])
def test_reduced_pooling_equals_the_full_layer_in_float64(case):
    """[sum_k softmax_k(A_hh h_k) h_k ; f] is the full 2C x 2C layer's output, and the three dead blocks of the score
    weight have no gradient: float64 leaves only rounding."""
    inputs = R.layer_inputs(*case, seed=5)
    C = case[3]
    full, gf, _, _ = R.layer_with_gradients(R.full_layer, inputs, 'cpu', torch.float64)
    red, gr, _, _ = R.layer_with_gradients(R.reduced_layer, inputs, 'cpu', torch.float64)
    assert R.rel(red, full) < 1e-13
    for k in R.PARAMS:
        if k == 'b':                              # an analytic zero in front of a training-mode BatchNorm
            assert gf[k].norm() <= 1e-10 * gf['w'].norm() and gr[k].norm() <= 1e-10 * gr['w'].norm()
        else:
            assert R.rel(gr[k], gf[k]) < 1e-11, k
    hh = gf['A'][:C, :C].norm()
    assert max(gf['A'][:C, C:].norm(), gf['A'][C:, :C].norm(), gf['A'][C:, C:].norm()) <= 1e-12 * hh
    assert not gr['A'][:C, C:].any() and not gr['A'][C:, :C].any() and not gr['A'][C:, C:].any()


def test_entry_points_validate_their_arguments_without_a_gpu():
    from adaptpoint_amd import _lib
    lib = _lib.load()
    EINVAL = lib.apn_rl_forward(1, 4, 0, 8, None, None, None, 0, None, None, None, None)
    assert EINVAL != 0
    buf = (ctypes.c_double * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    fwd = lambda b, n, k, c, q=p: lib.apn_rl_forward(b, n, k, c, q, q, q, 0, q, q, q, None)
    bwd = lambda b, n, k, c, q=p: lib.apn_rl_backward(b, n, k, c, q, q, q, 0, q, q, q, q, q, None)
    mom = lambda b, n, k, q=p: lib.apn_rl_moments(b, n, k, q, q, q, 0, q, q, None)
    for call in (fwd, bwd):
        assert call(1, 4, 4, 12) == EINVAL                      # a width outside {8, 16, 32, 64, 128}
        assert call(1, 4, 0, 8) == EINVAL and call(1, 4, 33, 8) == EINVAL
        assert call(1, 4, 4, 8, None) == EINVAL                 # null pointers
        assert call(1, 1 << 24, 4, 8) == EINVAL and call(-1, 4, 4, 8) == EINVAL
        assert call(0, 4, 4, 8) == 0 and call(0, 4, 4, 8, None) == 0          # B = 0: nothing to do
    assert mom(1, 4, 0) == EINVAL and mom(1, 4, 33) == EINVAL and mom(1, 4, 4, None) == EINVAL and mom(0, 4, 4) == 0
    fold = lambda c, m, w: lib.apn_rl_fold(c, m, 16.0, w, None, None, None, 1e-6, 0.99, 1, None, None, None, p, p, None)
    assert fold(12, p, p) == EINVAL and fold(8, None, p) == EINVAL and fold(8, p, None) == EINVAL
    assert lib.apn_rl_fold(8, None, 16.0, p, None, None, None, 1e-6, 0.99, 0, None, None, None, p, p, None) == EINVAL
    fin = lambda c, rows, part: lib.apn_rl_finalize(c, rows, part, p, 16.0, p, None, None, p, 1, p, p, None)
    assert fin(12, 1, p) == EINVAL and fin(8, 1, None) == EINVAL and fin(8, -1, p) == EINVAL and fin(8, 2000, p) == EINVAL
    assert lib.apn_rl_moment_rows(1, 4, 0) == 0 and lib.apn_rl_moment_rows(1, 4, 4) == 1
    assert lib.apn_rl_bwd_rows(1, 4, 4, 12) == 0 and lib.apn_rl_bwd_rows(3, 130, 16, 128) == 98
