"""CPU: adaptpoint_amd.partseg and the host side of adaptpoint_amd.part_metrics against goldens made by the reference's own
`PointNextPartDecoder`, `BasePartSeg`, losses and `get_ins_mious` (tests/golden/make_golden_partseg.py); inputs
regenerated from seeds by tests/partseg_reference.py."""
import os

import numpy as np
import pytest
import torch

import partseg_reference as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "partseg_golden.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


def mirror_decoder(cls_map, hoisted, **over):
    from adaptpoint_amd.partseg import PointNextPartDecoder
    from adaptpoint_amd.pointnext import fill_parameters_by_name
    dec = PointNextPartDecoder(hoisted=hoisted, cls2partembed=R.part_embed() if 'pointnext' in cls_map else None,
                               **R.decoder_args(cls_map, **over))
    return fill_parameters_by_name(dec).train()


def check_decoder(gold, tag, res):
    """tests/test_propagation_cpu.py's bars for the unconditioned decoder: rtol 1e-4 / atol 1e-5 on the output and on
    every gradient (the one gradient that is zero in exact arithmetic -- make_golden_partseg.py -- by atol alone)."""
    keys = [k[len(f"dec/{tag}/"):] for k in gold.files if k.startswith(f"dec/{tag}/") and not k.endswith("err64")]
    assert {k for k in keys if k.startswith("grad/")} == {k for k in res if k.startswith("grad/")}
    for k in keys:
        if k.endswith("num_batches_tracked"):
            assert int(res[k]) == int(gold[f"dec/{tag}/{k}"])
        else:
            np.testing.assert_allclose(res[k], gold[f"dec/{tag}/{k}"], rtol=1e-4, atol=1e-5, err_msg=f"{tag}: {k}")


@pytest.mark.parametrize("hoisted", [False, True], ids=["composed", "hoisted"])
@pytest.mark.parametrize("cls_map", R.CLS_MAPS)
def test_part_decoder_meets_reference_goldens(gold, cpu_mirrors, oracle, cls_map, hoisted):
    p, f, cls, gout = R.pyramid(int(gold["dec/seed"]), oracle.furthest_point_sampling)
    dec = mirror_decoder(cls_map, hoisted)
    assert all(stage[0].hoisted == hoisted for stage in dec.decoder)
    check_decoder(gold, cls_map, R.run_decoder(dec, p, f, cls, gout))


@pytest.mark.parametrize("hoisted", [False, True], ids=["composed", "hoisted"])
def test_part_decoder_with_an_invresmlp_block_meets_reference_goldens(gold, cpu_mirrors, oracle, hoisted):
    p, f, cls, gout = R.pyramid(int(gold["dec/seed"]), oracle.furthest_point_sampling)
    over = {k: v for k, v in R.BLOCKS_CASE.items() if k != 'cls_map'}
    dec = mirror_decoder(R.BLOCKS_CASE['cls_map'], hoisted, **over)
    assert [len(stage) for stage in dec.decoder] == [2, 1]
    check_decoder(gold, "blocks", R.run_decoder(dec, p, f, cls, gout))


def test_hoisted_conditioning_vector_is_the_repeated_tensor(cpu_mirrors, oracle):
    """`conditioning` (B,Cc) against the composed (B,Cc,N) tensor of the reference's statements: every column."""
    p, f, cls, _ = R.pyramid(0, oracle.furthest_point_sampling)
    for cls_map in R.CLS_MAPS:
        dec = mirror_decoder(cls_map, True)
        vec = dec.conditioning(f, cls)
        full = dec._conditioning_composed(f, cls, R.NARROW_N)
        assert tuple(vec.shape) == (R.NARROW_B, dec.cond_channels) and tuple(full.shape) == vec.shape + (R.NARROW_N,)
        torch.testing.assert_close(vec.unsqueeze(-1).expand_as(full), full, rtol=1e-6, atol=1e-6)


def test_default_basepartseg_carries_the_reference_state_dict(gold):
    from adaptpoint_amd.partseg import BasePartSeg
    for kw in (dict(), dict(hoisted=True)):
        sd = BasePartSeg(**kw).state_dict()
        assert list(sd.keys()) == list(gold["sd/names"])
        assert [",".join(str(s) for s in t.shape) for t in sd.values()] == list(gold["sd/shapes"])


def test_losses_meet_reference_values_and_gradients(gold):
    from adaptpoint_amd.partseg import Poly1FocalLoss, SmoothCrossEntropy, get_class_weights
    logits, labels, counts = R.loss_inputs(0)
    weight = get_class_weights(counts, normalize=True)
    np.testing.assert_array_equal(weight.numpy(), gold["loss/class_weights"])
    for tag, crit in (("poly1", Poly1FocalLoss()), ("smooth", SmoothCrossEntropy(0.2)),
                      ("smooth_weighted", SmoothCrossEntropy(0.2, weight=weight)), ("ce", SmoothCrossEntropy(0.0))):
        x = logits.clone().requires_grad_(True)
        v = crit(x, labels)
        v.backward()
        # the same torch operations in the same order on the same machine class: float32 rounding at most
        np.testing.assert_allclose(v.detach().numpy(), gold[f"loss/{tag}/value"], rtol=1e-6, err_msg=tag)
        np.testing.assert_allclose(x.grad.numpy(), gold[f"loss/{tag}/grad"], rtol=1e-5, atol=1e-8, err_msg=tag)


def _metric_cases():
    cases = [(n, p, t, c, tab) for n, p, t, c, tab, _ in R.crafted_cases()]
    for i, (B, N, C) in enumerate(((5, 63, 50), (7, 64, 64), (3, 2048, 50), (4, 1, 50))):
        logits, target, cls, table = R.random_case(B, N, C, 9500 + i)
        cases.append((f"random{i}", R.predict(logits), target, cls, table))
    return cases


def test_numpy_statement_of_the_metric_meets_get_ins_mious(gold):
    """The bar: twice the reference's own float32-against-float64 distance.  The quotients are correctly
    rounded on both sides; the reference's torch.mean adds them in another order than left to right, so the last bit of
    a shape's mean can differ (the generator measured one float32 ulp at 100, 7.6e-6)."""
    bar = 2.0 * float(gold["m/mean_err64"])
    assert float(gold["m/mean_diff"]) <= bar
    for name, pred, target, cls, table in _metric_cases():
        mine = R.shape_ious(pred, target, cls, table)
        ref = gold[f"m/{name}/ious"]
        assert np.abs(mine.astype(np.float64) - ref.astype(np.float64)).max() <= bar, name
    # the corners, by hand: an absent part scores 100; a label outside the category is in no part; all wrong
    crafted = {n: R.shape_ious(p, t, c, tab) for n, p, t, c, tab in _metric_cases()[:4]}
    np.testing.assert_allclose(crafted["absent_part"], [(100 * 5 / 6 + 100 * 6 / 7 + 100 + 100) / 4], rtol=1e-6)
    np.testing.assert_allclose(crafted["outside_label"], [(100 * 3 / 6 + 100 * 4 / 6) / 2], rtol=1e-6)
    np.testing.assert_array_equal(crafted["all_wrong"], [0.0, 0.0])


def test_totals_and_closing_arithmetic_meet_validate(gold):
    from adaptpoint_amd.part_metrics import finish
    state = None
    for name, pred, target, cls, table in _metric_cases()[:3]:           # three uneven batches, ShapeNetPart's table
        state = R.totals(R.shape_ious(pred, target, cls, table), cls, 16, state)
    ins_miou, cls_miou, cls_mious = finish(*state)
    # the shapes' means are the reference's to the last bit on these cases, and so are the per-category values; the
    # instance mean is a float64 sum here against torch.sum's float32 one: float32 rounding
    np.testing.assert_array_equal(cls_mious, gold["m/validate/cls_mious"])
    assert cls_mious[4:].tolist() == [0.0] * 12                          # categories that never occur contribute 0
    np.testing.assert_allclose(cls_miou, gold["m/validate/cls_miou"], rtol=1e-6)
    np.testing.assert_allclose(ins_miou, gold["m/validate/ins_miou"], rtol=1e-6)
    with pytest.raises(ValueError):
        finish(*state, rejected=1)


def test_csr_table_keeps_list_order():
    from adaptpoint_amd.part_metrics import csr_table
    offset, ids = csr_table([[5, 0, 9], [2, 3], [7], [1, 4, 6, 8]])
    assert offset.tolist() == [0, 3, 5, 6, 10] and ids.tolist() == [5, 0, 9, 2, 3, 7, 1, 4, 6, 8]
    assert offset.dtype == np.int32 and ids.dtype == np.int32


def test_propagate_with_cond_equals_the_composed_block_on_the_torch_path():
    """float64 on the CPU: the hoisted algebra with a conditioning vector against repeat + concatenate + conv + BN."""
    from adaptpoint_amd import propagation
    torch.manual_seed(0)
    B, Cc, C1, C2, O, n, m = 3, 5, 4, 6, 7, 20, 9
    for skip in (True, False):
        conv = torch.nn.Conv1d(Cc + (C1 if skip else 0) + C2, O, 1, bias=False).double()
        bn, bn2 = torch.nn.BatchNorm1d(O).double(), torch.nn.BatchNorm1d(O).double()
        cond = torch.randn(B, Cc, dtype=torch.double, requires_grad=True)
        f1 = torch.randn(B, C1, n, dtype=torch.double) if skip else None
        f2 = torch.randn(B, C2, m, dtype=torch.double)
        idx = torch.randint(0, m, (B, n, 3))
        w = torch.rand(B, n, 3, dtype=torch.double)
        w = w / w.sum(2, keepdim=True)
        assert not propagation.supported(f1, f2, conv, bn, cond)          # CPU tensors: the torch form
        out = propagation.propagate(f1, f2, idx, w, conv, bn, cond=cond)
        g = torch.autograd.grad(out.sum() + (out ** 2).sum(), [cond, conv.weight])
        parts = [cond.unsqueeze(-1).expand(-1, -1, n)] + ([f1] if skip else []) + [propagation.blend(f2, idx, w)]
        ref = torch.relu(bn2(conv(torch.cat(parts, 1))))
        g_ref = torch.autograd.grad(ref.sum() + (ref ** 2).sum(), [cond, conv.weight])
        torch.testing.assert_close(out, ref, rtol=1e-12, atol=1e-12)
        for a, b in zip(g, g_ref):
            torch.testing.assert_close(a, b, rtol=1e-10, atol=1e-12)
        torch.testing.assert_close(bn.running_var, bn2.running_var, rtol=1e-12, atol=1e-12)
