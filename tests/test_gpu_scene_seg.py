"""GPU: csrc/scene_seg.hip through adaptpoint_amd.sceneseg -- the channel-major confusion matrix, the streamed vote merge,
the nearest-neighbour projection and the nearest-k crop against the numpy statements of tests/scene_seg_reference.py
(exact), then `SceneTester` on the kernels against its composed form and one `SegStep` against the same step on the CPU."""
import itertools

import numpy as np
import pytest
import torch

import scene_seg_reference as R

pytestmark = pytest.mark.gpu

_CASES = {}


def _confusion_case(B, C, N, ignore):
    """(logits, target, counts of one full update + one update with valid = B - 1, pred), computed once."""
    key = (B, C, N, ignore)
    if key not in _CASES:
        logits, target = R.confusion_case(B, C, N, 1000 * B + 10 * C + N, ignore)
        full, pred = R.confusion(logits, target, ignore)
        part, _ = R.confusion(logits, target, ignore, valid=B - 1)
        _CASES[key] = (logits, target, full + part, pred)
    return _CASES[key]


# ------------------------------------------------------------------------------------------------------- confusion
@pytest.mark.parametrize("ignore", [None, -100, 255, "C"])
def test_confusion_counters_and_pred_equal_the_numpy_statement(dev, ignore):
    """Ties between channels, NaN, +-inf, all -inf / all-NaN columns, out-of-range and ignored targets; int64 targets
    in the first update, int32 ones under a `valid` scalar below B in the second, accumulated."""
    from adaptpoint_amd import sceneseg
    before = dict(sceneseg.COMPOSED_CALLS)
    for B, C, N in itertools.product((1, 3), (2, 13, 20, 64), (1, 63, 64, 65, 1000)):
        ign = C if ignore == "C" else ignore
        logits, target, want, want_pred = _confusion_case(B, C, N, ign)
        cm = sceneseg.SegMetrics(C, ign, device=dev)
        lg, tg = torch.from_numpy(logits).to(dev), torch.from_numpy(target).to(dev)
        pred = torch.full((B, N), -7, dtype=torch.int32, device=dev)
        cm.update(lg, tg, pred=pred)
        cm.update(lg, tg.clamp(-2 ** 31, 2 ** 31 - 1).to(torch.int32), valid=torch.tensor([B - 1], dtype=torch.int32, device=dev))
        np.testing.assert_array_equal(cm.counts.cpu().numpy(), want, err_msg=f"{(B, C, N, ign)}")
        np.testing.assert_array_equal(pred.cpu().numpy(), want_pred, err_msg=f"{(B, C, N, ign)}")
    assert sceneseg.COMPOSED_CALLS == before                                    # every update ran the kernel


def test_confusion_above_64_classes_takes_the_counted_composed_path(dev):
    from adaptpoint_amd import sceneseg
    B, C, N = 2, 65, 130
    logits, target = R.confusion_case(B, C, N, 77, 255)
    want, want_pred = R.confusion(logits, target, 255)
    cm = sceneseg.SegMetrics(C, 255, device=dev)
    why = f"more than {sceneseg.MAX_CLASSES} classes"
    before = sceneseg.COMPOSED_CALLS.get(why, 0)
    pred = torch.empty(B, N, dtype=torch.int32, device=dev)
    cm.update(torch.from_numpy(logits).to(dev), torch.from_numpy(target).to(dev), pred=pred)
    assert sceneseg.COMPOSED_CALLS.get(why, 0) == before + 1
    np.testing.assert_array_equal(cm.counts.cpu().numpy(), want)
    np.testing.assert_array_equal(pred.cpu().numpy(), want_pred)


def test_confusion_update_replays_from_a_captured_graph(dev):
    from adaptpoint_amd import graphs, sceneseg
    B, C, N = 3, 13, 1000
    logits, target, _, want_pred = _confusion_case(B, C, N, 255)
    want, _ = R.confusion(logits, target, 255)
    lg, tg = torch.from_numpy(logits).to(dev), torch.from_numpy(target).to(dev).to(torch.int32)
    cm = sceneseg.SegMetrics(C, 255, device=dev)
    pred = torch.empty(B, N, dtype=torch.int32, device=dev)
    cm.update(lg, tg, pred=pred)                                                # eager
    torch.cuda.synchronize()
    eager = cm.counts.clone()
    np.testing.assert_array_equal(eager.cpu().numpy(), want)
    graph, _, census = graphs.capture(lambda: cm.update(lg, tg, pred=pred), what="the confusion update")
    assert census.get("memset", 0) == 0
    cm.reset()
    pred.fill_(-1)
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(cm.counts, 2 * eager)
    np.testing.assert_array_equal(pred.cpu().numpy(), want_pred)


# ----------------------------------------------------------------------------------------------------------- votes
def _run_votes(dev, n, C, case, labels=None):
    from adaptpoint_amd.sceneseg import SegMetrics, Votes
    v = Votes(n, C, dev)
    cm = None if labels is None else SegMetrics(C, device=dev)
    for logits, rows in case:
        v.add(torch.from_numpy(logits).to(dev), torch.from_numpy(rows).to(dev))
    pred, mean = v.finish(None if labels is None else torch.from_numpy(labels).to(dev), cm, want_mean=True)
    return pred.cpu().numpy(), mean.cpu().numpy(), None if cm is None else cm.counts.cpu().numpy()


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "normal"])
def test_votes_equal_the_call_order_statement(dev, exact):
    """(i) multiples of 1/8 below 2^10: every partial sum is exact, so mean, pred and counters equal numpy in any order;
    (ii) seeded normal logits: the mean is bit-equal to the fp32 adds in call order, and two runs are bit-equal."""
    for n, C, nparts in itertools.product((1, 65, 1000), (2, 13), (1, 2, 3, 5)):
        case = R.votes_case(n, C, nparts, 100 * n + 10 * C + nparts, exact)
        want = R.votes(n, C, case)
        assert 1 <= want["cnt"].min() and want["cnt"].max() <= 5
        labels = np.random.RandomState(n + C).randint(0, C, n)
        pred, mean, counts = _run_votes(dev, n, C, case, labels)
        assert np.array_equal(mean.view(np.int32), want["mean"].view(np.int32)), (n, C, nparts)
        np.testing.assert_array_equal(pred, want["pred"])
        np.testing.assert_array_equal(counts, R.count(want["pred"], labels, C))
        if exact:                                                               # any order: the parts reversed
            pred_r, mean_r, _ = _run_votes(dev, n, C, case[::-1])
            assert np.array_equal(mean_r.view(np.int32), mean.view(np.int32)) and np.array_equal(pred_r, pred)
        else:
            pred2, mean2, counts2 = _run_votes(dev, n, C, case, labels)
            assert np.array_equal(mean2.view(np.int32), mean.view(np.int32)) and np.array_equal(counts2, counts)


@pytest.mark.parametrize("bad_rows", [[3, 9, 3], [5, 65], [-1, 2]], ids=["repeated", "beyond_n", "negative"])
def test_votes_refuse_repeated_and_out_of_range_rows(dev, bad_rows):
    """The kernel skips the row (range check) or adds it once (stamp exchange) and counts it; `finish` raises; every
    other point's result is the statement's."""
    from adaptpoint_amd.sceneseg import Votes
    n, C = 65, 13
    case = R.votes_case(n, C, 3, 5, exact=False)
    extra = (np.ones((C, len(bad_rows)), np.float32), np.array(bad_rows))
    want = R.votes(n, C, case + [extra])
    assert want["duplicates"] + want["rejected"] == 1
    v = Votes(n, C, dev)
    for logits, rows in case + [extra]:
        v.add(torch.from_numpy(logits).to(dev), torch.from_numpy(rows).to(dev))
    with pytest.raises(ValueError, match="repeated row|outside"):
        v.finish()
    assert v.flags.tolist() == [want["duplicates"], want["rejected"]]
    sure = ~want["unsure"]
    got = (v.acc / v.cnt.clamp(min=1).unsqueeze(1)).cpu().numpy()
    assert np.array_equal(got[sure].view(np.int32), want["mean"][sure].view(np.int32))
    np.testing.assert_array_equal(v.cnt.cpu().numpy(), want["cnt"])


# --------------------------------------------------------------------------------------------------------- project
def test_projection_equals_the_numpy_statement_and_counts_rejects(dev):
    from adaptpoint_amd import sceneseg
    C = 13
    for m, n in itertools.product((1, 70), (1, 500)):
        rng = np.random.RandomState(m + n)
        logits = (np.round(rng.randn(C, m) * 2) / 2).astype(np.float32)
        logits.reshape(-1)[rng.choice(C * m, max(1, C * m // 30), replace=False)] = np.nan
        slot, voxel_of, labels = rng.permutation(m), rng.randint(0, m, n), rng.randint(0, C, n)
        want, rejected = R.project(logits, slot, voxel_of)
        assert rejected == 0
        cm = sceneseg.SegMetrics(C, device=dev)
        to = lambda a: torch.from_numpy(a).to(dev)
        pred = sceneseg.project(to(logits), to(slot), to(voxel_of), to(labels), cm)
        np.testing.assert_array_equal(pred.cpu().numpy(), want)
        np.testing.assert_array_equal(cm.counts.cpu().numpy(), R.count(want, labels, C))
        # out-of-range entries: counted and skipped by the kernel (the raw entry), refused by the Python side
        slot_bad, voxel_bad = slot.copy(), voxel_of.copy()
        slot_bad[m // 2] = m
        voxel_bad[0] = -1
        if n > 3:
            voxel_bad[3] = m + 5
        want, rejected = R.project(logits, slot_bad, voxel_bad)
        assert rejected >= 2 and (want == -1).any()
        i32 = lambda a: torch.from_numpy(a).to(dev).to(torch.int32)
        lg, sl, vo, lb = to(logits), i32(slot_bad), i32(voxel_bad), i32(labels)
        pred_voxel, pred = torch.empty(m, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
        flags, counts = torch.zeros(2, dtype=torch.int32, device=dev), torch.zeros(C * C + 1, dtype=torch.int64, device=dev)
        sceneseg._call("apn_ss_project", dev, C, m, n, lg.data_ptr(), sl.data_ptr(), vo.data_ptr(), lb.data_ptr(), 0, 0,
                       pred_voxel.data_ptr(), counts.data_ptr(), pred.data_ptr(), flags.data_ptr())
        assert flags.tolist() == [0, rejected]
        np.testing.assert_array_equal(pred.cpu().numpy(), want)
        np.testing.assert_array_equal(counts.cpu().numpy(), R.count(want, labels, C))
        with pytest.raises(ValueError, match="outside"):
            sceneseg.project(lg, sl, vo)


# ------------------------------------------------------------------------------------------------------------ crop
@pytest.mark.parametrize("kind", ["uniform", "lattice"])
def test_crop_nearest_equals_the_stable_argsort_set(dev, kind):
    """Seeded uniform clouds, and integer-lattice clouds with repeated points where whole shells of rows tie at the
    cutoff: the output is np.sort(np.argsort(d, kind='stable')[:k]) per cloud -- ascending rows, ties to the lower row."""
    from adaptpoint_amd.sceneseg import crop_nearest
    make = R.uniform_cloud if kind == "uniform" else R.lattice_cloud
    for n, b in itertools.product((1, 64, 65, 1000, 5000), (1, 3)):
        sizes = [n] if b == 1 else [n + 3, n, 2 * n + 1]
        coord = np.concatenate([make(s, 7 * n + i) for i, s in enumerate(sizes)])
        centres = [(s * 2) // 3 for s in sizes]
        dcoord = torch.from_numpy(coord).to(dev)
        for k in sorted({k for k in (1, 24, n - 1, n) if 1 <= k <= n}):
            got = crop_nearest(dcoord, sizes, centres, k).cpu().numpy()
            np.testing.assert_array_equal(got, R.crop(coord, sizes, centres, k), err_msg=f"{(kind, n, b, k)}")
            assert (np.diff(got, axis=1) > 0).all()


def test_crop_refuses_short_clouds_before_any_launch_and_bad_coordinates_after(dev, monkeypatch):
    from adaptpoint_amd import sceneseg
    coord = torch.from_numpy(R.uniform_cloud(100, 1)).to(dev)
    launches = []
    real = sceneseg._call
    monkeypatch.setattr(sceneseg, "_call", lambda *a: (launches.append(a[0]), real(*a)))
    with pytest.raises(ValueError, match="pad first"):
        sceneseg.crop_nearest(coord, [60, 40], [0, 0], 41)
    assert launches == []
    coord[17, 2] = float("nan")
    with pytest.raises(ValueError, match="non-finite"):
        sceneseg.crop_nearest(coord, [60, 40], [0, 0], 8)
    assert launches == ["apn_ss_crop_nearest"]
    with pytest.raises(ValueError, match="refused"):
        sceneseg.crop_nearest(coord[:10].contiguous(), [10], [10], 2)           # a centre outside its cloud: nothing written


# ------------------------------------------------------------------------------------------------------ end to end
NARROW = dict(blocks=(1, 1, 1), strides=(1, 2, 2), width=8, nsample=16, radius=0.1)


def _narrow_model(device, narrow=NARROW, **kw):
    from adaptpoint_amd.pointnext import fill_parameters_by_name
    from adaptpoint_amd.sceneseg import POINTNEXT_S_ENCODER, BaseSeg
    model = BaseSeg(encoder_args=dict(POINTNEXT_S_ENCODER, **narrow), cls_args=dict(num_classes=R.NUM_CLASSES, dropout=0.0,
                                                                                   norm_args={'norm': 'bn'}), **kw)
    return fill_parameters_by_name(model).to(device)


def test_scene_tester_on_the_kernels_equals_its_composed_form(dev):
    """A width-8 BaseSeg with strides (1,2,2) on a seeded 2000-point scene at voxel 0.1: the kernels' pred and counters
    equal, bit for bit, the composed form's (index_add_ per part -- sequential, a part's rows being distinct)."""
    from adaptpoint_amd import sceneseg
    coord, feat, label = (torch.from_numpy(a).to(dev) for a in R.scene(2000, 44))
    model = _narrow_model(dev)
    results = []
    for fused in (True, False):
        before = dict(sceneseg.COMPOSED_CALLS)
        tester = sceneseg.SceneTester(model, R.NUM_CLASSES, voxel_size=0.1, ignore_index=12, fused=fused)
        np.random.seed(9)
        cm = tester(coord, feat, label)
        assert (sceneseg.COMPOSED_CALLS == before) == fused
        results.append((tester.pred.cpu().numpy(), cm.counts.cpu().numpy(), [r.cpu().numpy() for r in tester.parts]))
    (pred, counts, parts), (pred_c, counts_c, parts_c) = results
    assert len(parts) == len(parts_c) > 1 and all(np.array_equal(a, b) for a, b in zip(parts, parts_c))
    np.testing.assert_array_equal(pred, pred_c)
    np.testing.assert_array_equal(counts, counts_c)
    assert counts[:-1].sum() == int((label != 12).sum()) and counts[-1] == 0
    np.testing.assert_array_equal(counts, R.count(pred, label.cpu().numpy(), R.NUM_CLASSES, 12))
    # the nearest-neighbour mode, kernels against composed
    out = []
    for fused in (True, False):
        tester = sceneseg.SceneTester(model, R.NUM_CLASSES, voxel_size=0.1, mode='nearest_neighbor', fused=fused)
        np.random.seed(10)
        cm = tester(coord, feat, label)
        out.append((tester.pred.cpu().numpy(), cm.counts.cpu().numpy()))
    np.testing.assert_array_equal(out[0][0], out[1][0])
    np.testing.assert_array_equal(out[0][1], out[1][1])


def test_scene_sampler_on_the_kernels_equals_its_composed_form(dev):
    from adaptpoint_amd.sceneseg import SceneSampler
    scenes = [tuple(torch.from_numpy(a).to(dev) for a in R.scene(n, 60 + i)) for i, n in enumerate((3000, 90, 1500))]
    out = []
    for fused in (True, False):
        np.random.seed(4)
        out.append(SceneSampler(voxel_size=0.1, voxel_max=256, fused=fused).batch(scenes))
    for key in ('pos', 'x', 'y'):
        assert torch.equal(out[0][key], out[1][key]), key
    assert out[0]['pos'].shape == (3, 256, 3) and out[0]['x'].shape == (3, 4, 256)


def test_seg_step_on_the_gpu_meets_the_same_step_on_the_cpu(dev, oracle):
    """One `SegStep` (forward, smoothed cross entropy with an ignored label, backward, clipping, AdamW) on the device
    against the same step on CPU tensors over the oracle, at the bars tests/test_gpu_partseg.py quotes from
    tests/test_gpu_propagation.py: rtol 1e-5 / atol 1e-5 on the outputs, rtol 1e-4 / atol 1e-5 on the gradients; and the
    step's metric update against the numpy statement on the device's own logits.
    The model has two stages (one down-sampling, two propagation blocks): the step's logic does not depend on the depth,
    and the float32 distance between the two machines grows with it.  Measured on the MI355X: largest logit difference
    9.8e-6 here (0.53 of the bar; logits up to 7.2), against 3.2e-5 (1.3 of the bar, 4 of 6656 logits) with the three
    stages of the scene test above; the gradients stay below 0.11 of their bar in both, and two runs on the device are
    bit-equal."""
    import contextlib

    import golden_inputs as GI
    from adaptpoint_amd import sceneseg
    from oracle import cpu_block as CB
    B, N, C = 2, 256, R.NUM_CLASSES
    g = torch.Generator().manual_seed(3)
    pos = torch.from_numpy(GI.unit_sphere_cloud(B, N, seed=71)) * 0.5
    x = torch.cat([torch.rand(B, N, 3, generator=g), pos[:, :, 2:3] - pos[:, :, 2:3].min(1, keepdim=True)[0]], -1)
    y = torch.randint(0, C, (B, N), generator=g)
    y[0, :9] = 255
    data = {'pos': pos, 'x': x.transpose(1, 2).contiguous(), 'y': y}
    two_stages = dict(NARROW, blocks=(1, 1), strides=(1, 2))
    cpu_model = _narrow_model("cpu", two_stages)
    gpu_model = _narrow_model("cpu", two_stages)
    gpu_model.load_state_dict(cpu_model.state_dict())
    gpu_model.to(dev)
    runs = {}
    for name, model, device in (("cpu", cpu_model, torch.device("cpu")), ("gpu", gpu_model, dev)):
        grads = []
        cm = sceneseg.SegMetrics(C, 255, device=device)
        crit = sceneseg.SmoothCrossEntropy(0.2, ignore_index=255, num_classes=C).to(device)
        step = sceneseg.SegStep(model, criterion=crit, metrics=cm, grad_sync=lambda gs: grads.extend(t.detach().clone() for t in gs))
        with (CB.CpuOps() if name == "cpu" else contextlib.nullcontext()):     # the oracle under adaptpoint_amd.ops
            logits, loss = step({k: v.to(device) for k, v in data.items()})
        runs[name] = (logits.cpu().numpy(), float(loss), [t.cpu().numpy() for t in grads], cm.counts.cpu().numpy())
    (lc, loss_c, gc, _), (lg, loss_g, gg, counts) = runs["cpu"], runs["gpu"]
    np.testing.assert_allclose(lg, lc, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(loss_g, loss_c, rtol=1e-5, atol=1e-5)
    assert len(gg) == len(gc) == len(list(gpu_model.parameters()))
    for (pname, _), a, b in zip(gpu_model.named_parameters(), gg, gc):
        np.testing.assert_allclose(a, b, rtol=1e-4, atol=1e-5, err_msg=pname)
    want, _ = R.confusion(lg, y.numpy(), 255)
    np.testing.assert_array_equal(counts, want)
