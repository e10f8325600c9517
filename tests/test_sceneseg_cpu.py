"""CPU: adaptpoint_amd.sceneseg against goldens made by the reference's own `BaseSeg`, `PointNextDecoder`, `SegHead`,
`SmoothCrossEntropy(ignore_index=...)` and `ConfusionMatrix` (tests/golden/make_golden_sceneseg.py), and its composed
paths -- the confusion counters, the vote merge, the projection, the crop, `SceneTester`, `SceneSampler` -- against the
numpy statements of tests/scene_seg_reference.py.  Inputs are regenerated from seeds."""
import os

import numpy as np
import pytest
import torch

import scene_seg_reference as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sceneseg_golden.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


# ------------------------------------------------------------------------------------------------------- the model
def test_default_baseseg_carries_the_reference_state_dict_and_loads_strictly(gold):
    from adaptpoint_amd.sceneseg import BaseSeg
    for kw in (dict(), dict(hoisted=True)):
        model = BaseSeg(**kw)
        assert [n for n, _ in model.named_children()] == ["encoder", "decoder", "head"]
        sd = model.state_dict()
        assert list(sd.keys()) == list(gold["sd/names"])
        assert [",".join(str(s) for s in t.shape) for t in sd.values()] == list(gold["sd/shapes"])
    # a state_dict with the reference's names and shapes loads with strict=True
    ref_sd = {n: torch.zeros([int(s) for s in shape.split(",") if s]) for n, shape in zip(gold["sd/names"], gold["sd/shapes"])}
    ref_sd = {n: (t.long() if n.endswith("num_batches_tracked") else t) for n, t in ref_sd.items()}
    res = BaseSeg().load_state_dict(ref_sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys


def test_decoder_args_are_merged_over_encoder_args():
    from adaptpoint_amd.sceneseg import POINTNEXT_S_ENCODER, BaseSeg
    enc = dict(POINTNEXT_S_ENCODER, blocks=(1, 1, 1), strides=(1, 2, 2), width=8, in_channels=5)
    model = BaseSeg(encoder_args=dict(enc, NAME='PointNextEncoder'), decoder_args=dict(NAME='PointNextDecoder', decoder_layers=3),
                    cls_args=dict(NAME='SegHead', num_classes=4, global_feat='max,avg'), hoisted=True)
    # three encoder levels: two skip levels plus the input's channels (merged from the encoder's in_channels)
    assert len(model.decoder.decoder) == 3 and model.decoder.decoder[0][0].convs[0][0].in_channels == 5 + 16
    assert all(len(stage[0].convs) == 3 and stage[0].hoisted for stage in model.decoder.decoder)
    assert model.head.global_feat == ['max', 'avg'] and model.head.head[0][0].in_channels == 3 * 8
    assert model.head.head[-1][0].out_channels == 4


@pytest.mark.parametrize("hoisted", [False, True], ids=["composed", "hoisted"])
@pytest.mark.parametrize("head_case", list(R.HEAD_CASES))
def test_decoder_and_head_meet_reference_goldens(gold, cpu_mirrors, oracle, head_case, hoisted):
    """The bars tests/test_gpu_partseg.py quotes from tests/test_gpu_propagation.py: rtol 1e-5 / atol 1e-5 on the output,
    rtol 1e-4 / atol 1e-5 on the gradients."""
    from adaptpoint_amd.partseg import SegHead
    from adaptpoint_amd.pointnext import PointNextDecoder, fill_parameters_by_name
    p, f, gout = R.seg_pyramid(int(gold["dh/seed"]), oracle.furthest_point_sampling)
    dec = fill_parameters_by_name(PointNextDecoder(list(R.NARROW_CHANNELS), in_channels=R.NARROW_IN, hoisted=hoisted)).train()
    head = fill_parameters_by_name(SegHead(in_channels=dec.out_channels, **R.HEAD_CASES[head_case])).train()
    res = R.run_decoder_head(dec, head, p, f, gout)
    keys = [k[len(f"dh/{head_case}/"):] for k in gold.files if k.startswith(f"dh/{head_case}/")]
    assert {k for k in keys if k.startswith("grad/")} == {k for k in res if k.startswith("grad/")}
    for k in keys:
        want = gold[f"dh/{head_case}/{k}"]
        if k.endswith("num_batches_tracked"):
            assert int(res[k]) == int(want)
        else:
            np.testing.assert_allclose(res[k], want, rtol=1e-5 if k == "out" else 1e-4, atol=1e-5, err_msg=f"{head_case}: {k}")


# -------------------------------------------------------------------------------------------------------- the loss
@pytest.mark.parametrize("ignore", R.LOSS_IGNORES)
def test_smooth_cross_entropy_with_ignore_index_meets_reference(gold, ignore):
    from adaptpoint_amd.sceneseg import SmoothCrossEntropy
    logits, labels, _ = R.loss_inputs(0, ignore)
    C = logits.shape[1]
    for tag, smoothing in (("smooth", 0.2), ("ce", 0.0)):
        crit = SmoothCrossEntropy(label_smoothing=smoothing, ignore_index=ignore, num_classes=C)
        np.testing.assert_array_equal(crit.reducing_list.numpy(), gold[f"loss/{ignore}/reducing_list"])
        assert "reducing_list" not in crit.state_dict()
        x = logits.clone().requires_grad_(True)
        v = crit(x, labels)
        v.backward()
        # the same torch operations in the same order on the same machine class: float32 rounding at most
        np.testing.assert_allclose(v.detach().numpy(), gold[f"loss/{ignore}/{tag}/value"], rtol=1e-6, err_msg=tag)
        np.testing.assert_allclose(x.grad.numpy(), gold[f"loss/{ignore}/{tag}/grad"], rtol=1e-5, atol=1e-8, err_msg=tag)
    loss, kept, gt = SmoothCrossEntropy(0.2, ignore_index=ignore, num_classes=C, return_valid=True)(logits, labels)
    assert kept.shape == (int((labels != ignore).sum()), C) and gt.shape == kept.shape[:1]
    # without ignore_index it is partseg's loss
    from adaptpoint_amd import partseg
    plain, plain_labels, _ = R.PR.loss_inputs(0)
    assert torch.equal(SmoothCrossEntropy(0.2)(plain, plain_labels), partseg.SmoothCrossEntropy(0.2)(plain, plain_labels))


# ------------------------------------------------------------------------------------------------------ the metric
@pytest.mark.parametrize("case", R.METRIC_CASES, ids=[c[0] for c in R.METRIC_CASES])
def test_segmetrics_arithmetic_meets_the_reference_confusion_matrix(gold, case):
    """The composed counters on CPU tensors, fed logits whose argmax is the golden's prediction, and the closing
    arithmetic: the same torch operations on the same int64 tensors, so equal to the last bit."""
    from adaptpoint_amd import sceneseg
    name, C, n, ignore = case
    cm = sceneseg.SegMetrics(C, ignore, device="cpu")
    before = dict(sceneseg.COMPOSED_CALLS)
    for seed in gold[f"m/{name}/seeds"]:
        pred, true = R.metric_inputs(int(seed), C, n, ignore)
        logits = torch.zeros(1, C, n).scatter_(1, torch.from_numpy(pred).view(1, 1, n), 1.0)
        cm.update(logits, torch.from_numpy(true).view(1, n))
    assert sceneseg.COMPOSED_CALLS.get("CPU tensor", 0) == before.get("CPU tensor", 0) + 2
    np.testing.assert_array_equal(cm.value.numpy(), gold[f"m/{name}/value"])
    assert int(cm.rejected) == 0
    miou, macc, oa, ious, accs = cm.all_metrics()
    assert [miou, macc, oa] == list(gold[f"m/{name}/all_metrics"])
    np.testing.assert_array_equal(ious, gold[f"m/{name}/ious"])
    np.testing.assert_array_equal(accs, gold[f"m/{name}/accs"])
    assert list(cm.all_acc()[:2]) == list(gold[f"m/{name}/all_acc"])
    for got in (cm.mious(), sceneseg.get_mious(cm.tp, cm.union, cm.count)):
        assert list(got[:3]) == list(gold[f"m/{name}/get_mious"])
        np.testing.assert_array_equal(got[3], gold[f"m/{name}/get_mious_ious"])
        np.testing.assert_array_equal(got[4], gold[f"m/{name}/get_mious_accs"])
    assert cm.overall_accuray.item() == float(gold[f"m/{name}/overall_accuray"])
    assert int(cm.total) == int(gold[f"m/{name}/value"].sum())
    other = sceneseg.SegMetrics(C, ignore, device="cpu")
    other.add(cm)
    other.add(cm)
    np.testing.assert_array_equal(other.value.numpy(), 2 * gold[f"m/{name}/value"])
    cm.reset()
    assert int(cm.total) == 0


@pytest.mark.parametrize("ignore", [None, -100, 255, 5])
def test_composed_confusion_equals_the_numpy_statement(ignore):
    from adaptpoint_amd.sceneseg import SegMetrics
    B, C, N = 3, 5, 65
    logits, target = R.confusion_case(B, C, N, 3, ignore)
    want, want_pred = R.confusion(logits, target, ignore, valid=2)
    cm = SegMetrics(C, ignore, device="cpu")
    pred = torch.empty(B, N, dtype=torch.int32)
    cm.update(torch.from_numpy(logits), torch.from_numpy(target), valid=torch.tensor([2], dtype=torch.int32), pred=pred)
    np.testing.assert_array_equal(cm.counts.numpy(), want)
    np.testing.assert_array_equal(pred.numpy(), want_pred)
    assert want[-1] > 0
    with pytest.raises(ValueError, match="outside"):
        cm.all_metrics()


# ------------------------------------------------------------------------------------------- votes, projection, crop
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "normal"])
def test_composed_votes_equal_the_call_order_statement(exact):
    from adaptpoint_amd.sceneseg import SegMetrics, Votes
    n, C = 65, 13
    case = R.votes_case(n, C, 5, 11, exact)
    want = R.votes(n, C, case)
    labels = np.random.RandomState(1).randint(0, C, n)
    v, cm = Votes(n, C, "cpu"), SegMetrics(C, device="cpu")
    for logits, rows in case:
        v.add(torch.from_numpy(logits), torch.from_numpy(rows))
    pred, mean = v.finish(torch.from_numpy(labels), cm, want_mean=True)
    assert np.array_equal(mean.numpy().view(np.int32), want["mean"].view(np.int32))
    np.testing.assert_array_equal(pred.numpy(), want["pred"])
    np.testing.assert_array_equal(cm.counts.numpy(), R.count(want["pred"], labels, C))
    # a repeated row inside one add, a row outside [0, n): ValueError at finish, every other point as the statement has it
    for bad_rows in ([3, 9, 3], [5, n], [-1, 2]):
        v = Votes(n, C, "cpu")
        extra = (np.ones((C, len(bad_rows)), np.float32), np.array(bad_rows))
        for logits, rows in case + [extra]:
            v.add(torch.from_numpy(logits), torch.from_numpy(rows))
        want_bad = R.votes(n, C, case + [extra])
        assert want_bad["duplicates"] + want_bad["rejected"] == 1
        with pytest.raises(ValueError, match="repeated row|outside"):
            v.finish()
        sure = ~want_bad["unsure"]
        got = (v.acc / v.cnt.clamp(min=1).unsqueeze(1)).numpy()
        assert np.array_equal(got[sure].view(np.int32), want_bad["mean"][sure].view(np.int32))


def test_composed_projection_equals_the_numpy_statement():
    from adaptpoint_amd.sceneseg import SegMetrics, project
    rng = np.random.RandomState(4)
    C, m, n = 13, 70, 500
    logits = (np.round(rng.randn(C, m) * 2) / 2).astype(np.float32)
    slot, voxel_of = rng.permutation(m), rng.randint(0, m, n)
    labels = rng.randint(0, C, n)
    want, rejected = R.project(logits, slot, voxel_of)
    assert rejected == 0
    cm = SegMetrics(C, device="cpu")
    pred = project(torch.from_numpy(logits), torch.from_numpy(slot), torch.from_numpy(voxel_of), torch.from_numpy(labels), cm)
    np.testing.assert_array_equal(pred.numpy(), want)
    np.testing.assert_array_equal(cm.counts.numpy(), R.count(want, labels, C))
    voxel_of[7] = m
    with pytest.raises(ValueError, match="outside"):
        project(torch.from_numpy(logits), torch.from_numpy(slot), torch.from_numpy(voxel_of))


@pytest.mark.parametrize("kind", ["uniform", "lattice"])
def test_composed_crop_equals_the_numpy_statement(kind):
    from adaptpoint_amd.sceneseg import crop_distance, crop_nearest
    make = R.uniform_cloud if kind == "uniform" else R.lattice_cloud
    sizes = [65, 1000, 64]
    coord = np.concatenate([make(s, 20 + i) for i, s in enumerate(sizes)])
    centres = [3, 999, 0]
    d = crop_distance(torch.from_numpy(coord[:65]), torch.from_numpy(coord[3]))
    assert np.array_equal(d.numpy().view(np.int32), R.crop_distance(coord[:65], 3).view(np.int32))
    for k in (1, 24, 63, 64):
        got = crop_nearest(torch.from_numpy(coord), sizes, centres, k)
        assert got.dtype == torch.int32
        np.testing.assert_array_equal(got.numpy(), R.crop(coord, sizes, centres, k))
    with pytest.raises(ValueError, match="pad first"):
        crop_nearest(torch.from_numpy(coord), sizes, centres, 65)
    with pytest.raises(ValueError, match="outside its cloud"):
        crop_nearest(torch.from_numpy(coord), sizes, [65, 0, 0], 8)
    coord[5, 1] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        crop_nearest(torch.from_numpy(coord), sizes, centres, 8)


# --------------------------------------------------------------------------------------------- tester and sampler
class _PointModel(torch.nn.Module):
    """A stand-in network: per-point logits from a fixed linear map of [pos, x] (the merge, not the network, is what
    these tests are about); records what it was fed."""

    def __init__(self, cin, num_classes):
        super().__init__()
        g = torch.Generator().manual_seed(5)
        self.w = torch.nn.Parameter(torch.randn(num_classes, cin + 3, generator=g))
        self.seen = []

    def forward(self, data):
        x = torch.cat([data['pos'].transpose(1, 2), data['x']], 1)
        out = torch.einsum('oc,bcn->bon', self.w, x)
        self.seen.append((data['pos'].clone(), data['x'].clone(), out.clone(), self.training))
        return out


def test_composed_grid_has_voxel_grid_fields():
    from adaptpoint_amd.sceneseg import composed_grid
    coord = torch.tensor([[0.05, 0.0, 0.0], [0.95, 0.0, 0.0], [0.06, 0.01, 0.0], [0.5, 0.5, 0.5], [0.07, 0.0, 0.02]])
    g = composed_grid(coord, 0.1)
    assert g.voxel_of.tolist() == [0, 1, 0, 2, 0] and g.count.tolist() == [3, 1, 1] and g.start.tolist() == [0, 3, 4]
    assert g.idx_sort.tolist() == [0, 2, 4, 1, 3] and (g.m, g.count_max, g.n) == (3, 3, 5)
    assert g.part(1).tolist() == [2, 1, 3] and g.part(2).tolist() == [4, 1, 3]


@pytest.mark.parametrize("ignore", [None, 12])
def test_scene_tester_composed_equals_the_vote_statement(ignore):
    from adaptpoint_amd.sceneseg import SceneTester, composed_grid
    C, n = R.NUM_CLASSES, 700
    coord, feat, label = R.scene(n, 8)
    model = _PointModel(4, C).train()
    tester = SceneTester(model, C, voxel_size=0.1, ignore_index=ignore)
    np.random.seed(3)
    cm = tester(torch.from_numpy(coord), torch.from_numpy(feat), torch.from_numpy(label))
    assert model.training and all(not s[3] for s in model.seen)                 # eval inside, the flag restored
    shifted = torch.from_numpy(coord) - torch.from_numpy(coord).min(0).values
    grid = composed_grid(shifted, 0.1)
    assert len(tester.parts) == grid.count_max > 1 and len(model.seen) == grid.count_max
    # the host stream: one np.random.shuffle of length m per part, in order
    np.random.seed(3)
    for i, rows in enumerate(tester.parts):
        perm = np.arange(grid.m)
        np.random.shuffle(perm)
        np.testing.assert_array_equal(rows.numpy(), grid.part(i).numpy()[perm])
        pos, x, _, _ = model.seen[i]
        want_pos = shifted[rows.long()] - shifted[rows.long()].min(0).values
        assert torch.equal(pos[0], want_pos)
        assert torch.equal(x[0], torch.cat([torch.from_numpy(feat)[rows.long()], want_pos[:, 2:3]], 1).t())   # x, heights
    covered = np.zeros(n, bool)
    covered[np.concatenate([r.numpy() for r in tester.parts])] = True
    assert covered.all()
    want = R.votes(n, C, [(s[2][0].numpy(), rows.numpy()) for s, rows in zip(model.seen, tester.parts)])
    np.testing.assert_array_equal(tester.pred.numpy(), want["pred"])
    np.testing.assert_array_equal(cm.counts.numpy(), R.count(want["pred"], label, C, ignore))
    np.testing.assert_array_equal(tester.total.counts.numpy(), cm.counts.numpy())
    tester(torch.from_numpy(coord), torch.from_numpy(feat), torch.from_numpy(label), draws='device')
    assert int(tester.total.total) == 2 * int(cm.total)
    miou, macc, oa, ious, accs = tester.total.mious()
    assert ious.shape == (C,) and 0.0 <= oa <= 100.0


def test_scene_tester_nearest_neighbour_and_single_part_modes():
    from adaptpoint_amd.sceneseg import SceneTester, composed_grid
    C, n = R.NUM_CLASSES, 500
    coord, feat, label = R.scene(n, 9)
    model = _PointModel(4, C)
    tester = SceneTester(model, C, voxel_size=0.15, mode='nearest_neighbor')
    np.random.seed(6)
    cm = tester(torch.from_numpy(coord), torch.from_numpy(feat), torch.from_numpy(label))
    shifted = torch.from_numpy(coord) - torch.from_numpy(coord).min(0).values
    grid = composed_grid(shifted, 0.15)
    np.random.seed(6)
    pick = np.random.randint(0, grid.count_max, grid.m)
    perm = np.random.permutation(grid.m)
    rows = grid.pick(torch.from_numpy(pick)).numpy()[perm]
    assert len(model.seen) == 1 and np.array_equal(tester.parts[0].numpy(), rows)
    # the reference's statement: all_logits[reverse_idx_part][voxel_idx][reverse_idx].argmax(1)
    all_logits = model.seen[0][2][0].t().numpy()
    idx_sort = grid.idx_sort.numpy()
    voxel_idx = grid.voxel_of.numpy()[idx_sort]
    want = np.argmax(all_logits[np.argsort(perm)][voxel_idx][np.argsort(idx_sort)], 1)
    np.testing.assert_array_equal(tester.pred.numpy(), want)
    np.testing.assert_array_equal(cm.counts.numpy(), R.count(want, label, C))
    # no voxel size: one part, arange(n)
    model.seen.clear()
    single = SceneTester(model, C)
    cm = single(torch.from_numpy(coord), torch.from_numpy(feat), torch.from_numpy(label))
    assert len(model.seen) == 1 and single.parts[0].tolist() == list(range(n))
    want = np.argmax(model.seen[0][2][0].numpy(), 0)
    np.testing.assert_array_equal(single.pred.numpy(), want)
    np.testing.assert_array_equal(cm.counts.numpy(), R.count(want, label, C))


def test_scene_sampler_composed_follows_crop_pc():
    from adaptpoint_amd.sceneseg import SceneSampler, composed_grid
    k = 48
    scenes = [R.scene(600, 12), R.scene(40, 13), R.scene(300, 14)]                 # the second has fewer than k voxels
    tens = [tuple(torch.from_numpy(a) for a in s) for s in scenes]
    sampler = SceneSampler(voxel_size=0.2, voxel_max=k)
    np.random.seed(21)
    out = sampler.batch(tens)
    assert out['pos'].shape == (3, k, 3) and out['x'].shape == (3, 4, k) and out['y'].shape == (3, k)
    assert out['y'].dtype == torch.int64
    np.random.seed(21)                                                             # the reference's calls, in its order
    for s, (coord, feat, label) in enumerate(scenes):
        coord = coord - coord.min(0)
        grid = composed_grid(torch.from_numpy(coord), 0.2)
        pick = np.random.randint(0, grid.count_max, grid.m)
        uniq = grid.pick(torch.from_numpy(pick)).numpy()
        sub = coord[uniq]
        N = len(uniq)
        if N >= k:
            init_idx = np.random.randint(N)
            crop_idx = R.crop(sub, [N], [init_idx], k)[0]
            unstable = np.argsort(np.sum(np.square(sub - sub[init_idx]), 1))[:k]   # crop_pc :159-160: the same set
            assert set(unstable.tolist()) == set(crop_idx.tolist())
        else:
            assert s == 1
            crop_idx = np.hstack([np.arange(N), np.arange(N)[np.random.choice(N, k - N)]])
        crop_idx = crop_idx[np.random.permutation(np.arange(len(crop_idx)))]
        rows = uniq[crop_idx]
        np.testing.assert_array_equal(sampler.rows[s].numpy(), rows)
        pos = coord[rows] - coord[rows].min(0)
        np.testing.assert_array_equal(out['pos'][s].numpy(), pos)
        np.testing.assert_array_equal(out['x'][s].numpy(), np.concatenate([feat[rows], pos[:, 2:3]], 1).T)
        np.testing.assert_array_equal(out['y'][s].numpy(), label[rows])
    a = np.random.rand()
    np.random.seed(21)
    sampler.batch(tens)
    assert np.random.rand() == a                                                   # the same host stream was consumed
    dev = sampler.batch(tens, draws='device')
    assert dev['pos'].shape == (3, k, 3) and float(dev['pos'].min()) == 0.0


def test_seg_step_and_validate_on_the_cpu_stand_in():
    from adaptpoint_amd.sceneseg import SegMetrics, SegStep, SmoothCrossEntropy, validate
    C, B, N = 5, 2, 30
    g = torch.Generator().manual_seed(2)
    data = {'pos': torch.rand(B, N, 3, generator=g), 'x': torch.rand(B, 4, N, generator=g),
            'y': torch.randint(0, C, (B, N), generator=g)}
    data['y'][0, :4] = 255
    model = _PointModel(4, C)
    w0 = model.w.detach().clone()
    cm = SegMetrics(C, 255, device="cpu")
    step = SegStep(model, criterion=SmoothCrossEntropy(0.2, ignore_index=255, num_classes=C), metrics=cm)
    logits, loss = step(data)
    assert not torch.equal(model.w, w0) and model.w.grad is None and not logits.requires_grad and loss.dim() == 0
    want, _ = R.confusion(logits.numpy(), data['y'].numpy(), 255)
    np.testing.assert_array_equal(cm.counts.numpy(), want)
    assert int(cm.total) == B * N - 4
    model.train()
    val = SegMetrics(C, 255, device="cpu")
    res = validate(model, [data, data], val)
    assert model.training and len(res) == 5 and int(val.total) == 2 * (B * N - 4)
    assert list(res[:3]) == list(val.mious()[:3])
