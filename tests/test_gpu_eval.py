"""GPU: adaptpoint_amd.evaluate -- apn_cls_confusion (csrc/cls_metrics.hip) against torch.argmax + torch.bincount, the
captured Evaluator against the eager one, the padded last batch against the reference's unpadded loop, a captured graph
across a weight update, sharded validation, and the ScanObjectNN-C sweep."""
import os

import numpy as np
import pytest
import torch

from adaptpoint_amd import evaluate as E

pytestmark = pytest.mark.gpu
K = 15
B = 64
VAL = ['PointsToTensor', 'PointCloudCenterAndNormalize']
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_golden.npz")


def _classifier(dev):
    from adaptpoint_amd.pointnext import PointNextSClassifier, fill_parameters_by_name
    return fill_parameters_by_name(PointNextSClassifier(num_classes=K, fused=True)).to(dev)


def _transform():
    from adaptpoint_amd.transforms import CloudTransform
    return CloudTransform(VAL, 'val', gravity_dim=1)


def _split(dev, S, n_raw, seed):
    from adaptpoint_amd.synthetic import unit_sphere_cloud
    pts = torch.from_numpy(unit_sphere_cloud(S, n_raw, seed)).to(dev)
    lab = torch.randint(0, K, (S,), generator=torch.Generator().manual_seed(seed)).to(dev)
    return pts, lab


@pytest.fixture(scope="module")
def model(dev):
    return _classifier(dev)


@pytest.fixture(scope="module")
def split150(dev):
    return _split(dev, 150, 1024, 31)


def _identity(n, dev):
    p = torch.zeros(n, 12)
    p[:, :3] = 1
    p[:, 3:] = torch.eye(3).reshape(-1)
    return p.to(dev)


@torch.no_grad()
def reference_loop(model, points, labels, order, batch=B, num_points=1024, in_channels=4):
    """validate's structure (train_autoaug.py:528-549) on the device: unpadded batches of `order`, the transform,
    model(data), logits.argmax(dim=1) and the reference's bincount ConfusionMatrix (metrics.py:62-73), restated."""
    model.eval()
    tf = _transform()
    value = torch.zeros(K, K, dtype=torch.int64, device=points.device)
    preds, logits_all = [], []
    for lo in range(0, len(order), batch):
        rows = torch.tensor(order[lo:lo + batch], device=points.device)
        x = tf(points, rows, draws=(None, _identity(rows.numel(), points.device)))[:, :num_points]
        logits = model({'pos': x[:, :, :3].contiguous(), 'x': x[:, :, :in_channels].transpose(1, 2).contiguous()})
        pred, target = logits.argmax(dim=1), labels[rows]
        value += torch.bincount(target * K + pred, minlength=K * K).view(K, K)
        preds.append(pred)
        logits_all.append(logits)
    return value, torch.cat(preds), torch.cat(logits_all)


# --------------------------------------------------------------------------------------------------------- kernel
def _planted_logits(b, k, seed, dev):
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(b, k + 7, generator=g)
    lg = base[:, 3:3 + k]                                           # strided rows: ld = k + 7
    for r in range(b):
        kind = r % 7
        if kind == 1:                                               # a tie at the maximum: the first index wins
            i, j = sorted(torch.randperm(k, generator=g)[:2].tolist())
            lg[r, i] = lg[r, j] = lg[r].max() + 1
        elif kind == 2 and k > 2:                                   # NaNs beat every number; the first NaN wins
            i, j = sorted(torch.randperm(k, generator=g)[:2].tolist())
            lg[r, 0] = float('inf')
            lg[r, j] = float('nan')
            lg[r, i] = float('nan')
        elif kind == 3:                                             # +inf twice
            lg[r, k - 1] = lg[r, k // 2] = float('inf')
        elif kind == 4:                                             # all -inf: 0
            lg[r] = float('-inf')
        elif kind == 5:                                             # -inf around one finite value
            lg[r] = float('-inf')
            lg[r, k // 3] = -1e30
    return base.to(dev)[:, 3:3 + k]


@pytest.mark.parametrize("b", [1, 64, 1000])
@pytest.mark.parametrize("k", [15, 40, 100])
def test_confusion_kernel_matches_torch(dev, b, k):
    logits = _planted_logits(b, k, 1000 * b + k, dev)
    assert logits.stride(0) == k + 7
    g = torch.Generator().manual_seed(b + k)
    target = torch.randint(0, k, (b,), generator=g)
    if b > 2:
        target[1], target[b // 2] = -1, k                           # two labels the reject cell takes
    target = target.to(dev)
    nvalid = b if b < 3 else b - b // 3
    valid = torch.tensor([nvalid], dtype=torch.int32, device=dev)
    runs = []
    for _ in range(2):
        cm = E.ConfusionMatrix(k, dev)
        pred = torch.full((b,), -7, dtype=torch.int32, device=dev)
        cm.update(logits, target, valid=valid, pred=pred)
        runs.append((cm, pred))
    cm, pred = runs[0]
    assert torch.equal(cm.counts, runs[1][0].counts) and torch.equal(pred, runs[1][1])
    ref_pred = torch.argmax(logits.cpu(), dim=1)
    assert torch.equal(pred.cpu().long(), ref_pred), "pred == torch.argmax on every row"
    print(f"b={b} k={k}: device torch.argmax agrees: {torch.equal(torch.argmax(logits, 1).cpu(), ref_pred)}")
    t, p = target.cpu()[:nvalid], ref_pred[:nvalid]
    ok = (t >= 0) & (t < k)
    expect = torch.bincount(t[ok] * k + p[ok], minlength=k * k)
    assert torch.equal(cm.value.reshape(-1).cpu(), expect)
    assert int(cm.rejected) == int((~ok).sum())
    if int((~ok).sum()):
        with pytest.raises(ValueError, match="outside"):
            cm.all_acc()
    # without valid: every row counts; int32 targets; the counters add up
    cm2 = E.ConfusionMatrix(k, dev)
    cm2.update(logits, target.to(torch.int32))
    cm2.update(logits.contiguous(), target)
    okb = (target.cpu() >= 0) & (target.cpu() < k)
    assert int(cm2.value.sum()) == 2 * int(okb.sum()) and int(cm2.rejected) == 2 * int((~okb).sum())


def test_confusion_kernel_limits_and_golden(dev):
    from adaptpoint_amd._lib import load
    lib = load()
    z = torch.zeros(K * K + 1, dtype=torch.int64, device=dev)
    lg = torch.zeros(4, K, device=dev)
    t = torch.zeros(4, dtype=torch.int32, device=dev)
    s = torch.cuda.current_stream(dev).cuda_stream
    for args in ((-1, K, lg.data_ptr(), K), (4, 0, lg.data_ptr(), K), (4, K, lg.data_ptr(), K - 1), (4, K, None, K)):
        assert lib.apn_cls_confusion(*args, t.data_ptr(), None, z.data_ptr(), None, s) == -1
    assert lib.apn_cls_confusion(0, K, None, K, None, None, None, None, s) == 0
    torch.cuda.synchronize()
    assert int(z.sum()) == 0
    # the reference's ConfusionMatrix over the golden batches (one-hot logits: argmax = pred), valid masks nothing extra
    gold = np.load(GOLDEN)
    cm = E.ConfusionMatrix(K, dev)
    lo = 0
    for n in gold["cm_sizes"]:
        pred = torch.from_numpy(gold["cm_pred"][lo:lo + n]).to(dev)
        onehot = torch.nn.functional.one_hot(pred, K).float()
        pad = torch.cat([onehot, onehot[:1].expand(B - n, K)]) if n < B else onehot
        tgt = torch.from_numpy(gold["cm_true"][lo:lo + n]).to(dev)
        tgt = torch.cat([tgt, tgt[:1].expand(B - n)]) if n < B else tgt
        cm.update(pad, tgt, valid=torch.tensor([n], dtype=torch.int32, device=dev))
        lo += n
    assert np.array_equal(cm.value.cpu().numpy(), gold["cm_value"])
    macc, oa, accs = cm.all_acc()
    assert oa == float(gold["cm_oa"]) and np.array_equal(accs, gold["cm_accs"])
    # mAcc is a float32 mean: the device's reduction order may differ from the host's by one ulp
    assert abs(np.float32(macc) - np.float32(gold["cm_macc"])) <= np.spacing(np.float32(gold["cm_macc"]))


# ------------------------------------------------------------------------------------------------------ evaluator
def test_captured_validate_equals_eager(dev, model, split150):
    points, labels = split150
    model.train()
    res = {}
    for capture in (True, False):
        ev = E.Evaluator(model, _transform(), batch_size=B, capture=capture, keep_pred=True)
        res[capture] = ev.validate(points, labels), ev.pred.clone()
        assert model.training, "the model's training flag is restored"
        if capture:
            assert ev.captures == 1 and list(ev.graphs) == [(B, 1024)]
            census = ev.graphs[(B, 1024)].census
            print("evaluation batch graph:", census)
    (macc_c, oa_c, accs_c, cm_c), pred_c = res[True]
    (macc_e, oa_e, accs_e, cm_e), pred_e = res[False]
    assert pred_c.shape == (3, B)
    assert torch.equal(cm_c.counts, cm_e.counts) and torch.equal(pred_c, pred_e)
    assert (macc_c, oa_c) == (macc_e, oa_e) and np.array_equal(accs_c, accs_e)
    assert int(cm_c.value.sum()) == 150 and int(cm_c.rejected) == 0


def test_padding_is_sound(dev, model, split150):
    points, labels = split150
    S = points.shape[0]
    ev = E.Evaluator(model, _transform(), batch_size=B, capture=False, keep_pred=True)
    _, _, _, cm = ev.validate(points, labels)
    value, ref_pred, ref_logits = reference_loop(model, points, labels, list(range(S)))
    pred = ev.pred.reshape(-1)[:S].long()
    # the encoder features of the last batch's valid rows, padded (64 rows) and unpadded (22)
    tf = _transform()
    model.eval()
    last = torch.arange(128, S, device=dev)
    padded = torch.cat([last, last[:1].expand(B - last.numel())])
    feats = []
    with torch.no_grad():
        for rows in (padded, last):
            x = tf(points, rows, draws=(None, _identity(rows.numel(), dev)))
            feats.append(model.encoder.forward_cls_feat({'pos': x[:, :, :3].contiguous(),
                                                          'x': x.transpose(1, 2).contiguous()}))
    identical = torch.equal(feats[0][:last.numel()], feats[1])
    print(f"encoder features of the valid rows bit-identical padded vs unpadded: {identical} "
          f"(max |diff| {(feats[0][:last.numel()] - feats[1]).abs().max().item():.3e})")
    assert identical
    top2 = ref_logits.topk(2, dim=1).values
    clear = (top2[:, 0] - top2[:, 1]) > 1e-4
    assert clear.float().mean().item() >= 0.95
    assert torch.equal(pred[clear], ref_pred[clear])
    if bool(clear.all()):
        assert torch.equal(cm.value, value)


def test_captured_graph_sees_weight_updates(dev):
    from adaptpoint_amd.gan import ClassifierStep
    points, labels = _split(dev, 150, 1024, 32)
    model = _classifier(dev)
    ev = E.Evaluator(model, _transform(), batch_size=B, capture=True, keep_pred=True)
    _, _, _, cm1 = ev.validate(points, labels)
    pred1 = ev.pred.clone()
    step = ClassifierStep(model, lr=0.05)
    x = _transform()(points, torch.arange(32, device=dev))
    step(x, labels[:32])
    torch.cuda.synchronize()
    _, oa2, _, cm2 = ev.validate(points, labels)
    pred2 = ev.pred.clone()
    assert ev.captures == 1, "the same captured graph"
    fresh = E.Evaluator(model, _transform(), batch_size=B, capture=False, keep_pred=True)
    _, oa3, _, cm3 = fresh.validate(points, labels)
    assert not torch.equal(pred1, pred2), "the step changed some prediction (else this test shows nothing)"
    assert torch.equal(pred2, fresh.pred) and torch.equal(cm2.counts, cm3.counts) and oa2 == oa3


def test_shards_sum_to_the_whole(dev, model, split150):
    points, labels = split150[0][:149], split150[1][:149]
    ev = E.Evaluator(model, _transform(), batch_size=B, capture=True)
    total = torch.zeros(K * K + 1, dtype=torch.int64, device=dev)
    for rank in range(2):
        _, _, _, cm = ev.validate(points, labels, rank=rank, world=2)
        total += cm.counts
    padded = E.distributed_indices(149, 1, 0) + [0]              # DistributedSampler pads 149 to 150 by wrapping
    assert sorted(padded) == sorted(E.distributed_indices(149, 2, 0) + E.distributed_indices(149, 2, 1))
    eager = E.Evaluator(model, _transform(), batch_size=B, capture=False)
    with torch.no_grad():
        model.eval()
        whole = eager._run(points, labels, padded)
    assert torch.equal(total, whole.counts)
    assert int(total[:-1].sum()) == 150


def test_corruption_sweep(dev, model):
    from adaptpoint_amd import graphs
    Bs = 16
    splits = {}
    for i, name in enumerate(E.split_names()):
        splits[name] = _split(dev, 40, 2048 if i % 2 == 0 else 1536, 100 + i)
    ev = E.Evaluator(model, _transform(), batch_size=Bs, capture=True)
    records, summary = ev.corruption_sweep(splits)
    assert ev.captures == 2 and sorted(ev.graphs) == [(Bs, 1536), (Bs, 2048)]
    for st in ev.graphs.values():
        graphs.assert_replayable(st.graph)
        assert graphs.is_chain(st.graph), "single stream, no parallel branches"
    eager = E.Evaluator(model, _transform(), batch_size=Bs, capture=False)
    acc = {}
    for name in E.split_names():
        acc[name] = eager.validate(*splits[name])[1] / 100
    per_level = [r for r in records if 'acc' in r]
    assert [r['acc'] for r in per_level] == [acc[n] for n in E.split_names()]
    assert (records, summary) == E.corruption_summary(acc)
