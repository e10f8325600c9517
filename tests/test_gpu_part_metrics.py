"""GPU: apn_part_ious (csrc/part_metrics.hip) and adaptpoint_amd.part_metrics.PartMetrics against the numpy statement of
the metric (tests/partseg_reference.py, itself checked against the reference's get_ins_mious by the golden generator and
tests/test_partseg_cpu.py): the crafted corners, random logits with exact ties at the sizes where the kernel's loops
change, a padded batch, the batch split, rejected shapes, a captured replay, and the entry's argument checks."""
import numpy as np
import pytest
import torch

import partseg_reference as R

pytestmark = pytest.mark.gpu


def _logits_for(pred, C):
    """Logits (B,C,N) whose argmax is `pred`, with a tie on a HIGHER channel wherever there is one (the first wins)."""
    B, N = pred.shape
    x = np.zeros((B, C, N), np.float32)
    b, n = np.meshgrid(np.arange(B), np.arange(N), indexing="ij")
    x[b, pred, n] = 3.0
    x[b, np.minimum(pred + 1, C - 1), n] = 3.0
    return x


def _feed(dev, metrics, logits, target, cls, valid=None):
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(dev)
    return metrics.update(t(logits, torch.float32), t(target, torch.int64), t(cls, torch.int64),
                          None if valid is None else t(valid, torch.int32)).cpu().numpy()


def _state(metrics):
    return (metrics.cls_sum.cpu().numpy(), metrics.cls_num.cpu().numpy(), float(metrics.ins_sum.cpu()[0]),
            int(metrics.counts.cpu()[0]))


def _same_state(a, b):
    return (np.array_equal(a[0].view(np.int32), b[0].view(np.int32)) and np.array_equal(a[1], b[1])
            and np.float64(a[2]).tobytes() == np.float64(b[2]).tobytes() and a[3] == b[3])


def test_crafted_cases_equal_the_numpy_statement(dev):
    from adaptpoint_amd.part_metrics import PartMetrics
    for name, pred, target, cls, table, C in R.crafted_cases():
        m = PartMetrics(table, C, dev)
        got = _feed(dev, m, _logits_for(pred, C), target, cls)
        want = R.shape_ious(pred, target, cls, table)
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), (name, got, want)
        assert _same_state(_state(m), R.totals(want, cls, len(table))), name
    # the closing arithmetic over a table with a category that never occurs: it contributes 0 to the class mean
    name, pred, target, cls, table, C = R.crafted_cases()[3]
    m = PartMetrics(table, C, dev)
    _feed(dev, m, _logits_for(pred, C), target, cls)
    ins, cmean, per = m.result()
    want = R.shape_ious(pred, target, cls, table)
    assert per[2] == 0.0 and np.array_equal(per[[0, 1, 3]], want)
    np.testing.assert_allclose(cmean, want.sum() / 4, rtol=1e-6)
    np.testing.assert_allclose(ins, want.mean(), rtol=1e-6)


@pytest.mark.parametrize("C", [50, 64])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 2048])
@pytest.mark.parametrize("B", [1, 5, 67])
def test_random_logits_with_ties_equal_the_numpy_statement(dev, B, N, C):
    from adaptpoint_amd.part_metrics import PartMetrics
    logits, target, cls, table = R.random_case(B, N, C, seed=B * 10000 + N * 10 + C)
    pred = R.predict(logits)
    assert ((logits == logits.max(1, keepdims=True)).sum(1) > 1).any() or N == 1       # exact ties are present
    m = PartMetrics(table, C, dev)
    got = _feed(dev, m, logits, target, cls)
    want = R.shape_ious(pred, target, cls, table)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    assert _same_state(_state(m), R.totals(want, cls, len(table)))


def test_nan_and_infinite_logits_follow_torch_max(dev):
    """A NaN beats every number and the first NaN wins; an all -inf column gives channel 0: `logits.max(dim=1)[1]`."""
    from adaptpoint_amd.part_metrics import PartMetrics
    logits, target, cls, table = R.random_case(2, 64, 50, seed=77)
    logits[0, 7, 3] = np.nan
    logits[0, 20, 3] = np.nan
    logits[1, :, 5] = -np.inf
    logits[1, 9, 6] = np.inf
    pred = torch.from_numpy(logits).max(dim=1)[1].numpy()
    assert pred[0, 3] == 7 and pred[1, 5] == 0 and pred[1, 6] == 9
    got = _feed(dev, PartMetrics(table, 50, dev), logits, target, cls)
    want = R.shape_ious(pred, target, cls, table)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))


def test_padded_batch_and_batch_split_give_the_same_bits(dev):
    """70 shapes: as one batch, as three uneven ones, and as batches of 32 whose last is padded and masked by `valid`."""
    from adaptpoint_amd.part_metrics import PartMetrics
    logits, target, cls, table = R.random_case(70, 257, 50, seed=5)
    want = R.shape_ious(R.predict(logits), target, cls, table)
    one = PartMetrics(table, 50, dev)
    _feed(dev, one, logits, target, cls)
    three = PartMetrics(table, 50, dev)
    for lo, hi in ((0, 3), (3, 41), (41, 70)):
        _feed(dev, three, logits[lo:hi], target[lo:hi], cls[lo:hi])
    padded = PartMetrics(table, 50, dev)
    for lo in (0, 32, 64):
        rows = np.arange(lo, lo + 32)
        valid = (rows < 70).astype(np.int32)
        rows = np.where(rows < 70, rows, lo)
        got = _feed(dev, padded, logits[rows], target[rows], cls[rows], valid)
        assert np.array_equal(got[valid == 1].view(np.int32), want[rows[valid == 1]].view(np.int32))
        assert (got[valid == 0] == -1.0).all()
    ref = R.totals(want, cls, len(table))
    for m in (one, three, padded):
        assert _same_state(_state(m), ref)
    assert one.result()[0] == three.result()[0] == padded.result()[0]


def test_shapes_outside_the_table_are_rejected_and_counted(dev):
    from adaptpoint_amd.part_metrics import PartMetrics
    logits, target, cls, table = R.random_case(6, 65, 50, seed=9)
    cls = cls.copy()
    cls[1], cls[4] = -1, len(table)
    target = target.copy()
    target[0, :5] = 50                                  # a label outside [0, C): in no part, as in the reference
    target[0, 5:9] = -3
    m = PartMetrics(table, 50, dev)
    got = _feed(dev, m, logits, target, cls)
    keep = np.array([0, 2, 3, 5])
    want = R.shape_ious(R.predict(logits)[keep], target[keep], cls[keep], table)
    assert (got[[1, 4]] == -2.0).all() and np.array_equal(got[keep].view(np.int32), want.view(np.int32))
    assert int(m.counts.cpu()[1]) == 2 and _same_state(_state(m), R.totals(want, cls[keep], len(table)))
    with pytest.raises(ValueError):
        m.result()


def test_update_replayed_from_a_hipgraph_equals_eager(dev):
    from adaptpoint_amd import graphs
    from adaptpoint_amd.part_metrics import PartMetrics
    logits, target, cls, table = R.random_case(5, 130, 50, seed=11)
    t = lambda a, dt: torch.from_numpy(a).to(dt).to(dev)
    lg, tg, cl = t(logits, torch.float32), t(target, torch.int32), t(cls, torch.int32)
    eager = PartMetrics(table, 50, dev)
    e_ious = eager.update(lg, tg, cl).clone()
    m = PartMetrics(table, 50, dev)
    ious = torch.zeros(5, device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m.update(lg, tg, cl, ious=ious)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph, _, census = graphs.capture(lambda: m.update(lg, tg, cl, ious=ious), what="the part metric's graph")
    assert census.get("memset", 0) == 0 and census.get("kernel", 0) >= 2, census
    m.reset()
    ious.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(ious, e_ious) and _same_state(_state(m), _state(eager))
    graph.replay()
    torch.cuda.synchronize()
    eager.update(lg, tg, cl)
    assert _same_state(_state(m), _state(eager))


def test_entry_checks_its_arguments(dev):
    """Host-side checks only: every call returns before a launch."""
    from adaptpoint_amd import _lib
    lib = _lib.load()
    buf = torch.zeros(64, device=dev)
    ibuf = torch.zeros(64, dtype=torch.int32, device=dev)
    p, ip = buf.data_ptr(), ibuf.data_ptr()
    stream = torch.cuda.current_stream(dev).cuda_stream

    def call(b=2, c=4, n=3, s=2, nparts=4, logits=p, target=ip, cls=ip, off=ip, ids=ip, valid=None, ious=p, cs=p, cn=ip,
             isum=p, inum=ip, rej=None):
        return lib.apn_part_ious(b, c, n, s, nparts, logits, target, cls, off, ids, valid, ious, cs, cn, isum, inum, rej, stream)
    EINVAL, OK = -1, 0
    for kw in (dict(b=-1), dict(c=0), dict(c=65), dict(n=-1), dict(s=0), dict(nparts=0), dict(logits=None), dict(target=None),
               dict(cls=None), dict(off=None), dict(ids=None), dict(ious=None), dict(cs=None), dict(cn=None),
               dict(isum=None), dict(inum=None)):
        assert call(**kw) == EINVAL, kw
    assert call(b=0) == OK
    torch.cuda.synchronize()
    assert not buf.any() and not ibuf.any()          # nothing was launched
