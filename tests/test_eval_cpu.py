"""CPU: the host side of adaptpoint_amd.evaluate -- the corruption sweep's arithmetic and the metric formulas against the
reference's own outputs (tests/golden/eval_golden.npz, tests/golden/make_golden_eval.py), the distributed index order
against torch's DistributedSampler, and the batch plan."""
import os

import numpy as np
import pytest
import torch

from adaptpoint_amd import evaluate as E

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_golden.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


@pytest.mark.parametrize("table", [0, 1])
def test_corruption_summary_reproduces_the_wrappers_lines(gold, table):
    names = [str(s) for s in gold["sweep_splits"]]
    assert names == E.split_names()
    acc = dict(zip(names, gold["sweep_acc"][table].tolist()))
    records, summary = E.corruption_summary(acc)
    lines = [str(s) for s in gold[f"sweep_lines_{table}"]]
    assert lines[0].startswith("epoch: ")
    ours = [f"{r} " for r in records] + [f"{summary} "]
    assert ours == lines[1:]
    assert len(records) == 36 + 8
    assert list(summary) == ['mCE', 'RmCE', 'mOA']


def test_corruption_summary_needs_every_split():
    acc = {s: 0.5 for s in E.split_names()[:-1]}
    with pytest.raises(KeyError):
        E.corruption_summary(acc)


def test_cal_acc_on_cpu_equals_the_reference(gold):
    K = 15
    value = np.zeros((K, K), np.int64)
    np.add.at(value, (gold["cm_true"], gold["cm_pred"]), 1)
    assert np.array_equal(value, gold["cm_value"])
    assert value.sum(1)[int(gold["cm_absent"])] == 0
    cm = E.ConfusionMatrix(K, "cpu")
    cm.counts[:K * K] = torch.from_numpy(value.reshape(-1))
    macc, oa, accs = cm.cal_acc(cm.tp, cm.count)
    assert macc == float(gold["cm_macc"]) and oa == float(gold["cm_oa"])
    assert accs.dtype == gold["cm_accs"].dtype and np.array_equal(accs, gold["cm_accs"])
    assert cm.all_acc()[1] == oa
    assert int(cm.total) == value.sum() and torch.equal(cm.overall_accuray, cm.tp.sum() / cm.total)


def test_all_acc_raises_on_rejected_labels():
    cm = E.ConfusionMatrix(15, "cpu")
    cm.counts[0] = 5
    cm.counts[-1] = 3
    with pytest.raises(ValueError, match="3 counted row"):
        cm.all_acc()
    cm.reset()
    assert int(cm.counts.sum()) == 0


@pytest.mark.parametrize("S", [1, 63, 64, 65, 2882])
@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_distributed_indices_match_distributed_sampler(S, world):
    from torch.utils.data import DistributedSampler
    for rank in range(world):
        ref = list(DistributedSampler(range(S), num_replicas=world, rank=rank, shuffle=False))
        assert E.distributed_indices(S, world, rank) == ref


@pytest.mark.parametrize("S,batches,last", [(1, 1, 1), (64, 1, 64), (65, 2, 1), (2882, 46, 2)])
def test_batch_plan(S, batches, last):
    B = 64
    rows, valid = E.batch_plan(range(S), B)
    assert rows.shape == (batches, B) and valid.shape == (batches,)
    assert valid[:-1].tolist() == [B] * (batches - 1) and valid[-1] == last
    assert rows.reshape(-1)[:S].tolist() == list(range(S))
    lo = (batches - 1) * B
    assert (rows[-1, last:] == lo).all(), "the last batch is padded with copies of its first row"
