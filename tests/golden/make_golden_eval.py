"""Regenerates tests/golden/eval_golden.npz (run in the BUILD container only):

    python tests/golden/make_golden_eval.py

The reference's own `ConfusionMatrix` (openpoints/utils/metrics.py) and `eval_corrupt_wrapper_scanobjectnnc`
(openpoints/dataset/scanobjectnn_c/scanobjectnn_c.py, loaded from its file so that the dataset package's other loaders
are not imported; make_golden's stubs stand in for h5py) run on CPU, imported in memory through make_golden's stubs;
nothing is copied.

  cm_*      three fixed (pred, true) batches of 64, 64 and 22 rows, K = 15, class ABSENT_CLASS never a target (so that
            count.clamp(min=1) matters): the accumulated `value`, and `cal_acc(tp, count)` = macc, oa, accs
  sweep_*   two seeded tables of the 36 split accuracies (sweep_acc, in split order) with values on rounding edges
            (x.xxx5), and the text lines the wrapper writes for each into outcorruption.txt (epoch header included),
            driven by a stub `fn_test_corrupt` that returns the table's accuracy for the split it is asked for
"""
import importlib.util
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402

OUT = os.path.join(HERE, "eval_golden.npz")
K = 15
ABSENT_CLASS = 7
SIZES = (64, 64, 22)
SPLITS = ['clean'] + [f"{c}_{lv}" for c in ('scale', 'jitter', 'rotate', 'dropout_global', 'dropout_local',
                                              'add_global', 'add_local') for lv in range(5)]


def _ref_wrapper():
    spec = importlib.util.spec_from_file_location(
        "ref_scanobjectnn_c", os.path.join(MG.REF, "openpoints", "dataset", "scanobjectnn_c", "scanobjectnn_c.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.eval_corrupt_wrapper_scanobjectnnc


def confusion_batches():
    rs = np.random.RandomState(1234)
    labels = [c for c in range(K) if c != ABSENT_CLASS]
    pred, true = [], []
    for n in SIZES:
        t = rs.choice(labels, n)
        p = np.where(rs.rand(n) < 0.6, t, rs.randint(0, K, n))       # mostly right; the absent class is predicted too
        true.append(t.astype(np.int64))
        pred.append(p.astype(np.int64))
    return pred, true


def accuracy_tables():
    """Two tables of 36 accuracies: oa / 100 of float32 overall accuracies over 2882 clouds (what
    validate_scanobjectnnc returns), with planted values on a rounding edge of round(., 3)."""
    tables = []
    for seed, planted in ((11, {0: 0.8125, 1: 0.7775, 2: 0.6565, 7: 0.5005, 20: 0.6875, 33: 0.1235}),
                          (12, {0: 0.8435, 5: 0.3125, 9: 0.4445, 16: 0.7005, 26: 0.5555, 35: 0.9995})):
        rs = np.random.RandomState(seed)
        counts = rs.randint(1200, 2600, len(SPLITS))
        acc = [float(torch.tensor(c) / torch.tensor(2882) * 100) / 100 for c in counts]
        for i, v in planted.items():
            acc[i] = v
        tables.append(acc)
    return tables


def wrapper_lines(wrapper, acc, epoch):
    table = dict(zip(SPLITS, acc))

    def fn_test_corrupt(split, model, **kw):
        return {'acc': table[split]}

    with tempfile.TemporaryDirectory() as d:
        wrapper(None, fn_test_corrupt, {}, d, epoch)
        with open(os.path.join(d, 'outcorruption.txt')) as fh:
            return fh.read().splitlines()


def main():
    MG.import_reference()
    sys.path.insert(0, MG.REF)
    from openpoints.utils.metrics import ConfusionMatrix
    out = {}
    pred, true = confusion_batches()
    cm = ConfusionMatrix(num_classes=K)
    for p, t in zip(pred, true):
        cm.update(torch.from_numpy(p), torch.from_numpy(t))
    macc, oa, accs = cm.cal_acc(cm.tp, cm.count)
    out.update(cm_pred=np.concatenate(pred), cm_true=np.concatenate(true), cm_sizes=np.array(SIZES),
               cm_value=cm.value.numpy(), cm_macc=np.float64(macc), cm_oa=np.float64(oa), cm_accs=accs,
               cm_absent=np.int64(ABSENT_CLASS))
    assert int(cm.count[ABSENT_CLASS]) == 0
    wrapper = _ref_wrapper()
    tables = accuracy_tables()
    out['sweep_acc'] = np.array(tables, np.float64)
    out['sweep_splits'] = np.array(SPLITS)
    for i, acc in enumerate(tables):
        lines = wrapper_lines(wrapper, acc, epoch=9 + 10 * i)
        out[f'sweep_lines_{i}'] = np.array(lines)
        print("\n".join(lines[:3] + ["..."] + lines[-3:]))
    np.savez_compressed(OUT, **out)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
