"""The evaluation half of an epoch (adaptpoint_amd.evaluate): validate and the ScanObjectNN-C sweep, fused PointNeXt-S
with name-seeded weights over synthetic clouds (synthetic.unit_sphere_cloud, seeded labels), B = 64.

Cases:
  val        S = 2882, N = 1024                 validate (train_autoaug.py:528-549)
  c_split    S = 2882, N_raw = 2048 -> 1024     one ScanObjectNN-C split (validate_scanobjectnnc, :551-574)
  sweep      36 such splits, each uploaded from the host one at a time (upload time reported on its own)
Legs:
  captured   Evaluator(capture=True): per batch one device-to-device copy of the row block + one graph replay
  eager      Evaluator(capture=False): the same body launched op by op
  reference  the reference's per-batch structure on the device: the transform call, model(data), logits.argmax(1) and
             a bincount ConfusionMatrix (metrics.py:62-73, restated below) that reads the host once per batch

    python scripts/bench_eval.py [--repeats 5] [--out profiles/eval_bench.jsonl] [--stamp <commit>]

Every timed region ends in a device synchronise and is measured with the host clock; each shape is warmed first; the
figure is the median of --repeats runs.  One JSON line per measurement, also written to --out.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from adaptpoint_amd import evaluate as E
from adaptpoint_amd.pointnext import PointNextSClassifier, fill_parameters_by_name
from adaptpoint_amd.synthetic import unit_sphere_cloud
from adaptpoint_amd.transforms import CloudTransform

K, B, S = 15, 64, 2882
VAL = ['PointsToTensor', 'PointCloudCenterAndNormalize']


class BincountConfusionMatrix:
    """openpoints/utils/metrics.py:51-73 restated (no ignore_index): a bincount per update, which reads the host to size
    its output."""

    def __init__(self, num_classes):
        self.value, self.num_classes = 0, num_classes

    @torch.no_grad()
    def update(self, pred, true):
        k = self.num_classes
        bins = torch.bincount(true.flatten() * k + pred.flatten(), minlength=k ** 2)
        self.value += bins.view(k, k)[:k, :k]


@torch.no_grad()
def reference_leg(model, tf, points, labels, batch=B, num_points=1024, in_channels=4):
    model.eval()
    cm = BincountConfusionMatrix(K)
    ident = torch.zeros(batch, 12, device=points.device)
    ident[:, :3] = 1
    ident[:, 3:] = torch.eye(3, device=points.device).reshape(-1)
    n = points.shape[0]
    for lo in range(0, n, batch):
        rows = torch.arange(lo, min(lo + batch, n), device=points.device)
        x = tf(points, rows, draws=(None, ident[:rows.numel()]))[:, :num_points]
        logits = model({'pos': x[:, :, :3].contiguous(), 'x': x[:, :, :in_channels].transpose(1, 2).contiguous()})
        cm.update(logits.argmax(dim=1), labels[rows])
    tp, count = cm.value.diag(), cm.value.sum(dim=1)
    return tp.sum().item() / count.sum().item() * 100


def timed(fn, repeats):
    fn()                                   # warm the shape
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_bench.jsonl"))
    ap.add_argument("--stamp", default=None, help="the commit to record (default: git rev-parse HEAD)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    commit = args.stamp
    if commit is None:
        try:
            commit = subprocess.check_output(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, text=True,
                                             stderr=subprocess.DEVNULL).strip()
        except Exception:
            commit = "unknown"
    lines = []

    def emit(**kw):
        line = json.dumps({"bench": "eval", **kw, "commit": commit})
        print(line, flush=True)
        lines.append(line)

    model = fill_parameters_by_name(PointNextSClassifier(num_classes=K, fused=True)).to(dev)
    tf = CloudTransform(VAL, 'val', gravity_dim=1)
    labels = torch.randint(0, K, (S,), generator=torch.Generator().manual_seed(5)).to(dev)
    nb = -(-S // B)
    evs = {leg: E.Evaluator(model, tf, batch_size=B, capture=(leg == "captured")) for leg in ("captured", "eager")}

    for case, n_raw, seed in (("val", 1024, 41), ("c_split", 2048, 42)):
        points = torch.from_numpy(unit_sphere_cloud(S, n_raw, seed)).to(dev)
        oas = {}
        for leg in ("captured", "eager", "reference"):
            before = torch.cuda.memory_reserved(dev)
            if leg == "reference":
                fn = lambda: oas.__setitem__(leg, reference_leg(model, tf, points, labels))       # noqa: E731
            else:
                fn = lambda: oas.__setitem__(leg, evs[leg].validate(points, labels)[1])            # noqa: E731
            med, best = timed(fn, args.repeats)
            extra = {}
            if leg == "captured":
                st = evs[leg].graphs[(B, n_raw)]
                extra = dict(kernel_nodes_per_batch=st.census.get("kernel", 0), graph_nodes=sum(st.census.values()),
                             census=st.census, reserved_mb_after_capture=round(
                                 (torch.cuda.memory_reserved(dev) - before) / 2 ** 20, 1),
                             static_buffers_mb=round(sum(t.numel() * t.element_size() for t in (
                                 st.raw, st.labels, st.batch, st.counts, st.pred)) / 2 ** 20, 1))
            emit(case=case, leg=leg, S=S, N_raw=n_raw, N=1024, B=B, batches=nb, s_median=round(med, 4),
                 s_min=round(best, 4), ms_per_batch=round(med * 1e3 / nb, 4), clouds_per_s=round(S / med, 1),
                 oa=round(oas[leg], 4), **extra)
        del points

    # the sweep: 36 splits uploaded one at a time from host arrays (four distinct ones, reused), each evaluated
    hosts = [unit_sphere_cloud(S, 2048, 60 + i) for i in range(4)]
    names = E.split_names()

    def sweep(leg):
        up = ev_s = 0.0
        acc = {}
        for i, name in enumerate(names):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            points = torch.from_numpy(hosts[i % 4]).to(dev)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if leg == "reference":
                oa = reference_leg(model, tf, points, labels)
            else:
                oa = evs[leg].validate(points, labels)[1]
            torch.cuda.synchronize()
            acc[name] = oa / 100
            up += t1 - t0
            ev_s += time.perf_counter() - t1
            del points
        E.corruption_summary(acc)
        return up, ev_s

    for leg in ("captured", "eager", "reference"):
        sweep(leg)                                                 # warm
        runs = [sweep(leg) for _ in range(args.repeats)]
        ups, evals = [r[0] for r in runs], [r[1] for r in runs]
        emit(case="sweep", leg=leg, splits=len(names), S=S, N_raw=2048, N=1024, B=B,
             sweep_s_median=round(statistics.median(evals), 3), upload_s_median=round(statistics.median(ups), 3),
             clouds_per_s=round(len(names) * S / statistics.median(evals), 1),
             ms_per_batch=round(statistics.median(evals) * 1e3 / (len(names) * nb), 4))
    emit(case="graphs", captures=evs["captured"].captures, keys=[list(k) for k in evs["captured"].graphs],
         device=torch.cuda.get_device_name(dev))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
