"""The ScanObjectNN dataset transforms (adaptpoint_amd.transforms) with the train chain of cfgs/scanobjectnn/default.yaml
(shuffle, scale [0.9, 1.1], centre and normalise, rotation about y, heights), B in {32, 64}, N in {1024, 2048}:

  transform_host_draws     the reference's draws on the host (draw_params, sample by sample) + copy + one launch
  transform_device_draws   the draws from the device generator + one launch (capturable)
  classifier_step          one ClassifierStep (PointNeXt-S, fused blocks, B=32, N=2048 -> 1024), on a prepared batch
                           and with the device-draw transform in front of it
  cpu_restatement          context: the per-sample CPU cost of the same chain on one host thread, an own restatement
                           (numpy row shuffle, torch scale / centre / normalise / rotate, heights), NOT the reference

    python scripts/bench_transforms.py [--blocks 20] [--per-block 10] [--warmup 10]

Device times are HIP events around blocks of --per-block calls; the figure is the median over --blocks blocks of the
per-call time (the host-draw figure therefore includes the host's draws, which the device waits for).  One JSON line
per measurement.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

from adaptpoint_amd.transforms import build_transforms_from_cfg, axis_rotation

DT = {'train': ['PointsToTensor', 'PointCloudScaling', 'PointCloudCenterAndNormalize', 'PointCloudRotation'],
      'kwargs': {'scale': [0.9, 1.1], 'angle': [0.0, 1.0, 0.0], 'gravity_dim': 1}}


def event_ms(fn, blocks, per_block, warm):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(blocks):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(per_block):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / per_block)
    return statistics.median(ts), statistics.fmean(ts)


def cpu_restatement_ms(n, samples=200):
    """Own per-sample restatement of the train chain on one thread (not the reference's code)."""
    torch.set_num_threads(1)
    rs = np.random.RandomState(0)
    store = rs.randn(samples, n, 3).astype(np.float32)
    t0 = time.perf_counter()
    for i in range(samples):
        cp = store[i]
        np.random.shuffle(cp)
        pos = torch.from_numpy(np.array(cp))
        pos = pos * (torch.rand(3) * 0.2 + 0.9)
        h = pos[:, 1:2] - pos[:, 1:2].min()
        pos = pos - pos.mean(0, keepdim=True)
        pos = pos / torch.sqrt((pos ** 2).sum(-1)).max()
        mats = [axis_rotation(a, np.random.uniform(-b, b)) for a, b in enumerate((0.0, np.pi, 0.0))]
        np.random.shuffle(mats)
        rot = torch.tensor(mats[0] @ mats[1] @ mats[2], dtype=torch.float32)
        torch.cat([pos @ rot.T, h], 1)
    return (time.perf_counter() - t0) * 1e3 / samples


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=20)
    ap.add_argument("--per-block", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    try:
        commit = subprocess.check_output(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, text=True).strip()
    except Exception:
        commit = "unknown"

    def emit(**kw):
        print(json.dumps({"bench": "transforms", **kw, "commit": commit}), flush=True)

    S = 256
    raw = torch.randn(S, 2048, 3, device=dev) * 0.4
    np.random.seed(0)
    torch.manual_seed(0)
    for Bn in (32, 64):
        for n in (1024, 2048):
            tf = build_transforms_from_cfg('train', DT, num_points=n)
            rows = torch.randperm(S, device=dev)[:Bn]
            for mode, dd in (("transform_host_draws", False), ("transform_device_draws", True)):
                med, mean = event_ms(lambda: tf(raw, rows, device_draws=dd), args.blocks, args.per_block, args.warmup)
                emit(case=mode, B=Bn, N=n, ms_median=round(med, 4), ms_mean=round(mean, 4))

    from adaptpoint_amd.gan import ClassifierStep
    from adaptpoint_amd.pointnext import PointNextSClassifier
    Bn, n = 32, 2048
    model = PointNextSClassifier(fused=True).to(dev)
    step = ClassifierStep(model)
    tf = build_transforms_from_cfg('train', DT, num_points=n)
    rows = torch.randperm(S, device=dev)[:Bn]
    target = torch.randint(0, 15, (Bn,), device=dev)
    prepared = tf(raw, rows, device_draws=True)
    choice = torch.from_numpy(np.random.choice(1200, 1024, False).astype(np.int32)).to(dev)
    for case, fn in (("classifier_step", lambda: step(prepared.clone(), target, choice=choice)),
                     ("classifier_step_with_transform",
                      lambda: step(tf(raw, rows, device_draws=True), target, choice=choice))):
        med, mean = event_ms(fn, args.blocks, max(1, args.per_block // 2), args.warmup)
        emit(case=case, B=Bn, N=n, ms_median=round(med, 4), ms_mean=round(mean, 4))
    for n in (1024, 2048):
        emit(case="cpu_restatement_per_sample", N=n, ms_per_sample=round(cpu_restatement_ms(n), 4),
             note="own restatement on one host thread, not the reference's code")


if __name__ == "__main__":
    main()
