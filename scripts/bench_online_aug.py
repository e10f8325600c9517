"""The two online augmenters (adaptpoint_amd.online_aug) at the ScanObjectNN cfgs' parameters, B=32, N=2048, C=4:

  pointwolf      PointWOLF (w_num_anchor 4, sigma 0.5, R 10, S 3, T 0.25; pointnext-s_adaptpoint_1.yaml and
                 pointnext-s_valcorruption_wpointwolf1.yaml) with host draws and with device draws, against the
                 composed PyTorch form of the same arithmetic (the reference's structure: (B,M,N,3) temporaries,
                 CPU draws copied over);
  rsmix          RSMix (beta 1, nsample 512, knn; pointnext-s_valcorruption_wrsmix.yaml) on the device, against the
                 host round trip the reference's trainer makes (batch to numpy, the numpy restatement of
                 tests/online_aug_reference.py, back to the device);
  classifier     one ClassifierStep each way (PointNeXt-S, fused blocks; rsmix_prob 1 so that every step mixes).

    python scripts/bench_online_aug.py [--iters 50] [--warmup 10]

Prints one JSON line per measurement: milliseconds per call, median and mean over --iters calls, each call timed
with a device synchronisation on both sides.
"""
import argparse
import json
import math
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

import online_aug_reference as R
from adaptpoint_amd import augmentor as AUG
from adaptpoint_amd import online_aug as OA
from adaptpoint_amd.gan import ClassifierStep
from adaptpoint_amd.layers import furthest_point_sample
from adaptpoint_amd.pointnext import PointNextSClassifier

B, N, C = 32, 2048, 4


def timed(fn, iters, warm):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), statistics.fmean(ts)


class ComposedPointWOLF(OA.PointWOLF):
    """The same augmenter as elementwise PyTorch over (B,M,N,3) temporaries, its draws made on the host and copied."""

    def __call__(self, xyz, device_draws=False, draws=None):
        Bn, Nn, _ = xyz.shape
        M, dev = self.num_anchor, xyz.device
        keep, code, deg, scale, trl, kcode = (t.to(dev) for t in R.unpack_pointwolf_draws(self.draw_params(Bn), Bn, M))
        bits = torch.arange(3, device=dev)
        axis = ((code.unsqueeze(-1) >> bits) & 1).float()
        kax = ((kcode.unsqueeze(-1) >> bits) & 1).float()
        idx = furthest_point_sample(xyz.contiguous(), M).long()
        a = torch.gather(xyz, 1, idx.unsqueeze(-1).expand(-1, -1, 3))
        ang = math.pi * deg / 180.0 * keep[..., 0:1]
        s = scale * keep[..., 1:2] * axis
        s = s + (s == 0)
        t = trl * keep[..., 2:3] * axis
        sx, sy, sz = torch.sin(ang).unbind(-1)
        cx, cy, cz = torch.cos(ang).unbind(-1)
        rot = torch.stack([cz * cy, cz * sy * sx - sz * cx, cz * sy * cx + sz * sx,
                           sz * cy, sz * sy * sx + cz * cy, sz * sy * cx - cz * sx,
                           -sy, cy * sx, cy * cx], -1).view(Bn, M, 3, 3)
        moved = (xyz.unsqueeze(1) - a.unsqueeze(2)) @ rot @ torch.diag_embed(s) + t.unsqueeze(2) + a.unsqueeze(2)
        w = AUG.kernel_weights(xyz, a, kax, self.sigma)
        z = (w.unsqueeze(-1) * moved).sum(1) / w.sum(1).unsqueeze(-1)
        return xyz, AUG.unit_sphere(z)


def rsmix_host_round_trip(points, label, beta=1.0, n_sample=512, knn=False):
    out, lam, la, lb, _ = R.rsmix_np(points.cpu().numpy(), label.cpu().numpy(), beta, n_sample, knn)
    dev = points.device
    return (torch.from_numpy(out).to(dev), torch.from_numpy(lam).to(dev), torch.from_numpy(la).to(dev),
            torch.from_numpy(lb).to(dev))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--stamp", default=None, help="the commit the figures belong to (default: git's HEAD, if any)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    commit = a.stamp
    if commit is None:
        try:
            commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True,
                                    text=True).stdout.strip() or None
        except OSError:
            pass
    points = torch.from_numpy(R.golden_points(7, B=B, N=N)).to(dev)
    xyz = points[:, :, :3].contiguous()
    label = torch.arange(B, device=dev) % 15

    def emit(name, med, mean, **kw):
        print(json.dumps(dict(bench="online_aug", case=name, B=B, N=N, C=C, ms_median=round(med, 4),
                              ms_mean=round(mean, 4), commit=commit, **kw)), flush=True)

    pw, pwc = OA.PointWOLF(), ComposedPointWOLF()
    emit("pointwolf_host_draws", *timed(lambda: pw(xyz), a.iters, a.warmup))
    emit("pointwolf_device_draws", *timed(lambda: pw(xyz, device_draws=True), a.iters, a.warmup))
    emit("pointwolf_composed_pytorch", *timed(lambda: pwc(xyz), a.iters, a.warmup))
    for knn in (True, False):
        emit("rsmix_device", *timed(lambda: OA.rsmix(points, label, 1.0, 512, knn), a.iters, a.warmup), knn=knn)
        emit("rsmix_host_round_trip", *timed(lambda: rsmix_host_round_trip(points, label, 1.0, 512, knn), a.iters,
                                             a.warmup), knn=knn)

    torch.manual_seed(0)
    model = PointNextSClassifier(fused=True).to(dev)
    rs_cfg = dict(beta=1.0, nsample=512, knn=True, rsmix_prob=1.0)
    steps = [("classifier_step_pointwolf_device", dict(pointwolf=pw), None),
             ("classifier_step_pointwolf_composed", dict(pointwolf=pwc), None),
             ("classifier_step_rsmix_device", dict(rsmix=rs_cfg), None),
             ("classifier_step_rsmix_host_round_trip", dict(rsmix=rs_cfg), rsmix_host_round_trip),
             ("classifier_step_plain", {}, None)]
    device_rsmix = OA.rsmix
    for name, kw, swap in steps:
        OA.rsmix = swap or device_rsmix
        try:
            step = ClassifierStep(model, **kw)
            emit(name, *timed(lambda: step(points.clone(), label), max(10, a.iters // 2), a.warmup))
        finally:
            OA.rsmix = device_rsmix


if __name__ == "__main__":
    main()
