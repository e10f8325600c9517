"""The scene-segmentation kernels (csrc/scene_seg.hip through `adaptpoint_amd.sceneseg`) against the composed torch form
of the same commit, alternating in ONE process (the method of scripts/bench_voxel_grid.py):

  * confusion at (32, 13, 24000): the kernel replayed from a hipGraph and eager, against `argmax(1)` + `bincount` (eager:
    bincount reads its output size on the host and cannot be captured);
  * the vote merge of a 10^6-point scene at voxel 0.04 (count_max `add`s + `finish`, the flags' host read included),
    against `index_add_` + divide + `argmax` + `bincount`;
  * `crop_nearest` at 32 clouds of 3 * 10^5 rows with k = 24000 (its stats' host read included), against
    `torch.topk(largest=False)` per cloud on the device and numpy's `argsort` on the host;
  * with --e2e: one `SegStep` (B x 24000 points) and one `SceneTester` scene with PointNeXt-S, kernels against composed.

    python scripts/bench_scene_seg.py [--blocks 5] [--steps 50] [--warmup 3] [--e2e] [--out profiles/scene_seg.jsonl]

One JSON line per case: the median (and min / max) over `--blocks` alternating blocks of `--steps` calls, or fewer for a
slow form (about 0.3 s per block, at least 1 call), recorded as `<form>_steps`.  Results are checked equal before timing.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from adaptpoint_amd import graphs, sceneseg
from adaptpoint_amd.voxel_grid import voxel_grid


def time_forms(forms, a, host=()):
    """{name_us: median us per call}: alternating blocks, a device synchronise inside every timed window."""
    res, steps = {}, {}
    for k, fn in forms.items():
        for _ in range(1 if k in host else a.warmup):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        steps[k] = max(1, min(a.steps, int(0.3 / max(time.perf_counter() - t0, 1e-6))))
    times = {k: [] for k in forms}
    for _ in range(a.blocks):
        for k, fn in forms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps[k]):
                fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e6 / steps[k])
    for k, t in times.items():
        t = sorted(t)
        res[k + "_us"] = round(t[len(t) // 2], 1)
        res[k + "_us_min_max"] = [round(t[0], 1), round(t[-1], 1)]
        res[k + "_steps"] = steps[k]
    return res


def bench_confusion(dev, a):
    B, C, N = 32, 13, 24000
    g = torch.Generator().manual_seed(1)
    logits = torch.randn(B, C, N, generator=g).to(dev)
    target = torch.randint(0, C, (B, N), generator=g).to(dev)
    target32 = target.to(torch.int32)
    cm = sceneseg.SegMetrics(C, device=dev)
    cm.update(logits, target32)
    want = torch.bincount((target * C + logits.argmax(1)).flatten(), minlength=C * C)
    equal = bool(torch.equal(cm.counts[:-1], want))
    torch.cuda.synchronize()
    graph, _, _ = graphs.capture(lambda: cm.update(logits, target32), what="the confusion update")
    res = dict(op="confusion", shape=[B, C, N], equal=equal)
    res.update(time_forms({"kernel_graph": graph.replay, "kernel_eager": lambda: cm.update(logits, target32),
                           "composed": lambda: torch.bincount((target * C + logits.argmax(1)).flatten(), minlength=C * C)}, a))
    res["against_composed"] = round(res["composed_us"] / res["kernel_graph_us"], 2)
    return res


def bench_votes(dev, a):
    n, C, voxel = 1000000, 13, 0.04
    rng = np.random.default_rng(2)
    coord = torch.from_numpy((rng.uniform(0, 1, (n, 3)) * np.array([8.0, 6.0, 3.0])).astype(np.float32)).to(dev)
    labels = torch.from_numpy(rng.integers(0, C, n)).to(dev)
    grid = voxel_grid(coord, voxel)
    g = torch.Generator().manual_seed(3)
    parts = [(torch.randn(C, grid.m, generator=g).to(dev), grid.part(i).contiguous()) for i in range(grid.count_max)]
    labels32 = labels.to(torch.int32)

    def kernel():
        v, cm = sceneseg.Votes(n, C, dev), sceneseg.SegMetrics(C, device=dev)
        for logits, rows in parts:
            v.add(logits, rows)
        return v.finish(labels32, cm)[0], cm.counts

    def composed():
        acc, cnt = torch.zeros(n, C, device=dev), torch.zeros(n, device=dev)
        for logits, rows in parts:
            acc.index_add_(0, rows.long(), logits.t())
            cnt.index_add_(0, rows.long(), torch.ones(rows.numel(), device=dev))
        pred = (acc / cnt.clamp(min=1).unsqueeze(1)).argmax(1)
        return pred, torch.bincount(labels * C + pred, minlength=C * C)
    (pk, ck), (pc, cc) = kernel(), composed()
    res = dict(op="vote merge", n=n, voxel=voxel, m=grid.m, parts=grid.count_max,
               equal=bool(torch.equal(pk.long(), pc) and torch.equal(ck[:-1], cc)))
    res.update(time_forms({"kernel": kernel, "composed": composed}, a))
    res["against_composed"] = round(res["composed_us"] / res["kernel_us"], 2)
    return res


def bench_crop(dev, a):
    b, rows, k = 32, 300000, 24000
    rng = np.random.default_rng(4)
    coord_h = (rng.uniform(0, 1, (b * rows, 3)) * np.array([8.0, 6.0, 3.0])).astype(np.float32)
    coord = torch.from_numpy(coord_h).to(dev)
    sizes, centres = [rows] * b, [int(c) for c in rng.integers(0, rows, b)]

    def composed():
        out = []
        for i, c in enumerate(centres):
            cloud = coord[i * rows:(i + 1) * rows]
            out.append(torch.topk(sceneseg.crop_distance(cloud, cloud[c]), k, largest=False, sorted=False)[1])
        return torch.stack(out)

    def host():
        return [np.argsort(np.sum(np.square(coord_h[i * rows:(i + 1) * rows] - coord_h[i * rows + c]), 1))[:k]
                for i, c in enumerate(centres)]
    got = sceneseg.crop_nearest(coord, sizes, centres, k).long()
    want = torch.sort(composed() + torch.arange(b, device=dev).unsqueeze(1) * rows, dim=1)[0]
    res = dict(op="crop_nearest", clouds=b, rows=rows, k=k, equal=bool(torch.equal(got, want)))
    res.update(time_forms({"kernel": lambda: sceneseg.crop_nearest(coord, sizes, centres, k), "composed": composed,
                           "host": host}, a, host=("host",)))
    res["against_composed"] = round(res["composed_us"] / res["kernel_us"], 2)
    res["against_host"] = round(res["host_us"] / res["kernel_us"], 2)
    return res


def bench_e2e(dev, a):
    """One SegStep and one SceneTester scene with PointNeXt-S: the kernels' metric / merge against the composed ones."""
    out = []
    C, B, N = 13, a.e2e_batch, 24000
    g = torch.Generator().manual_seed(5)
    data = {'pos': (torch.rand(B, N, 3, generator=g) * torch.tensor([4.0, 4.0, 3.0])).to(dev),
            'x': torch.rand(B, 4, N, generator=g).to(dev), 'y': torch.randint(0, C, (B, N), generator=g).to(dev)}
    model = sceneseg.BaseSeg().to(dev)
    steps = {f: sceneseg.SegStep(model, metrics=sceneseg.SegMetrics(C, device=dev, fused=f)) for f in (True, False)}
    res = dict(op="SegStep PointNeXt-S", shape=[B, N])
    res.update(time_forms({"kernel": lambda: steps[True](data), "composed": lambda: steps[False](data)}, a))
    res["against_composed"] = round(res["composed_us"] / res["kernel_us"], 2)
    out.append(res)
    n = a.e2e_points
    rng = np.random.default_rng(6)
    coord = torch.from_numpy((rng.uniform(0, 1, (n, 3)) * np.array([4.0, 4.0, 3.0])).astype(np.float32)).to(dev)
    feat, label = torch.rand(n, 3, device=dev), torch.from_numpy(rng.integers(0, C, n)).to(dev)
    testers = {f: sceneseg.SceneTester(model, C, voxel_size=0.04, fused=f) for f in (True, False)}
    res = dict(op="SceneTester PointNeXt-S", n=n, voxel=0.04)
    res.update(time_forms({"kernel": lambda: testers[True](coord, feat, label, draws='device'),
                           "composed": lambda: testers[False](coord, feat, label, draws='device')}, a))
    res["parts"] = len(testers[True].parts)
    res["against_composed"] = round(res["composed_us"] / res["kernel_us"], 2)
    out.append(res)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--e2e", action="store_true", help="also time one SegStep and one SceneTester scene with PointNeXt-S")
    ap.add_argument("--only-e2e", action="store_true")
    ap.add_argument("--e2e-batch", type=int, default=2)
    ap.add_argument("--e2e-points", type=int, default=100000)
    ap.add_argument("--out", default="")
    ap.add_argument("--stamp", default=None, help="the commit to record (default: git rev-parse HEAD)")
    a = ap.parse_args()
    assert a.blocks >= 5, "medians are of at least 5 blocks"
    commit = a.stamp
    if commit is None:
        r = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True)
        commit = r.stdout.strip() if r.returncode == 0 else "unknown"
    if not torch.cuda.is_available():
        raise SystemExit("bench_scene_seg.py needs the GPU: a CPU run measures nothing")
    dev = torch.device("cuda:0")
    head = {"bench": "scene segmentation kernels against the composed torch form; whole calls, host reads included",
            "commit": commit, "blocks": a.blocks}
    lines = []

    def record(res):
        res = dict(head, **res)
        lines.append(res)
        print(json.dumps(res), flush=True)
    if not a.only_e2e:
        for fn in (bench_confusion, bench_votes, bench_crop):
            record(fn(dev, a))
            torch.cuda.empty_cache()
    if a.e2e or a.only_e2e:
        for res in bench_e2e(dev, a):
            record(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            for r in lines:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
