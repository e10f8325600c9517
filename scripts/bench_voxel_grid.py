"""The device voxel grid (csrc/voxel_grid.hip, `adaptpoint_amd.voxel_grid.voxel_grid`) against two yardsticks on the same
inputs, alternating in ONE process (the method of scripts/bench_pointops.py):

  * `composed`: the same partition composed in PyTorch on the device -- the (cloud, cell) tensor, then
    `torch.unique(dim=0, return_inverse=True, return_counts=True)`, then a stable `torch.sort` of the inverse;
  * `host`: the numpy form in this one process -- `floor`, `np.unique(axis=0)`, a stable argsort -- on host arrays.

Every form is timed EAGERLY and whole: the kernel form reads its stats on the host once per call (its only
synchronisation), `torch.unique` synchronises for its output size.  `VoxelGrid.mean` at c = 6 is timed against
`index_add_` plus a divide (float atomics: its bits change from run to run; the kernel's do not).

Shapes: one cloud of 10^6 uniform points in 8 x 6 x 3 at voxel 0.04; eight stacked clouds of 250 000; 32 ragged clouds of
20 000 to 40 000 at voxel 0.02; 10^6 points in ONE voxel (a mis-set voxel size: the case a design with work non-linear in
a voxel's population turns into a hang).

    python scripts/bench_voxel_grid.py [--blocks 5] [--steps 50] [--warmup 3] [--out profiles/voxel_grid.jsonl] [--stamp COMMIT]

Per shape one JSON line for the partition and one for the mean: the median (and min / max) over `--blocks` alternating
blocks of `--steps` calls, or fewer for a slow form (about 0.3 s per block, at least 1 call), recorded as `<form>_steps`.
Before timing, the kernel's partition is checked against the composed one at the timed size (`partition_equal`).
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

from adaptpoint_amd.voxel_grid import voxel_grid

BOX = (8.0, 6.0, 3.0)


def shapes():
    rng = np.random.default_rng(7)
    ragged = [int(s) for s in rng.integers(20000, 40001, 32)]
    return [("1 x 1000000", [1000000], 0.04), ("8 x 250000", [250000] * 8, 0.04),
            ("32 ragged 20000-40000", ragged, 0.02), ("1000000 in one voxel", [1000000], 16.0)]


def composed(coord, vs, offset):
    n = coord.shape[0]
    cloud = torch.searchsorted(offset.long(), torch.arange(n, device=coord.device), right=True)
    key = torch.cat([cloud.unsqueeze(1), torch.floor(coord.double() / vs).long()], 1)
    _, inverse, count = torch.unique(key, dim=0, return_inverse=True, return_counts=True)
    return inverse, count, torch.sort(inverse, stable=True)[1]


def host(coord, vs, offset):
    n = coord.shape[0]
    cloud = np.searchsorted(offset, np.arange(n), side="right")
    key = np.concatenate([cloud[:, None], np.floor(coord / np.array(vs)).astype(np.int64)], 1)
    _, inverse, count = np.unique(key, axis=0, return_inverse=True, return_counts=True)
    return inverse, count, np.argsort(inverse.reshape(-1), kind="stable")


def time_forms(forms, a):
    """{name_us: median us per call}: alternating blocks, a device synchronise inside every timed window."""
    res, steps = {}, {}
    for k, fn in forms.items():
        for _ in range(1 if k == "host" else a.warmup):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--stamp", default=None, help="the commit to record (default: git rev-parse HEAD)")
    a = ap.parse_args()
    assert a.blocks >= 5, "medians are of at least 5 blocks"
    commit = a.stamp
    if commit is None:
        r = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True)
        commit = r.stdout.strip() if r.returncode == 0 else "unknown"
    if not torch.cuda.is_available():
        raise SystemExit("bench_voxel_grid.py needs the GPU: a CPU run measures nothing")
    dev = torch.device("cuda:0")
    lines = []
    for name, sizes, voxel in shapes():
        n = sum(sizes)
        rng = np.random.default_rng(n + len(sizes))
        coord_h = (rng.uniform(0, 1, (n, 3)) * np.array(BOX)).astype(np.float32)
        offset_h = np.cumsum(sizes).astype(np.int32)
        coord, offset = torch.from_numpy(coord_h).to(dev), torch.from_numpy(offset_h).to(dev)
        grid = voxel_grid(coord, voxel, offset)
        inverse, count, _ = composed(coord, voxel, offset)
        pairs = torch.unique(torch.stack([grid.voxel_of.long(), inverse], 1), dim=0).shape[0]
        equal = bool(pairs == grid.m == count.numel() and
                     torch.equal(torch.sort(grid.count.long())[0], torch.sort(count)[0]))
        head = {"bench": "voxel grid against composed PyTorch (device) and numpy (host); whole eager calls, host read included",
                "commit": commit, "shape": name, "n": n, "clouds": len(sizes), "voxel": voxel, "m": grid.m,
                "count_max": grid.count_max, "blocks": a.blocks}
        res = dict(head, op="partition", partition_equal=equal)
        res.update(time_forms({"kernel": lambda: voxel_grid(coord, voxel, offset),
                               "composed": lambda: composed(coord, voxel, offset),
                               "host": lambda: host(coord_h, voxel, offset_h)}, a))
        res["against_composed"] = round(res["composed_us"] / res["kernel_us"], 2)
        res["against_host"] = round(res["host_us"] / res["kernel_us"], 2)
        lines.append(res)
        print(json.dumps(res), flush=True)

        vals = torch.randn(n, 6, device=dev)
        vo, cnt = grid.voxel_of.long(), grid.count.float().unsqueeze(1)
        res = dict(head, op="mean c=6")
        res.update(time_forms({"kernel": lambda: grid.mean(vals),
                               "composed": lambda: torch.zeros(grid.m, 6, device=dev).index_add_(0, vo, vals) / cnt}, a))
        res["against_composed"] = round(res["composed_us"] / res["kernel_us"], 2)
        lines.append(res)
        print(json.dumps(res), flush=True)
        del coord, vals, grid, inverse, count, vo, cnt
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            for r in lines:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
