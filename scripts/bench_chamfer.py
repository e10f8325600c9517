"""The Chamfer kernels against the composed PyTorch form, per shape (B, n, m), alternating in ONE process under hipGraph
replay (the method of scripts/bench_deepgcn.py):

  * forward alone: `chamfer_dist.forward` (csrc/chamfer.hip, one launch, both directions) against
    `d = (a[:, :, None] - b[:, None]).square().sum(-1)`, `d.min(2)`, `d.min(1)`, which materialises (B, n, m, 3);
  * forward + backward of `ChamferDistanceL1` (the masked autoencoder's loss): the kernels under the module's PyTorch
    reductions against the same composed distances with sqrt / mean and autograd.  Same inputs for both.

Shapes: whole clouds (32,1024,1024), (32,2048,2048), (8,8192,8192) and the per-patch loss (2048,32,32).

    python scripts/bench_chamfer.py [--blocks 5] [--steps 50] [--warmup 20] [--out profiles/chamfer.jsonl] [--stamp COMMIT]

Per shape: the median (and min / max) over `--blocks` blocks of `--steps` replays each, the forms alternating; one JSON
line per shape.  A form whose capture holds a memset node (refused by graphs.capture) is timed eagerly and marked so; a
composed form that cannot allocate its tensors is reported as "out of memory" and has no time.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from adaptpoint_amd import chamfer_dist, graphs
from adaptpoint_amd.synthetic import seeded_normal

SHAPES = [(32, 1024, 1024), (32, 2048, 2048), (8, 8192, 8192), (2048, 32, 32)]


def composed_distances(a, b):
    d = (a[:, :, None] - b[:, None]).square().sum(-1)
    return d.min(2)[0], d.min(1)[0]


def composed_l1(a, b):
    d1, d2 = composed_distances(a, b)
    return (d1.sqrt().mean() + d2.sqrt().mean()) / 2


def time_forms(forms, leaves, a):
    """{name_us: median us per call} (and min / max) of the callables in `forms`, each replayed from its own hipGraph."""
    res, live = {}, {}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for k, fn in forms.items():
            try:
                for _ in range(3):
                    fn()
                live[k] = fn
            except torch.OutOfMemoryError:
                res[k + "_timing"] = "out of memory"
                torch.cuda.empty_cache()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    replay, how, keep = {}, {}, []
    for k, fn in live.items():
        try:
            g = graphs.capture(fn, leaves=leaves, what=k)
            keep.append(g)
            replay[k], how[k] = g[0].replay, "graph"
        except graphs.MemsetNodeInGraph:
            replay[k], how[k] = fn, "eager"
        except torch.OutOfMemoryError:
            res[k + "_timing"] = "out of memory"
            torch.cuda.empty_cache()
    for _ in range(a.warmup):
        for fn in replay.values():
            fn()
    torch.cuda.synchronize()
    ev = {k: [] for k in replay}
    for _ in range(a.blocks):                       # alternating blocks: the forms see the same clocks
        for k, fn in replay.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                fn()
            e1.record()
            ev[k].append((e0, e1))
    torch.cuda.synchronize()
    for k, pairs in ev.items():
        t = sorted(e0.elapsed_time(e1) * 1e3 / a.steps for e0, e1 in pairs)
        res[k + "_us"] = round(t[len(t) // 2], 1)
        res[k + "_us_min_max"] = [round(t[0], 1), round(t[-1], 1)]
        if how[k] != "graph":
            res[k + "_timing"] = how[k]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default="")
    ap.add_argument("--stamp", default=None, help="the commit to record (default: git rev-parse HEAD)")
    a = ap.parse_args()
    assert a.blocks >= 5 and a.steps >= 50, "medians are of at least 5 blocks of at least 50 steps"
    commit = a.stamp
    if commit is None:
        r = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True)
        commit = r.stdout.strip() if r.returncode == 0 else "unknown"
    dev = torch.device("cuda:0")
    loss = chamfer_dist.ChamferDistanceL1()
    lines = []
    for B, n, m in SHAPES:
        x = torch.from_numpy(seeded_normal((B, n, 3), n + 1)).float().to(dev).requires_grad_(True)
        y = torch.from_numpy(seeded_normal((B, m, 3), m + 2)).float().to(dev).requires_grad_(True)
        xd, yd = x.detach(), y.detach()
        forms = {
            "kernel_fwd": lambda: chamfer_dist.forward(xd, yd),
            "composed_fwd": lambda: composed_distances(xd, yd),
            "kernel_fwd_bwd": lambda: torch.autograd.grad(loss(x, y), [x, y]),
            "composed_fwd_bwd": lambda: torch.autograd.grad(composed_l1(x, y), [x, y]),
        }
        res = {"bench": "Chamfer distance: forward alone; ChamferDistanceL1 forward + backward; kernels against composed "
                        "PyTorch; hipGraph replay", "commit": commit, "B": B, "n": n, "m": m, "blocks": a.blocks,
               "steps": a.steps}
        res.update(time_forms(forms, [x, y], a))
        for what in ("fwd", "fwd_bwd"):
            if f"kernel_{what}_us" in res and f"composed_{what}_us" in res:
                res[f"{what}_speedup"] = round(res[f"composed_{what}_us"] / res[f"kernel_{what}_us"], 2)
        res["composed_pair_bytes"] = 4 * B * n * m * 3          # the (B, n, m, 3) differences the composed form materialises
        lines.append(res)
        print(json.dumps(res), flush=True)
        del forms
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            for r in lines:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
