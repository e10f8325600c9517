"""The earth mover's distance kernels against the same algorithm composed in PyTorch, per shape (B, n, m), alternating in
ONE process under hipGraph replay (the method and the timing loop of scripts/bench_chamfer.py):

  * kernel: `emd.earth_mover_distance` -- the iteration (csrc/emd.hip) and the cost and gradients recomputed from its
    two tables; no (B,m,n) tensor exists;
  * materialising: `approxmatch_forward` + `matchcost_forward` (+ `matchcost_backward`), the reference extension's three
    calls on the same kernels: `match` (B,m,n) is written once and read back;
  * composed: ten levels of dense (B,m,n) operations under no_grad for `match`, then sum(d * match) / n with autograd
    through d (match is a constant in the gradient, as in the reference).
Forward alone and forward + backward.  Same inputs for all.

Shapes: whole clouds (32,1024,1024), (32,2048,2048), (4,8192,8192) and the per-patch loss (2048,32,32).

    python scripts/bench_emd.py [--blocks 5] [--steps 50] [--warmup 20] [--out profiles/emd.jsonl] [--stamp COMMIT]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import torch

from adaptpoint_amd import emd
from adaptpoint_amd.synthetic import seeded_normal
from bench_chamfer import time_forms

SHAPES = [(32, 1024, 1024), (32, 2048, 2048), (4, 8192, 8192), (2048, 32, 32)]
LEVELS = [-(4.0 ** j) for j in range(7, -2, -1)] + [0.0]


def composed_distances(a, b):
    return (b[:, :, None] - a[:, None]).square().sum(-1)                # (B,m,n)


@torch.no_grad()
def composed_match(a, b):
    n, m = a.shape[1], b.shape[1]
    multi_l, multi_r = (1, n // m) if n >= m else (m // n, 1)
    d = composed_distances(a, b)
    rem_l = torch.full_like(a[:, :, 0], multi_l)
    rem_r = torch.full_like(b[:, :, 0], multi_r)
    match = torch.zeros_like(d)
    for level in LEVELS:
        e = torch.exp(level * d)
        rat_l = rem_l / (1e-9 + (e * rem_r[:, :, None]).sum(1))
        sumr = (e * rat_l[:, None, :]).sum(2) * rem_r
        rat_r = (rem_r / (sumr + 1e-9)).clamp(max=1) * rem_r
        rem_r = (rem_r - sumr).clamp(min=0)
        w = e * rat_l[:, None, :] * rat_r[:, :, None]
        rem_l = (rem_l - w.sum(1)).clamp(min=0)
        match += w
    return match


def composed_loss(a, b):
    match = composed_match(a.detach(), b.detach())
    return ((composed_distances(a, b) * match).sum((1, 2)) / a.size(1)).mean()


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
    loss = emd.earth_mover_distance()
    lines = []
    for B, n, m in SHAPES:
        x = torch.from_numpy(seeded_normal((B, n, 3), n + 1)).float().to(dev).requires_grad_(True)
        y = torch.from_numpy(seeded_normal((B, m, 3), m + 2)).float().to(dev).requires_grad_(True)
        xd, yd = x.detach(), y.detach()
        scale = torch.full((B,), 1.0 / (n * B), device=dev)

        def materialising(backward):
            match = emd.approxmatch_forward(xd, yd)
            cost = emd.matchcost_forward(xd, yd, match)
            return (cost, *emd.matchcost_backward(scale, xd, yd, match)) if backward else cost
        forms = {
            "kernel_fwd": lambda: loss(xd, yd),
            "materialising_fwd": lambda: materialising(False),
            "composed_fwd": lambda: composed_loss(xd, yd),
            "kernel_fwd_bwd": lambda: torch.autograd.grad(loss(x, y), [x, y]),
            "materialising_fwd_bwd": lambda: materialising(True),
            "composed_fwd_bwd": lambda: torch.autograd.grad(composed_loss(x, y), [x, y]),
        }
        with torch.no_grad():
            ours, theirs = loss(xd, yd).item(), composed_loss(xd, yd).item()
        res = {"bench": "earth mover's distance: earth_mover_distance forward alone and forward + backward; kernels from "
                        "the tables, kernels through a materialised match, composed PyTorch; hipGraph replay",
               "commit": commit, "B": B, "n": n, "m": m, "blocks": a.blocks, "steps": a.steps,
               "loss_kernel": ours, "loss_composed": theirs}
        res.update(time_forms(forms, [x, y], a))
        for what in ("fwd", "fwd_bwd"):
            if f"kernel_{what}_us" in res and f"composed_{what}_us" in res:
                res[f"{what}_speedup"] = round(res[f"composed_{what}_us"] / res[f"kernel_{what}_us"], 2)
            if f"kernel_{what}_us" in res and f"materialising_{what}_us" in res:
                res[f"{what}_materialising_over_kernel"] = round(res[f"materialising_{what}_us"] / res[f"kernel_{what}_us"], 2)
        res["match_bytes"] = 4 * B * n * m                       # the (B, m, n) tensor the kernel path never allocates
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
