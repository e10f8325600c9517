"""One InvResMLP block, forward + backward in training mode, fused (csrc/local_aggr.hip) against composed (ball query +
group_points + Conv2d / BatchNorm2d / ReLU / max on PyTorch, the pointwise convolutions as modules: what the package
offered for this block before), alternating in ONE process under hipGraph replay.

    python scripts/bench_invres.py [--blocks 5] [--steps 50] [--warmup 20] [--out profiles/invres_blocks.jsonl] [--stamp COMMIT]

Both forms include their index work (the ball query of p around p; the fused form also its NeighbourIndex), because a
stand-alone block pays it; inside `PointNextEncoder` a stage's blocks share one.  `*_shared_us`: the same with the index
work done ahead, as the second and later blocks of a stage run.  Per shape: the median over `--blocks` blocks of
`--steps` replays each (fused block, composed block, fused block, ...), and the bytes each form must move, from the shapes.
One JSON line per shape.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from adaptpoint_amd import fused_wide, graphs, layers
from adaptpoint_amd.pointnext import InvResMLP, fill_parameters_by_name
from adaptpoint_amd.synthetic import seeded_normal, unit_sphere_cloud

SHAPES = [(32, 512, 64), (32, 256, 128), (32, 128, 256), (32, 64, 512), (8, 6000, 64), (8, 1500, 128)]
K = 32


def algorithmic(B, N, C, E, distinct):
    """Bytes (float32 tensors read or written once per use) of the AGGREGATION's forward + backward in both forms; the
    pointwise convolutions (C -> E C -> C) move the same bytes in both and are listed once."""
    grouped_in, grouped_out = B * (C + 3) * N * K, B * C * N * K
    composed = 4 * (B * (C + 3) * N + grouped_in                 # group: read points, write the grouped input
                    + grouped_in + grouped_out                   # conv: read, write
                    + 2 * grouped_out + 2 * grouped_out          # BatchNorm (statistics, apply), ReLU + max
                    + 3 * grouped_out + 2 * grouped_out          # backward: max / ReLU / BatchNorm over the grouped output
                    + grouped_out + grouped_in + grouped_in      # conv backward: input gradient, weight gradient
                    + grouped_in + B * (C + 3) * N)              # group backward
    rows = B * N * distinct
    fused = 4 * (2 * B * C * N                                   # U = Wf f
                 + rows * C + 3 * B * C * N                      # pool: distinct rows of U; ext, ysum (+ sel bytes)
                 + 2 * B * C * N                                 # out
                 + 3 * B * C * N + rows * C * 5 // 4             # backward prep; rows of g' and sel per point
                 + 3 * B * C * N + 4 * B * C * N)                # dU, dT; dL/df, dL/dW
    pw = 4 * 2 * 3 * (B * C * N + B * E * C * N)
    return {"composed_aggr_bytes": composed, "fused_aggr_bytes": fused, "pointwise_bytes": pw}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--radius", type=float, default=0.2)
    ap.add_argument("--expansion", type=int, default=4)
    ap.add_argument("--out", default="")
    ap.add_argument("--stamp", default=None, help="the commit to record (default: git rev-parse HEAD)")
    a = ap.parse_args()
    assert a.blocks >= 5 and a.steps >= 50, "medians are of at least 5 blocks of at least 50 steps"
    commit = a.stamp
    if commit is None:
        r = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True)
        commit = r.stdout.strip() if r.returncode == 0 else "unknown"
    dev = torch.device("cuda:0")
    lines = []
    for B, N, C in SHAPES:
        # the radius follows the density (6-10 distinct neighbours per point at the listed shapes; printed)
        radius = a.radius * (512.0 / N) ** (1.0 / 3.0)
        p = torch.from_numpy(unit_sphere_cloud(B, N, seed=N)).to(dev)
        f = torch.from_numpy(seeded_normal((B, C, N), N + 1)).float().to(dev).requires_grad_(True)
        gout = torch.from_numpy(seeded_normal((B, C, N), N + 2)).float().to(dev)
        group_args = dict(NAME='ballquery', normalize_dp=True, radius=radius, nsample=K)
        mods = {k: fill_parameters_by_name(InvResMLP(C, expansion=a.expansion, fused=k == "fused", group_args=group_args)).to(dev).train()
                for k in ("fused", "composed")}
        idx = layers.ball_query(radius, K, p, p)
        distinct = float((idx[:, :, 1:] != idx[:, :, :1]).sum(-1).float().mean()) + 1.0
        nbr = fused_wide.neighbour_index(idx, p, N)
        leaves = {k: [f] + list(m.parameters()) for k, m in mods.items()}

        def step(k, index):
            return torch.autograd.grad(mods[k]([p, f], index=index)[1], leaves[k], gout)
        forms = {"fused": lambda: step("fused", None), "composed": lambda: step("composed", None),
                 "fused_shared": lambda: step("fused", nbr), "composed_shared": lambda: step("composed", idx)}
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                for fn in forms.values():
                    fn()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        keep = {k: graphs.capture(fn, leaves=leaves[k.split("_")[0]], what=k) for k, fn in forms.items()}
        replay = {k: v[0].replay for k, v in keep.items()}
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
        res = {"bench": "InvResMLP block fwd+bwd, training, hipGraph replay", "commit": commit, "B": B, "N": N, "C": C,
               "expansion": a.expansion, "radius": round(radius, 4), "distinct_neighbours": round(distinct, 1),
               "blocks": a.blocks, "steps": a.steps}
        for k, pairs in ev.items():
            t = sorted(e0.elapsed_time(e1) * 1e3 / a.steps for e0, e1 in pairs)
            res[k + "_us"] = round(t[len(t) // 2], 1)
            res[k + "_us_min_max"] = [round(t[0], 1), round(t[-1], 1)]
        res["speedup"] = round(res["composed_us"] / res["fused_us"], 2)
        res["speedup_shared"] = round(res["composed_shared_us"] / res["fused_shared_us"], 2)
        res.update(algorithmic(B, N, C, a.expansion, distinct))
        lines.append(res)
        print(json.dumps(res), flush=True)
        del keep, replay
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            for r in lines:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
