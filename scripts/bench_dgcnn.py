"""DGCNN's two kernels against what the package offered before, per DGCNN layer shape at B = 32, N = 1024, K = 20,
alternating in ONE process under hipGraph replay (as scripts/bench_invres.py):

  * the kNN graph of the layer's input (C = 3, 64, 64, 128): `layers.knn_query` (csrc/knn.hip) against
    `torch.cdist(x, x).topk(k, largest=False)`, the reference's call, which materialises (B, N, N);
  * one EdgeConv block (C -> H = 3 -> 64, 64 -> 64, 64 -> 128, 128 -> 256), forward + backward in training mode: fused
    (csrc/edge_conv.hip, the reverse-neighbour lists built ahead as the index step does) against composed
    (group_points + Conv2d / BatchNorm2d / LeakyReLU / max on PyTorch: what the parent commit would run), both on the
    same graph handed in; `csr_us`: the fused form's index work (apn_ec_csr) alone.

    python scripts/bench_dgcnn.py [--blocks 5] [--steps 50] [--warmup 20] [--out profiles/dgcnn_blocks.jsonl] [--stamp COMMIT]

Per shape: the median over `--blocks` blocks of `--steps` replays each, the forms alternating; one JSON line per shape.
A form whose capture holds a memset node (refused by graphs.capture) is timed eagerly and marked so.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from adaptpoint_amd import edge_conv, graphs, layers
from adaptpoint_amd.dgcnn import LEAKY, EdgeConv
from adaptpoint_amd.pointnext import fill_parameters_by_name
from adaptpoint_amd.synthetic import seeded_normal, unit_sphere_cloud

LAYERS = [(3, 64), (64, 64), (64, 128), (128, 256)]
B, N, K = 32, 1024, 20


def time_forms(forms, leaves, a):
    """{name: median us per call} (and min / max) of the callables in `forms`, each replayed from its own hipGraph."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            for fn in forms.values():
                fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    replay, how, keep = {}, {}, []
    for k, fn in forms.items():
        try:
            g = graphs.capture(fn, leaves=leaves.get(k, ()), what=k)
            keep.append(g)
            replay[k], how[k] = g[0].replay, "graph"
        except graphs.MemsetNodeInGraph:
            replay[k], how[k] = fn, "eager"
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
    res = {}
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
    lines = []
    for li, (C, H) in enumerate(LAYERS):
        if C == 3:
            rows = torch.from_numpy(unit_sphere_cloud(B, N, seed=N)).to(dev)                  # the head: coordinates
        else:
            rows = torch.from_numpy(seeded_normal((B, N, C), N + li)).float().to(dev)         # a layer's features
        x = rows.transpose(1, 2).contiguous().requires_grad_(True)
        gout = torch.from_numpy(seeded_normal((B, H, N), N + 10 + li)).float().to(dev)
        mods = {k: fill_parameters_by_name(EdgeConv(C, H, norm_args={'norm': 'bn'}, act_args=dict(LEAKY),
                                                    fused=k == "fused")).to(dev).train() for k in ("fused", "composed")}
        idx = layers.knn_query(rows, rows, K)
        index = edge_conv.edge_index(idx)
        leaves = {k: [x] + list(m.parameters()) for k, m in mods.items()}
        forms = {
            "knn": lambda: layers.knn_query(rows, rows, K),
            "cdist_topk": lambda: torch.cdist(rows, rows).topk(k=K, dim=-1, largest=False, sorted=True).indices.int(),
            "csr": lambda: edge_conv.edge_index(idx),
            "fused": lambda: torch.autograd.grad(mods["fused"](x.unsqueeze(-1), index), leaves["fused"], gout.unsqueeze(-1)),
            "composed": lambda: torch.autograd.grad(mods["composed"](x.unsqueeze(-1), idx), leaves["composed"],
                                                    gout.unsqueeze(-1)),
        }
        res = {"bench": "DGCNN layer: kNN graph; EdgeConv block fwd+bwd, training; hipGraph replay", "commit": commit,
               "B": B, "N": N, "K": K, "C": C, "H": H, "blocks": a.blocks, "steps": a.steps}
        res.update(time_forms(forms, leaves, a))
        res["knn_speedup"] = round(res["cdist_topk_us"] / res["knn_us"], 2)
        res["block_speedup"] = round(res["composed_us"] / res["fused_us"], 2)
        # what the composed block materialises and the fused one does not: the grouped input and the grouped output
        res["composed_grouped_bytes"] = 4 * B * N * K * (2 * C + H)
        lines.append(res)
        print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            for r in lines:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
