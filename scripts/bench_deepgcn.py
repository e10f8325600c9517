"""DeepGCN's kernels against the composed forms, per block shape of the default model at B = 32, N = 1024, C = 64, k = 16
and dilation d in {1, 4, 8, 13}, alternating in ONE process under hipGraph replay (the method of scripts/bench_dgcnn.py):

  * the dilated kNN graph of the block's input: `layers.knn_dilated` (csrc/knn.hip, k d neighbours searched, k
    written) against `torch.cdist(x, x).topk(k d, largest=False).indices[..., ::d]`, the reference's lines, which
    materialise (B, N, N);
  * one `ResDynBlock` 64 -> 64, forward + backward in training mode: fused (csrc/edge_conv.hip with ReLU and the
    residual in the output kernel, the reverse-neighbour lists built ahead as the index step does) against composed
    (group_points + Conv2d / BatchNorm2d / ReLU / max + the residual add on PyTorch), both on the same graph handed in;
    `csr_us`: the fused form's index work (apn_ec_csr) alone;
  * the head (GraphConv 4 -> 64 on the coordinates' graph, d = 1), the same two forms.

    python scripts/bench_deepgcn.py [--blocks 5] [--steps 50] [--warmup 20] [--out profiles/deepgcn_blocks.jsonl] [--stamp COMMIT]

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
from adaptpoint_amd.deepgcn import GraphConv, ResDynBlock
from adaptpoint_amd.pointnext import fill_parameters_by_name
from adaptpoint_amd.synthetic import seeded_normal, unit_sphere_cloud

B, N, K = 32, 1024, 16
SHAPES = [(4, 64, 1), (64, 64, 1), (64, 64, 4), (64, 64, 8), (64, 64, 13)]          # (C, H, dilation); C = 4: the head


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
    kw = dict(norm_args={'norm': 'bn'}, act_args={'act': 'relu'})
    for li, (C, H, d) in enumerate(SHAPES):
        if C == 4:          # the head: (x, y, z, height) features on the coordinates' graph
            rows = torch.from_numpy(unit_sphere_cloud(B, N, seed=N)).to(dev)
            x = torch.cat([rows, rows[:, :, 1:2] - rows[:, :, 1:2].min(1, keepdim=True)[0]], -1).transpose(1, 2).contiguous()
        else:               # a block's features
            rows = torch.from_numpy(seeded_normal((B, N, C), N + li)).float().to(dev)
            x = rows.transpose(1, 2).contiguous()
        x.requires_grad_(True)
        gout = torch.from_numpy(seeded_normal((B, H, N), N + 10 + li)).float().to(dev)
        make = (lambda f: GraphConv(C, H, 'edge', fused=f, bias=False, **kw)) if C != H else \
               (lambda f: ResDynBlock(C, 'edge', K, d, fused=f, **kw))
        mods = {k: fill_parameters_by_name(make(k == "fused")).to(dev).train() for k in ("fused", "composed")}
        idx = layers.knn_dilated(rows, rows, K, d)
        index = edge_conv.edge_index(idx)
        leaves = {k: [x] + list(m.parameters()) for k, m in mods.items()}
        forms = {
            "knn": lambda: layers.knn_dilated(rows, rows, K, d),
            "cdist_topk": lambda: torch.cdist(rows, rows).topk(k=K * d, dim=-1, largest=False, sorted=True)
                                       .indices[..., ::d].int().contiguous(),
            "csr": lambda: edge_conv.edge_index(idx),
            "fused": lambda: torch.autograd.grad(mods["fused"](x.unsqueeze(-1), index), leaves["fused"], gout.unsqueeze(-1)),
            "composed": lambda: torch.autograd.grad(mods["composed"](x.unsqueeze(-1), idx), leaves["composed"],
                                                    gout.unsqueeze(-1)),
        }
        res = {"bench": "DeepGCN block: dilated kNN graph; " + ("head GraphConv" if C != H else "ResDynBlock")
                        + " fwd+bwd, training; hipGraph replay", "commit": commit,
               "B": B, "N": N, "K": K, "dilation": d, "searched": K * d, "C": C, "H": H, "blocks": a.blocks, "steps": a.steps}
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
