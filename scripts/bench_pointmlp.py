"""PointMLP's fused stages against the composed PyTorch form of the same commit, for `pointMLP` and `pointMLPElite` at
B = 32, N = 1024, on the same graphs (built once, ahead: the index step is not timed), alternating in ONE process:

  * each stage's LocalGrouper + PreExtraction, forward (no_grad, training-mode BatchNorm) and forward + backward:
    fused (csrc/affine_group.hip + the contraction kernels) against composed (gather, normalise, affine, concatenate,
    permute, Conv1d / BatchNorm1d / ReLU, adaptive_max_pool1d on PyTorch);
  * a whole training step of the classifier (forward, loss, every parameter's gradient), graphs handed in;
  * peak allocated memory of one eager training step of each form.

    python scripts/bench_pointmlp.py [--blocks 5] [--steps 20] [--warmup 5] [--out profiles/pointmlp.jsonl] [--stamp COMMIT]

Per row: the median over `--blocks` blocks of `--steps` runs each, the forms alternating; one JSON line per row.  Both
forms of a row are timed the same way: from hipGraph replay when BOTH capture, eagerly otherwise (the row says which).
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from adaptpoint_amd import graphs
from adaptpoint_amd.pointmlp import ELITE, FULL, PointMlpClassifier
from adaptpoint_amd.pointnext import fill_parameters_by_name
from adaptpoint_amd.synthetic import seeded_normal, unit_sphere_cloud

B, N = 32, 1024
CONFIGS = {"pointMLP": FULL, "pointMLPElite": ELITE}


def time_pair(forms, leaves, a):
    """{name_us: median us per call} of the two callables in `forms`, both replayed from hipGraphs when both capture,
    both run eagerly otherwise."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            for fn in forms.values():
                fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    run, keep, how = dict(forms), [], "graph"
    try:
        for k, fn in forms.items():
            g = graphs.capture(fn, leaves=leaves, what=k)
            keep.append(g)
            run[k] = g[0].replay
    except Exception as e:                                   # a memset node, or an operation capture refuses
        run, how = dict(forms), f"eager ({k} does not capture: {type(e).__name__})"
        torch.cuda.synchronize()
    for _ in range(a.warmup):
        for fn in run.values():
            fn()
    torch.cuda.synchronize()
    ev = {k: [] for k in run}
    for _ in range(a.blocks):                       # alternating blocks: the forms see the same clocks
        for k, fn in run.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                fn()
            e1.record()
            ev[k].append((e0, e1))
    torch.cuda.synchronize()
    res = {"timing": how}
    for k, pairs in ev.items():
        t = sorted(e0.elapsed_time(e1) * 1e3 / a.steps for e0, e1 in pairs)
        res[k + "_us"] = round(t[len(t) // 2], 1)
        res[k + "_us_min_max"] = [round(t[0], 1), round(t[-1], 1)]
    return res


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    del out
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--stamp", default=None, help="the commit to record (default: git rev-parse HEAD)")
    a = ap.parse_args()
    assert a.blocks >= 5 and a.steps >= 10, "medians are of at least 5 blocks of at least 10 runs"
    commit = a.stamp
    if commit is None:
        r = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True)
        commit = r.stdout.strip() if r.returncode == 0 else "unknown"
    dev = torch.device("cuda:0")
    pos = torch.from_numpy(unit_sphere_cloud(B, N, seed=N)).to(dev)
    height = pos[:, :, 1:2] - pos[:, :, 1:2].min(1, keepdim=True)[0]
    feats = torch.cat([pos, height], -1).transpose(1, 2).contiguous()
    gt = torch.randint(0, 15, (B,), generator=torch.Generator().manual_seed(N)).to(dev)
    lines = []

    def emit(res):
        lines.append(res)
        print(json.dumps(res), flush=True)

    for name, cfg in CONFIGS.items():
        models = {k: fill_parameters_by_name(PointMlpClassifier(fused=k == "fused", **cfg)).to(dev).train()
                  for k in ("fused", "composed")}
        index = models["fused"].encoder.index(pos)
        head = {"bench": "PointMLP: fused stage against composed PyTorch, same graphs", "commit": commit, "model": name,
                "B": B, "blocks": a.blocks, "steps": a.steps}
        p, n, C = pos, N, cfg["embed_dim"]
        for i, g in enumerate(index):
            S, K = g.idx.shape[1:]
            O = C * cfg["dim_expansion"][i]
            x = torch.from_numpy(seeded_normal((B, C, n), N + 20 + i)).float().to(dev).requires_grad_(True)
            gout = torch.from_numpy(seeded_normal((B, O, S), N + 30 + i)).float().to(dev)
            encs = {k: m.encoder for k, m in models.items()}
            stage = {
                "fused": lambda e=encs["fused"], i=i, g=g, x=x: e._fused_stage(i, x, g, pos_blocks=False),
                "composed": lambda e=encs["composed"], i=i, g=g, x=x, p=p: e.pre_blocks_list[i](
                    e.local_grouper_list[i](p, x.permute(0, 2, 1), g)[1]),
            }
            leaves = {k: [x] + list(e.local_grouper_list[i].parameters()) + list(e.pre_blocks_list[i].parameters())
                      for k, e in encs.items()}

            def fwd(k):
                with torch.no_grad():
                    return stage[k]()
            row = dict(head, what="stage forward", stage=i + 1, N=n, S=S, K=K, C=C, O=O)
            row.update(time_pair({k: (lambda k=k: fwd(k)) for k in stage}, (), a))
            row["speedup"] = round(row["composed_us"] / row["fused_us"], 2)
            emit(row)
            row = dict(head, what="stage forward + backward", stage=i + 1, N=n, S=S, K=K, C=C, O=O)
            row.update(time_pair({k: (lambda k=k: torch.autograd.grad(stage[k](), leaves[k], gout)) for k in stage},
                                 leaves["fused"] + leaves["composed"], a))
            row["speedup"] = round(row["composed_us"] / row["fused_us"], 2)
            # what the composed stage materialises ahead of its first convolution and the fused one does not: the
            # grouped tensor, its difference, the normalised and the affine copy, the repeated anchor (C wide each), the
            # concatenation and its permuted copy (2C wide each)
            row["composed_grouped_bytes"] = 4 * B * S * K * 9 * C
            emit(row)
            p, n, C = g.new_xyz, S, O
        params = {k: [q for q in m.parameters() if q.requires_grad] for k, m in models.items()}

        def step(k):
            logits, loss = models[k].get_logits_loss({'pos': pos, 'x': feats}, gt, graphs=index)
            return torch.autograd.grad(loss, params[k], allow_unused=True)
        row = dict(head, what="training step (forward, loss, all gradients)", N=N)
        row.update(time_pair({k: (lambda k=k: step(k)) for k in models}, params["fused"] + params["composed"], a))
        row["speedup"] = round(row["composed_us"] / row["fused_us"], 2)
        for k in models:
            row[k + "_peak_bytes"] = peak_bytes(lambda k=k: step(k))
        emit(row)
        del models, index, params
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            for r in lines:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
