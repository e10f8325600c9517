"""RandLA-Net's LocalFeatureAggregation block, fused (csrc/randla.hip) against composed, and a whole RandLANet training
step, in ONE process with the forms alternating (the method and the timer of scripts/bench_pointops.py):

  * one `LocalFeatureAggregation` block in training mode, forward and forward + backward (gradients of the input
    features and of every parameter), at the four encoder shapes of a 45 056-point cloud -- B 4, K 16, decimation 4:
    N = 45056 / 11264 / 2816 / 704 with d_out 16 / 64 / 128 / 256 --, `fused` against `composed` (the reference's operator
    sequence in PyTorch) on the SAME precomputed graph; the graph's own cost (`layers.knn_query`) is a field of the
    line.  hipGraph replay unless a form's capture holds a memset node (then eager, and the line says so; `fused_eager_*`
    is the fused form timed eagerly on purpose beside an eager composed form).  `*_peak_mb`: the growth of
    `torch.cuda.max_memory_allocated` over one eager call;
  * `RandLANet(d_in 6, 19 classes, K 16, decimation 4)` at 4 x 45 056 points, one training step (forward, summed
    cross-entropy, backward; no optimiser) with a supplied device permutation, eager, fused against composed, with the
    peak memory of both.

    python scripts/bench_randla.py [--blocks 5] [--steps 50] [--warmup 5] [--out profiles/randla.jsonl] [--stamp COMMIT]
                                   [--no-model]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch

from adaptpoint_amd.pointnext import fill_parameters_by_name
from adaptpoint_amd.randla import LocalFeatureAggregation, RandLANet, knn_graph
from bench_pointops import time_forms

B, K, POINTS = 4, 16, 45056
LEVELS = [(45056, 8, 16), (11264, 32, 64), (2816, 128, 128), (704, 256, 256)]          # (N, d_in, d_out)


def peak_mb(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)


def event_us(fn, reps=5):
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) * 1000.0 / reps, 1)


def block_lines(a, dev, head, emit):
    for N, d_in, d_out in LEVELS:
        g = torch.Generator().manual_seed(N)
        coords = (torch.rand(B, N, 3, generator=g) * 50.0).to(dev)
        x = torch.randn(B, d_in, N, 1, generator=g).to(dev).requires_grad_(True)
        w = torch.randn(B, 2 * d_out, N, 1, generator=g).to(dev)
        blocks = {}
        for form in ("fused", "composed"):
            torch.manual_seed(3)
            blocks[form] = LocalFeatureAggregation(d_in, d_out, K, dev, fused=form == "fused").to(dev).train()
        graph = knn_graph(coords, coords, K)
        knn_us = event_us(lambda: knn_graph(coords, coords, K))

        def run(form, backward):
            block = blocks[form]
            leaves = [x, *block.parameters()]

            def fn():
                out = block(coords, x, graph)
                if not backward:
                    return [out.detach()]
                return [out.detach(), *torch.autograd.grad(out, leaves, w)]
            return fn
        for what, backward in (("fwd", False), ("fwd_bwd", True)):
            forms = {f"{form}_{what}": run(form, backward) for form in blocks}
            forms[f"fused_eager_{what}"] = run("fused", backward)
            leaves = [x, *(q for block in blocks.values() for q in block.parameters())]
            res = dict(head, batch=f"{B} x {N}", k=K, d_in=d_in, d_out=d_out, c=d_out // 2, op=f"lfa_{what}", knn_us=knn_us)
            for key, fn in forms.items():
                if not key.startswith("fused_eager"):
                    res[key + "_peak_mb"] = peak_mb(fn)
            res.update(time_forms(forms, leaves, a, eager=(f"fused_eager_{what}",)))
            res["speedup_over_composed"] = round(res[f"composed_{what}_us"] / res[f"fused_{what}_us"], 2)
            emit(res)
        del blocks, graph, coords, x, w
        torch.cuda.empty_cache()


def model_line(a, dev, head, emit):
    g = torch.Generator().manual_seed(12)
    inp = torch.cat([torch.rand(B, POINTS, 3, generator=g) * 50.0, torch.randn(B, POINTS, 3, generator=g)], -1).to(dev)
    labels = torch.randint(0, 19, (B, POINTS), generator=g).to(dev)
    perm = torch.randperm(POINTS, generator=g).to(dev)
    models = {form: fill_parameters_by_name(RandLANet(6, 19, K, 4, device=dev, fused=form == "fused")).train()
              for form in ("fused", "composed")}

    def step(form):
        m = models[form]

        def fn():
            m.zero_grad(set_to_none=True)
            torch.nn.functional.cross_entropy(m(inp, permutation=perm), labels, reduction='sum').backward()
        return fn
    forms = {f"{form}_step": step(form) for form in models}
    res = dict(head, batch=f"{B} x {POINTS}", k=K, op="randlanet_train_step", timing="eager")
    for key, fn in forms.items():
        fn()
        res[key + "_peak_mb"] = peak_mb(fn)
    ev = {key: [] for key in forms}
    steps = max(2, min(a.steps, 4))
    for _ in range(a.blocks):                                   # alternating blocks: the forms see the same clocks
        for key, fn in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                fn()
            e1.record()
            ev[key].append((e0, e1))
    torch.cuda.synchronize()
    for key, pairs in ev.items():
        t = sorted(e0.elapsed_time(e1) / steps for e0, e1 in pairs)
        res[key + "_ms"] = round(t[len(t) // 2], 2)
        res[key + "_ms_min_max"] = [round(t[0], 2), round(t[-1], 2)]
    res["steps_per_block"] = steps
    res["speedup_over_composed"] = round(res["composed_step_ms"] / res["fused_step_ms"], 2)
    emit(res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--stamp", default=None, help="the commit to record (default: git rev-parse HEAD)")
    ap.add_argument("--no-model", action="store_true", help="the block lines only")
    a = ap.parse_args()
    assert a.blocks >= 5, "medians are of at least 5 blocks"
    commit = a.stamp
    if commit is None:
        r = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True)
        commit = r.stdout.strip() if r.returncode == 0 else "unknown"
    dev = torch.device("cuda:0")
    head = dict(bench="randla", commit=commit, device=torch.cuda.get_device_name(0), blocks=a.blocks)
    lines = []

    def emit(res):
        lines.append(res)
        print(json.dumps(res), flush=True)
        if a.out:                                               # written line by line: a run cut short keeps what it measured
            with open(os.path.join(ROOT, a.out) if not os.path.isabs(a.out) else a.out, "w") as fh:
                fh.writelines(json.dumps(line) + "\n" for line in lines)
    block_lines(a, dev, head, emit)
    if not a.no_model:
        model_line(a, dev, head, emit)


if __name__ == "__main__":
    main()
