"""Point Transformer's layer, fused (csrc/point_transformer.hip) against composed, and a whole PTSeg training step, in ONE
process with the forms alternating (the method and the timer of scripts/bench_pointops.py):

  * one `PointTransformerLayer` in training mode, forward and forward + backward (gradients of the input and of every
    parameter), three forms: `fused` (the kernels, on a shared stage graph), `composed` (the module's composed path on
    the same shared graph) and `reference` (composed as the reference runs a layer: two kNN queries and a fresh
    grouping of the coordinates in every call).  hipGraph replay unless a form's capture holds a memset node (then
    eager, and the line says so; `fused_eager_fwd_bwd` is the fused form timed eagerly on purpose, to compare with
    those); the reverse lists are built before capture.  `*_peak_mb`: the growth of `torch.cuda.max_memory_allocated`
    over one eager call;
  * PTSeg([2,3,4,6,3], width 32) at 8 clouds of 24 000 points, one training step (forward, backward; no optimiser),
    eager -- the sampler reads the offsets on the host --, fused against composed, both with one graph per level.

Shapes: 8 x 24 000 (k 8, C 32), 8 x 6 000 (k 16, C 64), 8 x 1 500 (k 16, C 128), 32 ragged clouds of 700-1300 (k 16, C 64).

    python scripts/bench_point_transformer.py [--blocks 5] [--steps 50] [--warmup 5] [--out profiles/point_transformer.jsonl]
                                              [--stamp COMMIT] [--no-model]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

from adaptpoint_amd import pointops
from adaptpoint_amd.point_transformer import PTSeg, PointTransformerLayer, StageGraph
from adaptpoint_amd.pointnext import fill_parameters_by_name
from bench_pointops import time_forms

SHAPES = [
    ("8 x 24000", [24000] * 8, 8, 32),
    ("8 x 6000", [6000] * 8, 16, 64),
    ("8 x 1500", [1500] * 8, 16, 128),
    ("32 ragged 700-1300", None, 16, 64),
]


def clouds(sizes, dev, seed):
    g = torch.Generator().manual_seed(seed)
    n = int(sum(sizes))
    p = (torch.rand(n, 3, generator=g) * 2 - 1).to(dev)
    o = torch.tensor(np.cumsum(sizes), dtype=torch.int32, device=dev)
    return p, o, g


def peak_mb(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)


def layer_lines(a, dev, head, emit):
    for name, sizes, k, C in SHAPES:
        if sizes is None:
            sizes = np.random.default_rng(5).integers(700, 1301, 32).tolist()
        p, o, g = clouds(sizes, dev, 11)
        n = p.shape[0]
        x = torch.randn(n, C, generator=g).to(dev).requires_grad_(True)
        w = torch.randn(n, C, generator=g).to(dev)
        layers = {}
        for form in ("fused", "composed", "reference"):
            torch.manual_seed(3)
            layers[form] = PointTransformerLayer(C, C, 8, k, fused=form == "fused").to(dev).train()
        graph = StageGraph(p, o, k)
        graph.csr(), graph.d

        def run(form, backward):
            layer = layers[form]
            leaves = [x, *layer.parameters()]

            def fn():
                if form == "reference":                       # two queries and a fresh grouping per call
                    pointops.knnquery(k, p, p, o, o)
                    own = StageGraph(p, o, k)
                    own.csr()
                    out = layer([p, x, o, own])
                else:
                    out = layer([p, x, o, graph])
                if not backward:
                    return [out.detach()]
                return [out.detach(), *torch.autograd.grad(out, leaves, w)]
            return fn
        for what, backward in (("fwd", False), ("fwd_bwd", True)):
            forms = {f"{form}_{what}": run(form, backward) for form in layers}
            if backward:                                      # the composed captures hold memset nodes and run eagerly:
                forms["fused_eager_fwd_bwd"] = run("fused", True)   # the fused form eagerly too, for a like-for-like ratio
            leaves = [x, *(q for layer in layers.values() for q in layer.parameters())]
            res = dict(head, batch=name, rows=n, k=k, c=C, op=f"layer_{what}")
            for key, fn in forms.items():
                res[key + "_peak_mb"] = peak_mb(fn)
            res.update(time_forms(forms, leaves, a, eager=("fused_eager_fwd_bwd",)))
            for other in ("composed", "reference"):
                res[f"speedup_over_{other}"] = round(res[f"{other}_{what}_us"] / res[f"fused_{what}_us"], 2)
            emit(res)


def model_line(a, dev, head, emit):
    sizes = [24000] * 8
    p, o, g = clouds(sizes, dev, 12)
    n = p.shape[0]
    x = torch.cat([p, torch.randn(n, 3, generator=g).to(dev)], 1)
    w = torch.randn(n, 13, generator=g).to(dev)
    models = {form: fill_parameters_by_name(PTSeg('PointTransformerBlock', [2, 3, 4, 6, 3], width=32, fused=form == "fused"))
              .to(dev).train() for form in ("fused", "composed")}

    def step(form):
        m = models[form]

        def fn():
            m.zero_grad(set_to_none=True)
            (m(p, x, o) * w).sum().backward()
        return fn
    forms = {f"{form}_step": step(form) for form in models}
    res = dict(head, batch="8 x 24000", rows=n, op="ptseg_2_3_4_6_3_w32_train_step", timing="eager")
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
    ap.add_argument("--no-model", action="store_true", help="the layer lines only")
    a = ap.parse_args()
    assert a.blocks >= 5, "medians are of at least 5 blocks"
    commit = a.stamp
    if commit is None:
        r = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True)
        commit = r.stdout.strip() if r.returncode == 0 else "unknown"
    dev = torch.device("cuda:0")
    head = dict(bench="point_transformer", commit=commit, device=torch.cuda.get_device_name(0), blocks=a.blocks)
    lines = []

    def emit(res):
        lines.append(res)
        print(json.dumps(res), flush=True)
        if a.out:                                               # written line by line: a run cut short keeps what it measured
            with open(os.path.join(ROOT, a.out) if not os.path.isabs(a.out) else a.out, "w") as fh:
                fh.writelines(json.dumps(line) + "\n" for line in lines)
    layer_lines(a, dev, head, emit)
    if not a.no_model:
        model_line(a, dev, head, emit)


if __name__ == "__main__":
    main()
