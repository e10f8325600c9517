"""SimpleView's six-view depth rasteriser (csrc/depth_views.hip) against the reference's composition of the same commit,
alternating in ONE process:

  * `depth_views` under the six views at 128 x 128, forward (no_grad) and forward + backward, at
    (B, N) = (32, 1024), (32, 2048), (128, 1024), and with all 1024 points of every cloud in one pixel of every view
    (B = 32: the longest run one thread can be handed);
  * one `SimpleViewClassifier` training step (channels 16, 128 x 128, B = 32, N = 1024), fused against fused=False.

    python scripts/bench_simpleview.py [--blocks 5] [--steps 20] [--warmup 5] [--out profiles/simpleview.jsonl] [--stamp COMMIT]

Per row: the median over `--blocks` blocks of `--steps` runs each, the forms alternating; one JSON line per row.  The
kernel is replayed from a hipGraph.  The composition is replayed too where its capture holds no memset node; where it does
(its `torch.zeros(...).scatter_add(...)` fills: graphs.assert_replayable refuses them) it runs EAGERLY, the row says so
(`composed_timing`) and holds the census of that capture.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from adaptpoint_amd import graphs
from adaptpoint_amd import simpleview as SV
from adaptpoint_amd.pointnext import fill_parameters_by_name
from adaptpoint_amd.synthetic import unit_sphere_cloud

RES = 128
SHAPES = [(32, 1024), (32, 2048), (128, 1024)]


def _warm(forms):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            for fn in forms.values():
                fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()


def composed_census(fn, leaves):
    """The node census of the composition's capture, memset nodes included (the graph is never replayed)."""
    import gc
    gc.collect()
    g = graphs.new_graph()
    with torch.cuda.graph(g):
        fn()
    census = graphs.node_census(g)
    del g
    torch.cuda.synchronize()
    return census


def time_forms(forms, leaves, a):
    """{name_us: median us per call}: each form replayed from its hipGraph when it captures cleanly, eagerly otherwise."""
    _warm(forms)
    run, keep, res = dict(forms), [], {}
    for k, fn in forms.items():
        try:
            g = graphs.capture(fn, leaves=leaves, what=k)
            keep.append(g)
            run[k] = g[0].replay
            res[k + "_timing"] = "graph"
            res[k + "_census"] = g[2]
        except graphs.MemsetNodeInGraph:
            res[k + "_timing"] = "eager (its capture holds memset nodes)"
            res[k + "_census"] = composed_census(fn, leaves)
        except Exception as e:                                   # an operation capture refuses
            res[k + "_timing"] = f"eager (does not capture: {type(e).__name__})"
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
    for k, pairs in ev.items():
        t = sorted(e0.elapsed_time(e1) * 1e3 / a.steps for e0, e1 in pairs)
        res[k + "_us"] = round(t[len(t) // 2], 1)
        res[k + "_us_min_max"] = [round(t[0], 1), round(t[-1], 1)]
    return res


def one_pixel_clouds(B, N, seed):
    """Clouds on a short line through the origin (|p| < 0.002, a tenth of a pixel at 128 x 128): in every view all N points
    project into the centre pixel."""
    s = np.random.default_rng(seed).uniform(-0.002, 0.002, size=(B, N, 1))
    return np.repeat(s, 3, axis=-1).astype(np.float32) * np.array([1.0, 0.5, 0.25], np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--stamp", default=None, help="the commit to record (default: git rev-parse HEAD)")
    ap.add_argument("--only", default="views,step", help="comma-separated parts to run")
    a = ap.parse_args()
    assert a.blocks >= 5 and a.steps >= 10, "medians are of at least 5 blocks of at least 10 runs"
    commit = a.stamp
    if commit is None:
        r = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True)
        commit = r.stdout.strip() if r.returncode == 0 else "unknown"
    dev = torch.device("cuda:0")
    parts = a.only.split(",")

    def emit(res):
        if "composed_us" in res and "fused_us" in res:
            res["speedup"] = round(res["composed_us"] / res["fused_us"], 2)
        print(json.dumps(res), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as fh:
                fh.write(json.dumps(res) + "\n")

    head = {"bench": "SimpleView: fused six-view depth rasteriser against the composed form, same inputs", "commit": commit,
            "resolution": RES, "blocks": a.blocks, "steps": a.steps}
    before = dict(SV.COMPOSED_CALLS)
    views = SV.PCViews()
    rot, trans = views.matrices(dev)
    cases = [(B, N, "unit-ball clouds", unit_sphere_cloud(B, N, seed=N)) for B, N in SHAPES]
    cases.append((32, 1024, "every point of a cloud in one pixel", one_pixel_clouds(32, 1024, 1)))
    for B, N, what, cloud in (cases if "views" in parts else ()):
        p = torch.from_numpy(np.ascontiguousarray(cloud[:, :, :3], dtype=np.float32)).to(dev).requires_grad_(True)
        g = torch.randn(B * 6, RES, RES, generator=torch.Generator().manual_seed(N)).to(dev)
        form = {"fused": lambda: SV.depth_views(p, rot, trans, RES, RES),
                "composed": lambda: SV.depth_views(p, rot, trans, RES, RES, fused=False)}
        with torch.no_grad():
            occupied = int((form["fused"]() != 0).sum())

        def fwd(k):
            with torch.no_grad():
                return form[k]()
        row = dict(head, what="depth_views forward", clouds=what, B=B, N=N, occupied_pixels=occupied)
        row.update(time_forms({k: (lambda k=k: fwd(k)) for k in form}, (), a))
        emit(row)
        row = dict(head, what="depth_views forward + backward", clouds=what, B=B, N=N, occupied_pixels=occupied)
        row.update(time_forms({k: (lambda k=k: torch.autograd.grad(form[k](), [p], g)) for k in form}, [p], a))
        emit(row)
        del p, g, form
        torch.cuda.empty_cache()
    if "step" in parts:
        B, N = 32, 1024
        pos = torch.from_numpy(np.ascontiguousarray(unit_sphere_cloud(B, N, seed=N)[:, :, :3], dtype=np.float32)).to(dev)
        gt = torch.randint(0, 15, (B,), generator=torch.Generator().manual_seed(N)).to(dev)
        models = {k: fill_parameters_by_name(SV.SimpleViewClassifier(fused=k == "fused")).to(dev).train()
                  for k in ("fused", "composed")}
        params = {k: [q for q in m.parameters() if q.requires_grad] for k, m in models.items()}

        def step(k):
            logits, loss = models[k].get_logits_loss({'pos': pos}, gt)
            return torch.autograd.grad(loss, params[k], allow_unused=True)
        row = dict(head, what="SimpleView training step (forward, loss, all gradients)", B=B, N=N, channels=16)
        row.update(time_forms({k: (lambda k=k: step(k)) for k in models}, params["fused"] + params["composed"], a))
        emit(row)
    assert SV.COMPOSED_CALLS == before, "a fused call fell back"


if __name__ == "__main__":
    main()
