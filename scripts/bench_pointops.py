"""The stacked-cloud operators (csrc/pointops.hip) against the composed PyTorch forms, per batch of clouds, alternating in
ONE process under hipGraph replay where a form captures (the method of scripts/bench_chamfer.py):

  * kNN (`pointops.knnquery`, queries = supports) against per-cloud `cdist` + `topk`;
  * furthest sampling at stride 4 (`pointops.furthestsampling`, whose host read of the offsets keeps it eager) against
    the dense `apn_furthest_point_sampling` run cloud by cloud, and a per-cloud Python loop of torch operations -- timed
    over its first PICKS picks and scaled to the full count (marked "extrapolated": the full loop is tens of thousands
    of launches);
  * grouping forward, and forward + backward (the reverse lists rebuilt in every step), against `index_select` and
    autograd's `index_add_`;
  * interpolation (k = 3, coarse -> fine) forward and forward + backward against the reference's Python loop;
  * aggregation (share 8: w_c = c / 8) forward and forward + backward against the broadcast product.

Batches: PointTransformer's stage shapes -- 8 clouds of 24 000 points with k = 8 and c = 32, 8 clouds of 6 000 points with
k = 16 and c = 64 -- and a small ragged batch, 32 clouds of 700 to 1300 points (k = 16, c = 64).

    python scripts/bench_pointops.py [--blocks 5] [--steps 50] [--warmup 5] [--out profiles/pointops.jsonl] [--stamp COMMIT]

Per batch and operator one JSON line: the median (and min / max) over `--blocks` blocks, the forms alternating.  A block is
`--steps` calls, or fewer for a slow form (at least 3; about 0.3 s per block), recorded as `<form>_steps`.  A form whose
capture holds a memset node, or that reads the host, is timed eagerly and marked so.
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

from adaptpoint_amd import graphs, pointops
from adaptpoint_amd.layers import furthest_point_sample

PICKS = 64
BATCHES = [
    ("8 x 24000", [24000] * 8, 8, 32),
    ("8 x 6000", [6000] * 8, 16, 64),
    ("32 ragged 700-1300", None, 16, 64),
]


def time_forms(forms, leaves, a, eager=()):
    """{name_us: median us per call} of the callables in `forms`; a form replays from its own hipGraph unless it is
    named in `eager` or its capture is refused."""
    res, replay, how, keep = {}, {}, {}, []
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for k, fn in list(forms.items()):
            try:
                fn()
            except RuntimeError as err:             # a form that does not take this batch is reported, not timed
                res[k + "_timing"] = f"refused: {str(err)[:120]}"
                forms = {kk: f for kk, f in forms.items() if kk != k}
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for k, fn in forms.items():
        if k in eager:
            replay[k], how[k] = fn, "eager"
            continue
        try:
            g = graphs.capture(fn, leaves=leaves, what=k)
            keep.append(g)
            replay[k], how[k] = g[0].replay, "graph"
        except graphs.MemsetNodeInGraph:
            replay[k], how[k] = fn, "eager"
    steps = {}
    for k, fn in replay.items():                    # one timed call sizes the block
        for _ in range(min(a.warmup, 2)):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        steps[k] = max(3, min(a.steps, int(0.3 / max(time.perf_counter() - t0, 1e-6))))
    ev = {k: [] for k in replay}
    for _ in range(a.blocks):                       # alternating blocks: the forms see the same clocks
        for k, fn in replay.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps[k]):
                fn()
            e1.record()
            ev[k].append((e0, e1))
    torch.cuda.synchronize()
    for k, pairs in ev.items():
        t = sorted(e0.elapsed_time(e1) * 1e3 / steps[k] for e0, e1 in pairs)
        res[k + "_us"] = round(t[len(t) // 2], 1)
        res[k + "_us_min_max"] = [round(t[0], 1), round(t[-1], 1)]
        res[k + "_steps"] = steps[k]
        if how[k] != "graph":
            res[k + "_timing"] = how[k]
    return res


def composed_knn(xyz, ranges, k):
    out = []
    for s, e in ranges:
        d, i = torch.cdist(xyz[s:e], xyz[s:e]).topk(k, dim=1, largest=False)
        out.append((i + s, d))
    return torch.cat([i for i, _ in out]), torch.cat([d for _, d in out])


def composed_fps(xyz, ranges, picks):
    """The textbook loop, per cloud: `picks` picks each."""
    out = []
    for s, e in ranges:
        p = xyz[s:e]
        dmin = torch.full((e - s,), 1e10, device=xyz.device)
        cur = torch.zeros((), dtype=torch.long, device=xyz.device)
        idx = [cur]
        for _ in range(picks - 1):
            dmin = torch.minimum(dmin, (p - p[cur]).square().sum(-1))
            cur = dmin.argmax()
            idx.append(cur)
        out.append(torch.stack(idx) + s)
    return torch.cat(out)


def fresh(idx):
    """`idx` without its cached reverse lists: a training step builds them once per index, so the timed step does too."""
    if hasattr(idx, "_apn_po_csr"):
        del idx._apn_po_csr
    return idx


def dense_fps(xyz, ranges, counts):
    return torch.cat([furthest_point_sample(xyz[s:e].unsqueeze(0), m).view(-1) + s for (s, e), m in zip(ranges, counts)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--stamp", default=None, help="the commit to record (default: git rev-parse HEAD)")
    a = ap.parse_args()
    assert a.blocks >= 5, "medians are of at least 5 blocks"
    commit = a.stamp
    if commit is None:
        r = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True)
        commit = r.stdout.strip() if r.returncode == 0 else "unknown"
    dev = torch.device("cuda:0")
    lines = []

    def emit(head, op, forms, leaves, eager=(), extra=None):
        res = dict(head, op=op)
        res.update(time_forms(forms, leaves, a, eager))
        res.update(extra or {})
        for what in ("fwd", "fwd_bwd"):
            if f"kernel_{what}_us" in res and f"composed_{what}_us" in res:
                res[f"{what}_speedup"] = round(res[f"composed_{what}_us"] / res[f"kernel_{what}_us"], 2)
        lines.append(res)
        print(json.dumps(res), flush=True)
        torch.cuda.empty_cache()

    for name, sizes, k, c in BATCHES:
        rng = np.random.default_rng(len(name))
        if sizes is None:
            sizes = [int(s) for s in rng.integers(700, 1301, 32)]
        n = sum(sizes)
        ends = np.cumsum(sizes)
        ranges = list(zip([0] + [int(e) for e in ends[:-1]], [int(e) for e in ends]))
        counts = [s // 4 for s in sizes]
        xyz = torch.from_numpy(rng.uniform(-1, 1, (n, 3)).astype(np.float32)).to(dev)
        off = torch.from_numpy(ends.astype(np.int32)).to(dev)
        noff = torch.from_numpy(np.cumsum(counts).astype(np.int32)).to(dev)
        head = {"bench": "stacked-cloud operators against composed PyTorch; hipGraph replay unless marked",
                "commit": commit, "batch": name, "n": n, "k": k, "c": c, "blocks": a.blocks}

        emit(head, "knn", {"kernel_fwd": lambda: pointops.knnquery(k, xyz, xyz, off, off),
                           "composed_fwd": lambda: composed_knn(xyz, ranges, k)}, [])

        full = max(counts)
        forms = {"kernel_fwd": lambda: pointops.furthestsampling(xyz, off, noff),
                 "dense_per_cloud_fwd": lambda: dense_fps(xyz, ranges, counts),
                 "composed_first_picks_fwd": lambda: composed_fps(xyz, ranges, PICKS)}
        res = time_forms(forms, [], a, eager=tuple(forms))
        res["composed_fwd_us"] = round(res["composed_first_picks_fwd_us"] * (sum(counts) / (PICKS * len(sizes))), 1)
        res["composed_fwd_timing"] = f"extrapolated from the first {PICKS} picks of every cloud"
        res["fwd_speedup"] = round(res["composed_fwd_us"] / res["kernel_fwd_us"], 2)
        if "dense_per_cloud_fwd_us" in res:
            res["against_dense_per_cloud"] = round(res["dense_per_cloud_fwd_us"] / res["kernel_fwd_us"], 2)
        res = dict(head, op="fps stride 4", picks_per_cloud_max=full, **res)
        lines.append(res)
        print(json.dumps(res), flush=True)

        idx = pointops.knnquery(k, xyz, xyz, off, off)[0]
        lidx = idx.long().view(-1)
        feat = torch.randn(n, c, device=dev, requires_grad=True)
        w3 = torch.randn(n, k, c, device=dev)
        emit(head, "grouping", {
            "kernel_fwd": lambda: pointops.grouping(feat.detach(), idx),
            "composed_fwd": lambda: feat.detach().index_select(0, lidx).view(n, k, c),
            "kernel_fwd_bwd": lambda: torch.autograd.grad(pointops.grouping(feat, fresh(idx)), [feat], w3),
            "composed_fwd_bwd": lambda: torch.autograd.grad(feat.index_select(0, lidx).view(n, k, c), [feat], w3)}, [feat])

        cidx = pointops.furthestsampling(xyz, off, noff).long()
        coarse = xyz[cidx].contiguous()
        cfeat = torch.randn(len(coarse), c, device=dev, requires_grad=True)
        w2 = torch.randn(n, c, device=dev)

        def composed_interp(f):
            i3, dist = pointops.knnquery(3, coarse, xyz, noff, off)
            recip = 1.0 / (dist + 1e-8)
            wgt = recip / recip.sum(1, keepdim=True)
            out = f[i3[:, 0].long()] * wgt[:, 0:1]
            for j in (1, 2):
                out = out + f[i3[:, j].long()] * wgt[:, j:j + 1]
            return out
        emit(head, "interpolation k=3 coarse->fine (both forms include the kNN)", {
            "kernel_fwd": lambda: pointops.interpolation2(coarse, xyz, cfeat.detach(), noff, off, 3),
            "composed_fwd": lambda: composed_interp(cfeat.detach()),
            "kernel_fwd_bwd": lambda: torch.autograd.grad(pointops.interpolation2(coarse, xyz, cfeat, noff, off, 3), [cfeat], w2),
            "composed_fwd_bwd": lambda: torch.autograd.grad(composed_interp(cfeat), [cfeat], w2)}, [cfeat])

        w_c = c // 8
        pos = torch.randn(n, k, c, device=dev, requires_grad=True)
        wgt = torch.randn(n, k, w_c, device=dev, requires_grad=True)

        def composed_agg(f, p, w):
            return ((f.index_select(0, lidx).view(n, k, c) + p).view(n, k, 8, w_c) * w.unsqueeze(2)).sum(1).view(n, c)
        leaves = [feat, pos, wgt]
        emit(head, "aggregation share 8", {
            "kernel_fwd": lambda: pointops.aggregation(feat.detach(), pos.detach(), wgt.detach(), idx),
            "composed_fwd": lambda: composed_agg(feat.detach(), pos.detach(), wgt.detach()),
            "kernel_fwd_bwd": lambda: torch.autograd.grad(pointops.aggregation(feat, pos, wgt, fresh(idx)), leaves, w2),
            "composed_fwd_bwd": lambda: torch.autograd.grad(composed_agg(feat, pos, wgt), leaves, w2)}, leaves)
        del feat, pos, wgt, w3, w2, idx, lidx
        torch.cuda.empty_cache()

    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            for r in lines:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
