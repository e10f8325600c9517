"""Part segmentation: what the two new kernel families and the whole step cost, each against the composed form of the
same commit, alternating in ONE process, under hipGraph replay.

    python scripts/bench_partseg.py [--batch 32] [--points 2048] [--iters 100] [--warmup 10] [--only block metric step]
                                    [--out profiles/partseg.jsonl]

  block   the LAST decoder block of PointNeXt-S with cls_map 'curvenet' (cond 208, skip 32, coarse 64 -> 32 channels on
          N / N/2 points), forward + backward: `propagate(..., cond=)` against repeat + three_interpolate + cat +
          pointwise.conv_bn_act
  metric  one evaluation batch's metric: `PartMetrics.update` (replayed) against the reference's loop
          (examples/shapenetpart/train_adapt.py:77-107 and :576-580 restated: three host reads per (shape, part), one
          `.cpu()` per shape; eager, wall clock -- it cannot be captured)
  step    a whole PointNeXt-S part-segmentation training step (7 input channels, cls_map 'curvenet', Poly1 focal loss,
          clip, fused AdamW): fused + hoisted against composed (fused=False, hoisted=False); a form whose capture holds
          a memset node is timed eagerly and says so

One JSON line per case.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from adaptpoint_amd import graphs, layers, pointwise, propagation
from adaptpoint_amd.part_metrics import SHAPENETPART_CLS2PARTS, PartMetrics


def _warm(fns, n=3):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(n):
            for fn in fns:
                fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()


def _time(forms, iters, warmup):
    """forms: {name: callable}; alternating, one event pair per call -> {name: (median, p10, p90) in us}."""
    for _ in range(warmup):
        for fn in forms.values():
            fn()
    torch.cuda.synchronize()
    ev = {k: [] for k in forms}
    for _ in range(iters):
        for k, fn in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            ev[k].append((e0, e1))
    torch.cuda.synchronize()
    out = {}
    for k, pairs in ev.items():
        t = sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in pairs)
        out[k] = (round(t[len(t) // 2], 1), round(t[len(t) // 10], 1), round(t[(9 * len(t)) // 10], 1))
    return out


def _replayable(fn, leaves, what):
    """(callable, 'hipGraph replay') or, when the capture holds a memset node, (fn, 'eager')."""
    try:
        g = graphs.capture(fn, leaves=leaves, what=what)[0]
        return g.replay, "hipGraph replay", g
    except graphs.MemsetNodeInGraph:
        return fn, "eager (its capture holds a memset node)", None


def bench_block(dev, B, N, iters, warmup):
    Cc, C1, C2, O, n, m = 208, 32, 64, 32, N, N // 2
    g = torch.Generator().manual_seed(N)
    conv = torch.nn.Conv1d(Cc + C1 + C2, O, 1, bias=False).to(dev)
    bn = torch.nn.BatchNorm1d(O).to(dev)
    cond = torch.randn(B, Cc, generator=g).to(dev).requires_grad_(True)
    f1 = torch.randn(B, C1, n, generator=g).to(dev).requires_grad_(True)
    f2 = torch.randn(B, C2, m, generator=g).to(dev).requires_grad_(True)
    gout = torch.randn(B, O, n, generator=g).to(dev)
    p1 = torch.rand(B, n, 3, generator=g).to(dev)
    nearest, weights = layers.three_nn_weights(p1, p1[:, :m].contiguous())
    params = [cond, f1, f2, conv.weight, bn.weight, bn.bias]

    def conditioned():
        return torch.autograd.grad(propagation.propagate(f1, f2, nearest, weights, conv, bn, cond=cond), params, gout)

    def composed():
        x = torch.cat([cond.unsqueeze(-1).expand(-1, -1, n), f1, layers.three_interpolate(f2, nearest, weights)], dim=1)
        return torch.autograd.grad(pointwise.conv_bn_act(x.contiguous(), conv, bn), params, gout)
    assert propagation.supported(f1, f2, conv, bn, cond)
    _warm([conditioned, composed])
    keep, forms, how = [], {}, {}
    for k, fn in (("conditioned", conditioned), ("composed", composed)):
        forms[k], how[k], gr = _replayable(fn, params, k)
        keep.append(gr)
    t = _time(forms, iters, warmup)
    res = {"bench": "last part-decoder block fwd+bwd", "B": B, "N": N, "Cc": Cc, "C1": C1, "C2": C2, "O": O, "m": m}
    for k in forms:
        res.update({f"{k}_us_median": t[k][0], f"{k}_us_p10": t[k][1], f"{k}_us_p90": t[k][2], f"{k}_launch": how[k]})
    # the repeat's share of the concatenation, which the conditioned form never touches: written by the cat and read by
    # the convolution forward, read again for the weight gradient and written as an input gradient backward
    res["bytes_not_moved"] = 4 * 4 * B * Cc * n
    return res


def reference_loop(pred, target, cls, cls2parts, cls_mious, cls_nums):
    """get_ins_mious (:90-106) and validate's per-shape accumulation (:576-580), statement for statement."""
    ins_mious = []
    for shape_idx in range(pred.shape[0]):
        part_ious = []
        parts = cls2parts[cls[shape_idx]]
        for part in parts:
            pred_part = pred[shape_idx] == part
            target_part = target[shape_idx] == part
            I = torch.logical_and(pred_part, target_part).sum()
            U = torch.logical_or(pred_part, target_part).sum()
            if U == 0:
                iou = torch.tensor(100, device=pred.device, dtype=torch.float32)
            else:
                iou = I * 100 / float(U)
            part_ious.append(iou)
        ins_mious.append(torch.mean(torch.stack(part_ious)))
    for shape_idx in range(pred.shape[0]):
        cur_gt_label = int(cls[shape_idx].cpu().numpy())
        cls_mious[cur_gt_label] += ins_mious[shape_idx]
        cls_nums[cur_gt_label] += 1
    return ins_mious


def bench_metric(dev, B, N, iters, warmup):
    import time
    rng = np.random.RandomState(N)
    table = [list(p) for p in SHAPENETPART_CLS2PARTS]
    cls = torch.from_numpy(rng.randint(0, 16, B)).to(dev)
    target = torch.stack([torch.from_numpy(rng.choice(table[int(k)], N)) for k in cls.cpu()]).to(dev)
    logits = torch.randn(B, 50, N, device=dev)
    logits.scatter_add_(1, target.unsqueeze(1), 3.0 * (torch.rand(B, 1, N, device=dev) < 0.8).float())
    m = PartMetrics(table, 50, dev)
    t32, c32 = target.int(), cls.int()
    ious = torch.empty(B, device=dev)
    fn = lambda: m.update(logits, t32, c32, ious=ious)
    _warm([fn])
    replay, how, keep = _replayable(fn, (), "the part metric")
    t = _time({"kernel": replay}, iters, warmup)
    cls_mious = torch.zeros(16, device=dev)
    cls_nums = torch.zeros(16, dtype=torch.int32, device=dev)
    wall = []
    for _ in range(max(3, iters // 20)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        reference_loop(logits.max(dim=1)[1], target, cls, table, cls_mious, cls_nums)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e6)
    wall.sort()
    return {"bench": "part metric of one batch", "B": B, "N": N, "parts": 50, "kernel_us_median": t["kernel"][0],
            "kernel_us_p10": t["kernel"][1], "kernel_us_p90": t["kernel"][2], "kernel_launch": how,
            "reference_loop_wall_us_median": round(wall[len(wall) // 2], 1), "reference_loop_launch": "eager, host loop",
            "host_reads_reference": int(sum(3 * len(table[int(k)]) + 1 for k in cls.cpu())), "host_reads_kernel": 0}


def bench_step(dev, B, N, iters, warmup):
    from adaptpoint_amd.partseg import BasePartSeg, PartSegStep
    from adaptpoint_amd.pointnext import fill_parameters_by_name
    rng = torch.Generator().manual_seed(N)
    pos = torch.rand(B, N, 3, generator=rng) * 2 - 1
    pos = (pos / pos.norm(dim=-1, keepdim=True).clamp_min(1.0)).to(dev)
    x = torch.cat([pos, torch.nn.functional.normalize(torch.randn(B, N, 3, generator=rng), dim=-1).to(dev),
                   pos[:, :, 1:2] - pos[:, :, 1:2].min(1, keepdim=True)[0]], -1).transpose(1, 2).contiguous()
    data = {'pos': pos, 'x': x, 'y': torch.randint(0, 50, (B, N), generator=rng).to(dev),
            'cls': torch.randint(0, 16, (B, 1), generator=rng).to(dev)}
    res = {"bench": "PointNeXt-S part-segmentation training step", "B": B, "N": N, "in_channels": 7, "cls_map": "curvenet"}
    forms, keep = {}, []
    for name, kw in (("fused_hoisted", dict(fused=True, hoisted=True)), ("composed", dict(fused=False, hoisted=False))):
        model = fill_parameters_by_name(BasePartSeg(**kw)).to(dev)
        opt = torch.optim.AdamW(model.parameters(), lr=1e-3, weight_decay=1e-4, capturable=True, fused=True)
        step = PartSegStep(model, optimizer=opt)
        fn = lambda step=step: step(data)
        _warm([fn], 2)
        torch.cuda.reset_peak_memory_stats()
        forms[name], res[f"{name}_launch"], gr = _replayable(fn, list(model.parameters()), name)
        keep.append((model, opt, step, gr))
        forms[name]()
        torch.cuda.synchronize()
        res[f"{name}_peak_GiB"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
    t = _time(forms, iters, warmup)
    for k in forms:
        res.update({f"{k}_us_median": t[k][0], f"{k}_us_p10": t[k][1], f"{k}_us_p90": t[k][2]})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--points", type=int, nargs="+", default=[2048])
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--only", nargs="+", default=["block", "metric", "step"], choices=["block", "metric", "step"])
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    benches = {"block": bench_block, "metric": bench_metric, "step": bench_step}
    lines = []
    for N in a.points:
        for name in a.only:
            res = benches[name](dev, a.batch, N, a.iters if name != "step" else max(10, a.iters // 5), a.warmup)
            lines.append(res)
            print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "a") as fh:
            for r in lines:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
