"""PointViT's head-dim-64 attention kernel (csrc/token_attention.hip) against the reference's composition of the same
commit, alternating in ONE process:

  * the attention core on a packed qkv (B, T, 3*6*64), forward (no_grad) and forward + backward, at
    (B, T) = (32, 65), (32, 129), (32, 257), (8, 1025), (2, 4097): `token_attention` against `token_attention.composed`
    (which materialises (B,H,T,T) twice), and -- recorded as information, not as a bar -- torch's
    `scaled_dot_product_attention` in float32 where the installed torch runs it on this device;
  * one `Block` (dim 384, 6 heads) at (32, 65) and (32, 257), forward + backward, fused against fused=False;
  * a whole PointViT-S training step (dim 384, depth 12, 6 heads; B = 32, N = 1024; 64 and 256 groups of 32), index
    handed in, fused against fused=False, with the peak allocated memory of one eager step of each form.

    python scripts/bench_pointvit.py [--blocks 5] [--steps 20] [--warmup 5] [--out profiles/pointvit.jsonl] [--stamp COMMIT]

Per row: the median over `--blocks` blocks of `--steps` runs each, the forms alternating; one JSON line per row.  All
forms of a row are timed the same way: from hipGraph replay when ALL capture, eagerly otherwise (the row says which).
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import torch.nn.functional as F

from adaptpoint_amd import graphs
from adaptpoint_amd import token_attention as TA
from adaptpoint_amd.pointnext import fill_parameters_by_name
from adaptpoint_amd.pointvit import Block, PointVitClassifier
from adaptpoint_amd.synthetic import seeded_normal, unit_sphere_cloud

H = 6
CORE_SHAPES = [(32, 65), (32, 129), (32, 257), (8, 1025), (2, 4097)]


def time_forms(forms, leaves, a):
    """{name_us: median us per call} of the callables in `forms`, all replayed from hipGraphs when all capture, all run
    eagerly otherwise."""
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


def sdpa(qkv, heads):
    B, T, C3 = qkv.shape
    q, k, v = qkv.reshape(B, T, 3, heads, C3 // (3 * heads)).permute(2, 0, 3, 1, 4).unbind(0)
    return F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B, T, C3 // 3)


def sdpa_runs(dev):
    """Whether the installed torch runs scaled_dot_product_attention in float32 on this device (forward + backward)."""
    try:
        x = torch.randn(1, 65, 3 * H * 64, device=dev, requires_grad=True)
        sdpa(x, H).sum().backward()
        torch.cuda.synchronize()
        return True
    except Exception as e:
        print(f"scaled_dot_product_attention does not run in float32 here: {type(e).__name__}: {e}", file=sys.stderr)
        return False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--stamp", default=None, help="the commit to record (default: git rev-parse HEAD)")
    ap.add_argument("--only", default="core,block,step", help="comma-separated parts to run")
    a = ap.parse_args()
    assert a.blocks >= 5 and a.steps >= 10, "medians are of at least 5 blocks of at least 10 runs"
    commit = a.stamp
    if commit is None:
        r = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True)
        commit = r.stdout.strip() if r.returncode == 0 else "unknown"
    dev = torch.device("cuda:0")
    lines = []
    parts = a.only.split(",")

    def emit(res):
        if "composed_us" in res and "fused_us" in res:
            res["speedup"] = round(res["composed_us"] / res["fused_us"], 2)
        lines.append(res)
        print(json.dumps(res), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as fh:
                fh.write(json.dumps(res) + "\n")

    head = {"bench": "PointViT: head-dim-64 token attention against the composed form, same inputs", "commit": commit,
            "H": H, "blocks": a.blocks, "steps": a.steps}
    with_sdpa = "core" in parts and sdpa_runs(dev)
    before = dict(TA.COMPOSED_CALLS)
    for B, T in (CORE_SHAPES if "core" in parts else ()):
        qkv = torch.from_numpy(seeded_normal((B, T, 3 * H * 64), T)).float().to(dev).requires_grad_(True)
        g = torch.from_numpy(seeded_normal((B, T, H * 64), T + 1)).float().to(dev)
        core = {"fused": lambda: TA.token_attention(qkv, H), "composed": lambda: TA.composed(qkv, H)}
        if with_sdpa:
            core["sdpa"] = lambda: sdpa(qkv, H)

        def fwd(k):
            with torch.no_grad():
                return core[k]()
        row = dict(head, what="attention core forward", B=B, T=T)
        row.update(time_forms({k: (lambda k=k: fwd(k)) for k in core}, (), a))
        row["composed_score_bytes"] = 2 * 4 * B * H * T * T
        emit(row)
        row = dict(head, what="attention core forward + backward", B=B, T=T)
        row.update(time_forms({k: (lambda k=k: torch.autograd.grad(core[k](), [qkv], g)) for k in core}, [qkv], a))
        emit(row)
        del qkv, g, core
        torch.cuda.empty_cache()
    for B, T in ((32, 65), (32, 257)) if "block" in parts else ():
        blocks = {k: fill_parameters_by_name(Block(384, H, fused=k == "fused")).to(dev).train() for k in ("fused", "composed")}
        x = torch.from_numpy(seeded_normal((B, T, 384), T + 2)).float().to(dev).requires_grad_(True)
        g = torch.from_numpy(seeded_normal((B, T, 384), T + 3)).float().to(dev)
        leaves = {k: [x] + list(m.parameters()) for k, m in blocks.items()}
        row = dict(head, what="Block forward + backward", B=B, T=T, dim=384)
        row.update(time_forms({k: (lambda k=k: torch.autograd.grad(blocks[k](x), leaves[k], g)) for k in blocks},
                              leaves["fused"] + leaves["composed"], a))
        emit(row)
        del blocks, x, g, leaves
        torch.cuda.empty_cache()
    B, N = 32, 1024
    for groups in (64, 256) if "step" in parts else ():
        pos = torch.from_numpy(unit_sphere_cloud(B, N, seed=N)).to(dev)
        height = pos[:, :, 1:2] - pos[:, :, 1:2].min(1, keepdim=True)[0]
        feats = torch.cat([pos, height], -1).transpose(1, 2).contiguous()
        gt = torch.randint(0, 15, (B,), generator=torch.Generator().manual_seed(N)).to(dev)
        cfg = dict(embed_dim=384, depth=12, num_heads=H,
                   embed_args=dict(NAME='PointPatchEmbed', sample_ratio=groups / N, group_size=32, group='knn',
                                   feature_type='fj', norm_args={'norm': 'in2d'}))
        models = {k: fill_parameters_by_name(PointVitClassifier(fused=k == "fused", **cfg)).to(dev).train()
                  for k in ("fused", "composed")}
        index = models["fused"].encoder.patch_embed.index(pos)
        params = {k: [q for q in m.parameters() if q.requires_grad] for k, m in models.items()}

        def step(k):
            logits, loss = models[k].get_logits_loss({'pos': pos, 'x': feats}, gt, index=index)
            return torch.autograd.grad(loss, params[k], allow_unused=True)
        row = dict(head, what="PointViT-S training step (forward, loss, all gradients)", B=B, N=N, T=groups + 1, group_size=32)
        row.update(time_forms({k: (lambda k=k: step(k)) for k in models}, params["fused"] + params["composed"], a))
        for k in models:
            row[k + "_peak_bytes"] = peak_bytes(lambda k=k: step(k))
        emit(row)
        del models, index, params
        torch.cuda.empty_cache()
    assert TA.COMPOSED_CALLS == before, "a fused call fell back"


if __name__ == "__main__":
    main()
