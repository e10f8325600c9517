"""Regenerates tests/golden/randla_golden.npz (run in the BUILD container only):

    python tests/golden/make_golden_randla.py

The reference's own `RandLANet` (openpoints/models/backbone/randlenet.py) is imported in memory through
`make_golden.import_reference()`'s stubs -- nothing is copied.  The library it takes its neighbours from
(`torch_points` / `torch_points_kernels`) is not installed here: a stand-in module is put in its place, in this process,
whose `knn(support, query, k)` is `tests/knn_reference.knn` on float32 coordinates (direct differences, ties to the
smaller index, SQUARED distances: randla_reference.knn_standin).  THE STAND-IN IS OURS: these goldens pin the network --
its operator sequence, parameter names, BatchNorm bookkeeping and its place in the host random stream -- and not that
library, whose distance convention could not be checked.

The run is on the CPU (device=cpu) with name-seeded weights (`fill_parameters_by_name`) and dropout off, at
randla_reference.MODEL (d_in 6, 5 classes, 8 neighbours, decimation 2), B 2, N 256: levels of 256 / 128 / 64 / 32 points.

  train/...  after torch.manual_seed, in training mode: the permutation the forward drew, logits, the BatchNorm buffers
             after the step, every parameter's gradient of the summed cross-entropy (sampled beyond 8192 entries:
             randla_reference.sample_index), the next torch.rand(1), the graphs of every level, err64/<tensor>: the
             reference's own relative distance to a float64 rerun, dead/<layer>: the norm of each dead block of the
             score weight's gradient relative to its A_hh block (asserted <= 1e-4 here)
  eval/...   the same in eval mode: permutation and logits
  names, shapes: the state_dict's"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as MG  # noqa: E402
import randla_reference as R  # noqa: E402

OUT = os.path.join(HERE, "randla_golden.npz")
DEAD_BAR = 1e-4


def import_reference(calls):
    MG.import_reference()

    def knn(support, query, k):
        idx, dist = R.knn_standin(support, query, k)
        calls.append((support.shape[1], query.shape[1], k, idx))
        return idx, dist.to(support.dtype)
    for name in ("torch_points", "torch_points_kernels"):
        m = types.ModuleType(name)
        m.knn = knn
        sys.modules[name] = m
    import openpoints.models.backbone.randlenet as ref
    return ref


def build(ref, dtype=torch.float32):
    from adaptpoint_amd.pointnext import fill_parameters_by_name
    model = fill_parameters_by_name(ref.RandLANet(device=torch.device('cpu'), **R.MODEL))
    model.fc_end[2].p = 0.0                      # dropout off
    return model.to(dtype)


def step(model, x, labels):
    torch.manual_seed(R.MODEL_SEED)
    state = torch.get_rng_state()
    perm = torch.randperm(x.shape[1])            # what the forward is about to draw
    torch.set_rng_state(state)
    logits = model(x)
    R.model_loss(logits, labels).backward()
    return perm, logits.detach(), float(torch.rand(1))


def main():
    calls = []
    ref = import_reference(calls)
    x, labels = R.model_inputs()
    out = {}

    model = build(ref).train()
    perm, logits, nxt = step(model, x, labels)
    out["train/perm"], out["train/logits"], out["train/next_rand"] = perm.numpy(), logits.numpy(), np.float64(nxt)
    grads = {n: p.grad for n, p in model.named_parameters()}
    for n, g in grads.items():
        out[f"train/grad/{n}"] = g.numpy().ravel()[R.sample_index(n, g.numel())]
    for n, b in model.named_buffers():
        out[f"train/buf/{n}"] = b.numpy().copy()
    levels = len(model.encoder)
    enc = [c for c in calls if c[2] == R.MODEL['num_neighbors']]
    dec = [c for c in calls if c[2] == 1]
    assert len(enc) == levels and len(dec) == levels
    for i, c in enumerate(enc):
        out[f"train/graph/encoder{i}"] = c[3].numpy().astype(np.int16)
    for i, c in enumerate(dec):
        out[f"train/graph/decoder{i}"] = c[3].numpy().astype(np.int16)

    worst = 0.0
    for n, g in grads.items():
        if n.endswith("score_fn.0.weight"):
            C = g.shape[0] // 2
            hh = g[:C, :C].norm().item()
            dead = [g[:C, C:].norm().item() / hh, g[C:, :C].norm().item() / hh, g[C:, C:].norm().item() / hh]
            out[f"train/dead/{n}"] = np.array(dead)
            worst = max(worst, *dead)
    assert worst <= DEAD_BAR, f"a dead block of a score weight has a gradient of {worst:.1e} of its A_hh block"

    model64 = build(ref, torch.float64).train()
    perm64, logits64, _ = step(model64, x.double(), labels)
    assert torch.equal(perm, perm64)
    out["train/err64/logits"] = np.float64(R.rel(logits, logits64))
    for n, p in model64.named_parameters():
        out[f"train/err64/grad/{n}"] = np.float64(R.rel(grads[n], p.grad))
    for n, b in model64.named_buffers():
        if not n.endswith("num_batches_tracked"):
            out[f"train/err64/buf/{n}"] = np.float64(R.rel(dict(model.named_buffers())[n], b))
    errs = [float(v) for k, v in out.items() if k.startswith("train/err64/")]
    print(f"reference fp32 against float64: logits {float(out['train/err64/logits']):.1e}, median {np.median(errs):.1e}, "
          f"max {max(errs):.1e}; worst dead block {worst:.1e}")

    model_e = build(ref).eval()
    with torch.no_grad():
        torch.manual_seed(R.MODEL_SEED)
        state = torch.get_rng_state()
        out["eval/perm"] = torch.randperm(x.shape[1]).numpy()
        torch.set_rng_state(state)
        out["eval/logits"] = model_e(x).numpy()

    sd = model.state_dict()
    out["names"] = np.array(list(sd.keys()))
    out["shapes"] = np.array([",".join(str(s) for s in t.shape) for t in sd.values()])
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes, {len(out)} members)")


if __name__ == "__main__":
    main()
