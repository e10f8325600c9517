"""Regenerates tests/golden/invres_golden.npz (run in the BUILD container only):

    python tests/golden/make_golden_invres.py

The reference's own `InvResMLP` and `PointNextEncoder` (openpoints/models/backbone/pointnext.py, imported in memory
through make_golden's stubs; nothing copied) run on CPU over the oracle's index operators, with name-seeded weights
(`fill_parameters_by_name`).  Inputs are regenerated from seeds by tests/invres_reference.py and not stored.

  (a) a/...   InvResMLP(64, expansion 4) in training mode at B=4, N=512, r=0.3, K=32, loss (out * w).sum(): the output
              and dL/df at a name-seeded sample of 16384 entries (`invres_reference.sample_index`), dL/dp, every
              parameter's gradient (sampled beyond 8192 entries; a/grad64/: the 1-D ones once more from the reference
              run in float64, see _vector_grads64) and the BatchNorm buffers after the step;
              a/err64: the reference's own distance to the float64 restatement; ab/seed: the input seed (the first
              whose gates and pool winners float32 and float64 decide alike, see main)
  (b) b/...   the same block with the signs of every third gamma of convs.convs.0.1 flipped
  (c) c/...   a narrow encoder (invres_reference.NARROW) at B=2, N=512 in eval mode: forward_cls_feat and every level of
              forward_seg_feat
  (d) d/...   the name -> shape list of the encoder built with PointNeXt-B's settings (invres_reference.POINTNEXT_B)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402
import invres_reference as R  # noqa: E402

OUT = os.path.join(HERE, "invres_golden.npz")
KEEP_ACT = 16384


def _args(EasyDict, **group):
    return dict(aggr_args={'feature_type': 'dp_fj', 'reduction': 'max'},
                group_args=EasyDict(NAME='ballquery', normalize_dp=True, **group),
                conv_args={'order': 'conv-norm-act'}, act_args={'act': 'relu'}, norm_args={'norm': 'bn'})


def block_case(ref_pn, EasyDict, tag, flip, seed):
    from adaptpoint_amd.pointnext import fill_parameters_by_name
    c = R.BLOCK
    blk = fill_parameters_by_name(ref_pn.InvResMLP(c['C'], expansion=c['expansion'],
                                                   **_args(EasyDict, radius=c['radius'], nsample=c['nsample'])))
    if flip:
        R.flip_every_third_gamma(blk)
    blk.train()
    p, f, w = R.block_inputs(c['B'], c['N'], c['C'], seed)
    p.requires_grad_(True)
    f.requires_grad_(True)
    _, out = blk([p, f.clone()])               # (the reference adds the identity in place)
    (out * w).sum().backward()
    res = {f"{tag}/out": out.detach().numpy().ravel()[R.sample_index(f"{tag}/out", out.numel(), KEEP_ACT)],
           f"{tag}/df": f.grad.numpy().ravel()[R.sample_index(f"{tag}/df", f.numel(), KEEP_ACT)],
           f"{tag}/dp": p.grad.numpy()}
    for n, q in blk.named_parameters():
        res[f"{tag}/grad/{n}"] = q.grad.numpy().ravel()[R.sample_index(n, q.numel())]
    for n, b in blk.named_buffers():
        res[f"{tag}/buf/{n}"] = b.numpy()
    res.update(_vector_grads64(blk, p, f, w, tag))
    # the reference's own distance to float64 (the mirror shares the reference's names, so it carries its weights)
    from adaptpoint_amd.pointnext import InvResMLP
    from oracle import oracle as O
    mirror = fill_parameters_by_name(InvResMLP(c['C'], expansion=c['expansion'],
                                               group_args=dict(NAME='ballquery', normalize_dp=True, radius=c['radius'],
                                                               nsample=c['nsample'])))
    if flip:
        R.flip_every_third_gamma(mirror)
    idx = torch.from_numpy(O.ball_query(c['radius'], c['nsample'], p.detach().numpy(), p.detach().numpy()))
    r64 = R.run_invres64(mirror, p.detach(), f.detach(), idx, w)
    errs = (R.rel(out, r64['out']), R.rel(f.grad, r64['df']), R.rel(p.grad, r64['dp']))
    print(f"{tag} (seed {seed}): reference fp32 against float64: out {errs[0]:.2e} dL/df {errs[1]:.2e} dL/dp {errs[2]:.2e}")
    res[f"{tag}/err64"] = np.array(errs)
    return res


def _vector_grads64(blk, p, f, w, tag):
    """The gradients of the block's 1-D parameters (BatchNorm gamma / beta) from the reference module itself run in
    float64.  They are per-channel sums over every position with heavy cancellation: the reference's own float32 values
    sit up to 3e-5 from them (printed), which says nothing about a restatement in float64 -- so the fixture carries
    both.  Index operators for the float64 run: the oracle's ball query on the float32 coordinates, a torch gather."""
    import copy
    ref_group = MG.import_reference()[0]
    blk64 = copy.deepcopy(blk).double()
    blk64.zero_grad()
    saved = ref_group.ball_query, ref_group.grouping_operation
    ref_group.ball_query = lambda r, k, xyz, new_xyz: saved[0](r, k, xyz.float(), new_xyz.float())
    ref_group.grouping_operation = lambda x, idx: x.unsqueeze(2).expand(-1, -1, idx.shape[1], -1).gather(
        3, idx.long().unsqueeze(1).expand(-1, x.shape[1], -1, -1))
    try:
        _, out = blk64([p.detach().double(), f.detach().double()])
        (out * w.double()).sum().backward()
    finally:
        ref_group.ball_query, ref_group.grouping_operation = saved
    res, worst = {}, 0.0
    for (n, q), (_, q32) in zip(blk64.named_parameters(), blk.named_parameters()):
        if q.dim() == 1:
            res[f"{tag}/grad64/{n}"] = q.grad.numpy()
            worst = max(worst, R.rel(q32.grad, q.grad))
    print(f"{tag}: the reference's float32 gamma / beta gradients against its own float64 run: worst {worst:.2e}")
    return res


def encoder_case(ref_pn, EasyDict):
    from adaptpoint_amd.pointnext import fill_parameters_by_name
    cfg = dict(R.NARROW)
    enc = fill_parameters_by_name(ref_pn.PointNextEncoder(sa_layers=1, **cfg, **_args(EasyDict))).eval()
    pos = torch.from_numpy(R.GI.unit_sphere_cloud(2, 512, seed=931))
    x = torch.cat([pos, MG.height_channel(pos)], -1).transpose(1, 2).contiguous()
    res = {}
    with torch.no_grad():
        res["c/cls"] = enc.forward_cls_feat(pos, x.clone()).numpy()
        ps, fs = enc.forward_seg_feat(pos, x.clone())
    for i, (p, f) in enumerate(zip(ps, fs)):
        res[f"c/p{i}"], res[f"c/f{i}"] = p.numpy(), f.numpy()
    res["c/radii"] = np.array([r for st in enc.radii for r in st])
    return res


def shapes_case(ref_pn, EasyDict):
    enc = ref_pn.PointNextEncoder(**R.POINTNEXT_B, **_args(EasyDict))
    sd = enc.state_dict()
    res = {"d/names": np.array(list(sd.keys())),
           "d/shapes": np.array([",".join(str(s) for s in t.shape) for t in sd.values()])}
    # _to_full_list for a scalar and for a nested list (radius and nsample per block)
    res["d/radii_scalar"] = np.array([r for st in enc.radii for r in st])
    nested = ref_pn.PointNextEncoder(**dict(R.POINTNEXT_B, radius=[[0.1], [0.1, 0.2], [0.2, 0.3, 0.4], [0.4], [0.8, 1.0]],
                                            nsample=[[16], [32], [32, 24], [16], [8]]), **_args(EasyDict))
    res["d/radii_nested"] = np.array([r for st in nested.radii for r in st])
    res["d/nsample_nested"] = np.array([r for st in nested.nsample for r in st])
    return res


def main():
    _, ref_pn, _ = MG.import_reference()
    from easydict import EasyDict
    out = {}
    # A ReLU gate or a pool winner that float32 rounding decides differently from float64 moves a gradient by ~1e-3 of
    # its norm (one entry in 131072): such an input says nothing about arithmetic, and its seed is rejected -- as
    # make_golden.py rejects seeds without a margin.  The accepted seed is stored.
    for seed in range(16):
        cases = {**block_case(ref_pn, EasyDict, "a", False, seed), **block_case(ref_pn, EasyDict, "b", True, seed)}
        if max(cases["a/err64"].max(), cases["b/err64"].max()) < 2e-6:
            break
    else:
        raise SystemExit("no seed with a margin")
    out.update(cases)
    out["ab/seed"] = np.int64(seed)
    out.update(encoder_case(ref_pn, EasyDict))
    out.update(shapes_case(ref_pn, EasyDict))
    out = {k: (v.astype(np.float32) if isinstance(v, np.ndarray) and v.dtype == np.float64 and not k.endswith("err64")
               and "radii" not in k and "/grad64/" not in k else v) for k, v in out.items()}
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
