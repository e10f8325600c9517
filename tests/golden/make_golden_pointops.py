"""Regenerates tests/golden/pointops_golden.npz (run in the BUILD container only).

    python tests/golden/make_golden_pointops.py

The reference's own `openpoints/cpp/pointops/functions/pointops.py` is imported in memory through
`make_golden.import_reference()` -- nothing is copied -- with the compiled `pointops_cuda` module it calls replaced, in
this process, by the float64 statements of tests/pointops_reference.py, and `torch.cuda.FloatTensor` / `IntTensor`
pointed at CPU constructors (float64 / int32), and run on the scene of `pointops_reference.golden_scene`.  Recorded:
knnquery, ballquery, furthestsampling, and -- each as the loss sum(out * w) with its autograd gradients --
queryandgroup (with and without xyz), interpolation2 (with its output), subtraction and aggregation.

Asserted here, so that an fp32 kernel cannot legitimately differ (tau = 6 x 2^-24): among every query's k + 1 nearest
float64 distances consecutive relative gaps exceed 2 tau; every sampling step's best and second-best running minimum
differ by more than 2 tau; every pair's |d2 - r^2| / r^2 exceeds 2 tau for the ball query.  Seeds are walked from
`GOLDEN_FIRST_SEED` until all of these hold."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as MG  # noqa: E402
import pointops_reference as PR  # noqa: E402

F = np.float64


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _n(t):
    return t.detach().contiguous().numpy()


def _fake_module():
    """`pointops_cuda` as the float64 statements: the reference's names, argument order and in-place outputs."""
    mod = types.ModuleType("pointops_cuda")

    def knnquery_cuda(m, nsample, xyz, new_xyz, offset, new_offset, idx, dist2):
        i, d = PR.knn(nsample, _n(xyz), _n(new_xyz), _n(offset), _n(new_offset), F)
        idx.copy_(_t(i))
        dist2.copy_(_t(d))

    def ballquery_cuda(m, radius, nsample, xyz, new_xyz, offset, new_offset, idx):
        idx.copy_(_t(PR.ball(radius, nsample, _n(xyz), _n(new_xyz), _n(offset), _n(new_offset), F)))

    def furthestsampling_cuda(b, n_max, xyz, offset, new_offset, tmp, idx):
        i, t, written, _ = PR.fps_tree(_n(xyz), _n(offset), _n(new_offset), int(n_max), F, tmp=_n(tmp))
        idx[_t(written)] = _t(i)[_t(written)]
        tmp.copy_(_t(t))

    def grouping_forward_cuda(m, nsample, c, input, idx, output):
        output.copy_(_t(PR.grouping_fwd(_n(input), _n(idx), F)))

    def grouping_backward_cuda(m, nsample, c, grad_output, idx, grad_input):
        grad_input.copy_(_t(PR.grouping_bwd(_n(grad_output), _n(idx), grad_input.shape[0], F)))

    def interpolation_forward_cuda(n, c, k, input, idx, weight, output):
        output.copy_(_t(PR.interpolation_fwd(_n(input), _n(idx), _n(weight), F)))

    def interpolation_backward_cuda(n, c, k, grad_output, idx, weight, grad_input):
        grad_input.copy_(_t(PR.interpolation_bwd(_n(grad_output), _n(idx), _n(weight), grad_input.shape[0], F)))

    def subtraction_forward_cuda(n, nsample, c, input1, input2, idx, output):
        output.copy_(_t(PR.subtraction_fwd(_n(input1), _n(input2), _n(idx), F)))

    def subtraction_backward_cuda(n, nsample, c, idx, grad_output, grad_input1, grad_input2):
        g1, g2 = PR.subtraction_bwd(_n(grad_output), _n(idx), grad_input2.shape[0], F)
        grad_input1.copy_(_t(g1))
        grad_input2.copy_(_t(g2))

    def aggregation_forward_cuda(n, nsample, c, w_c, input, position, weight, idx, output):
        output.copy_(_t(PR.aggregation_fwd(_n(input), _n(position), _n(weight), _n(idx), F)))

    def aggregation_backward_cuda(n, nsample, c, w_c, input, position, weight, idx, grad_output, grad_input,
                                  grad_position, grad_weight):
        gi, gp, gw = PR.aggregation_bwd(_n(input), _n(position), _n(weight), _n(idx), _n(grad_output), F)
        grad_input.copy_(_t(gi))
        grad_position.copy_(_t(gp))
        grad_weight.copy_(_t(gw))

    for fn in (knnquery_cuda, ballquery_cuda, furthestsampling_cuda, grouping_forward_cuda, grouping_backward_cuda,
               interpolation_forward_cuda, interpolation_backward_cuda, subtraction_forward_cuda,
               subtraction_backward_cuda, aggregation_forward_cuda, aggregation_backward_cuda):
        setattr(mod, fn.__name__, fn)
    return mod


def knn_gap(k, xyz, new_xyz, offset, new_offset):
    """The smallest consecutive relative gap among every query's k + 1 nearest float64 distances, in units of tau."""
    worst = np.inf
    for q, (s, e) in enumerate(PR.query_ranges(len(new_xyz), len(xyz), offset, new_offset)):
        d = np.sort(PR.dist2(new_xyz[q:q + 1], xyz[s:e], F)[0])[:k + 1]
        if len(d) > 1:
            worst = min(worst, ((d[1:] - d[:-1]) / d[1:]).min())
    return worst / PR.TAU


def ball_gap(radius, xyz, new_xyz, offset, new_offset):
    r2 = float(np.float32(radius)) ** 2
    worst = np.inf
    for q, (s, e) in enumerate(PR.query_ranges(len(new_xyz), len(xyz), offset, new_offset)):
        if e > s:
            worst = min(worst, (np.abs(PR.dist2(new_xyz[q:q + 1], xyz[s:e], F)[0] - r2) / r2).min())
    return worst / PR.TAU


def scene_gaps(sc):
    """name -> gap in tau of every decision the golden records; all must exceed 2."""
    xyz, off, noff = sc["xyz"], sc["offset"], sc["new_offset"]
    fidx, _, _, fgap = PR.fps_tree(xyz, off, noff, max(PR.SIZES), F)
    coarse = xyz[fidx]
    radius = PR.GOLDEN_CASES["ball"][3]
    return coarse, {
        "fps": fgap / PR.TAU,
        "knn3 fine": knn_gap(3, xyz, xyz, off, off),
        "knn16": knn_gap(16, xyz, coarse, off, noff),
        "knn33": knn_gap(33, xyz, coarse, off, noff),
        "knn3 coarse": knn_gap(3, coarse, coarse, noff, noff),
        "knn3 interp": knn_gap(3, coarse, xyz, noff, off),
        "ball": ball_gap(radius, xyz, coarse, off, noff),
    }


def kept_seed(first=PR.GOLDEN_FIRST_SEED, tries=200):
    for seed in range(first, first + tries):
        gaps = scene_gaps(PR.golden_scene(seed))[1]
        if min(gaps.values()) > 2:
            return seed, gaps
        print(f"seed {seed} rejected:", {k: round(v, 2) for k, v in gaps.items() if v <= 2})
    raise SystemExit("no seed satisfies the gap conditions")


def main():
    MG.import_reference()
    sys.modules["pointops_cuda"] = _fake_module()
    torch.cuda.FloatTensor = torch.DoubleTensor          # CPU constructors, in this process only
    torch.cuda.IntTensor = torch.IntTensor
    import openpoints.cpp.pointops.functions.pointops as ref
    assert ref.pointops_cuda is sys.modules["pointops_cuda"]

    seed, gaps = kept_seed()
    print(f"seed {seed}: gaps in tau", {k: round(v, 1) for k, v in gaps.items()})
    sc = PR.golden_scene(seed)
    d = lambda name, grad=False: _t(sc[name]).double().requires_grad_(grad)
    xyz, off, noff = d("xyz"), _t(sc["offset"]), _t(sc["new_offset"])
    out = {"seed": np.int64(seed)}
    i16 = lambda t: _n(t).astype(np.int16)

    fidx = ref.furthestsampling(xyz, off, noff)
    out["fps_idx"] = i16(fidx)
    coarse = xyz[fidx.long()].contiguous()
    for name, (q, qo) in (("knn3", (xyz, off)), ("knn16", (coarse, noff)), ("knn33", (coarse, noff))):
        idx, dist = ref.knnquery(PR.GOLDEN_CASES[name][1], xyz, q, off, qo)
        out[f"{name}_idx"] = i16(idx)
        if name == "knn3":
            out[f"{name}_dist"] = _n(dist)
    out["ball_idx"] = i16(ref.ballquery(PR.GOLDEN_CASES["ball"][3], 16, xyz, coarse, off, noff))

    for name, use_xyz in (("qg_xyz", True), ("qg_feat", False)):
        a, b, f = d("xyz", True), coarse.detach().clone().requires_grad_(True), d("feat", True)
        loss = (ref.queryandgroup(16, a, b, f, None, off, noff, use_xyz=use_xyz) * d(f"w_{name}")).sum()
        loss.backward()
        out[f"{name}_loss"], out[f"{name}_gfeat"] = _n(loss), _n(f.grad)
        if use_xyz:
            out[f"{name}_gxyz"], out[f"{name}_gnew"] = _n(a.grad), _n(b.grad)

    f = d("cfeat", True)
    val = ref.interpolation2(coarse.detach(), xyz, f, noff, off, 3)
    (val * d("w_interp")).sum().backward()
    out["interp_out"], out["interp_gfeat"] = _n(val), _n(f.grad)
    val2 = ref.interpolation(coarse.detach(), xyz, f.detach(), noff, off, 3)     # the composed form: the same numbers
    assert np.abs(_n(val2) - _n(val)).max() <= 1e-12 * np.abs(_n(val)).max()

    cidx, _ = ref.knnquery(3, coarse.detach(), coarse.detach(), noff, noff)
    out["cknn3_idx"] = i16(cidx)
    a, b = d("in1", True), d("in2", True)
    loss = (ref.subtraction(a, b, cidx) * d("w_sub")).sum()
    loss.backward()
    out["sub_loss"], out["sub_g1"], out["sub_g2"] = _n(loss), _n(a.grad), _n(b.grad)
    a, p, w = d("ainp", True), d("apos", True), d("aw", True)
    val = ref.aggregation(a, p, w, cidx)
    (val * d("w_agg")).sum().backward()
    out["agg_out"], out["agg_ginp"], out["agg_gpos"], out["agg_gw"] = _n(val), _n(a.grad), _n(p.grad), _n(w.grad)

    path = os.path.join(HERE, "pointops_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
