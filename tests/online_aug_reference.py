"""CPU restatements of the two online augmenters (openpoints/online_aug/), written from their semantics and independent
of adaptpoint_amd's host code: PointWOLF in torch float64 from a packed set of draws, RSMix in numpy with the
reference's float64 expanded squared distance and its random draws in the reference's order.  Test infrastructure for
tests/test_online_aug_cpu.py, tests/test_gpu_online_aug.py and tests/golden/make_golden_online_aug.py."""
import math

import numpy as np
import torch


# ------------------------------------------------------------------------------------------------------------ PointWOLF
def unpack_pointwolf_draws(draws, B, M):
    """The packed layout of `PointWOLF.draw_params`: keep | axis code | degree | scale | translation | kernel code."""
    d = torch.as_tensor(np.asarray(draws, np.float32))
    sizes = [B * M * 3, B * M, B * M * 3, B * M * 3, B * M * 3, B]
    keep, code, deg, scale, trl, kcode = torch.split(d, sizes)
    return (keep.view(B, M, 3), code.view(B, M).long(), deg.view(B, M, 3), scale.view(B, M, 3), trl.view(B, M, 3),
            kcode.view(B, 1).long())


def axis_bits(code):
    return ((code.unsqueeze(-1) >> torch.arange(3)) & 1).to(torch.float64)


def pointwolf_f64(xyz, fps_idx, draws, sigma=0.5):
    """xyz (B,N,3), fps_idx (B,M) the anchors, draws packed -> the deformed, unit-sphere-scaled cloud (B,N,3) float64
    (pointwolf.py:27-54, 77-148, 165-176)."""
    x = torch.as_tensor(np.asarray(xyz)).to(torch.float64)
    idx = torch.as_tensor(np.asarray(fps_idx)).long()
    B, N, _ = x.shape
    M = idx.shape[1]
    keep, code, deg, scale, trl, kcode = (t.to(torch.float64) if t.is_floating_point() else t
                                          for t in unpack_pointwolf_draws(draws, B, M))
    axis, kax = axis_bits(code), axis_bits(kcode)
    a = x[torch.arange(B).unsqueeze(1), idx]                                   # (B,M,3)
    ang = math.pi * deg / 180.0 * keep[..., 0:1]
    s = scale * keep[..., 1:2] * axis
    s = torch.where(s == 0, torch.ones_like(s), s)
    t = trl * keep[..., 2:3] * axis
    sx, sy, sz = torch.sin(ang).unbind(-1)
    cx, cy, cz = torch.cos(ang).unbind(-1)
    R = torch.stack([cz * cy, cz * sy * sx - sz * cx, cz * sy * cx + sz * sx,
                     sz * cy, sz * sy * sx + cz * cy, sz * sy * cx - cz * sx,
                     -sy, cy * sx, cy * cx], -1).view(B, M, 3, 3)
    moved = (x.unsqueeze(1) - a.unsqueeze(2)) @ R @ torch.diag_embed(s) + t.unsqueeze(2) + a.unsqueeze(2)
    sub = (a.unsqueeze(2) - x.unsqueeze(1)) * kax.unsqueeze(2)                 # (B,M,N,3)
    w = torch.exp(-0.5 * sub.square().sum(-1) / sigma ** 2)
    z = (w.unsqueeze(-1) * moved).sum(1) / w.sum(1).unsqueeze(-1)
    z = z - z.mean(1, keepdim=True)
    return z * (0.999999 / z.norm(dim=-1).amax(-1)).view(B, 1, 1)


# ---------------------------------------------------------------------------------------------------------------- RSMix
def rsmix_distance(cloud_xyz, q, order="reference"):
    """numpy's square_distance(q, x) for one float64 query against float32 points: (-2 q.x + |q|^2) + |x|^2_f32.
    order: "reference" sums left to right; "reversed" / "exact" (math.fsum) are the rounding variants a golden must be
    indifferent to (products of two float32 values are exact in float64, so a fused multiply-add changes nothing but
    where the sums round)."""
    x = np.asarray(cloud_xyz, np.float32)
    q = np.asarray(q, np.float64)
    xd = x.astype(np.float64)
    p = [q[k] * xd[:, k] for k in range(3)]
    xx = (x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2]          # float32
    if order == "reference":
        dot, qq = (p[0] + p[1]) + p[2], (q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]
        return (-2.0 * dot + qq) + xx.astype(np.float64)
    if order == "reversed":
        dot, qq = p[0] + (p[1] + p[2]), q[0] * q[0] + (q[1] * q[1] + q[2] * q[2])
        return (-2.0 * dot + qq) + xx.astype(np.float64)
    qq = math.fsum([q[0] * q[0], q[1] * q[1], q[2] * q[2]])
    return np.array([math.fsum([-2.0 * p[0][i], -2.0 * p[1][i], -2.0 * p[2][i], qq, float(xx[i])])
                     for i in range(x.shape[0])])


def rsmix_select(cloud, qi, r2, knn_k, n_sample, order="reference"):
    """The first n_sample points (ascending index) with d <= r2 (knn_k < 0) or d <= the knn_k-th smallest d."""
    d = rsmix_distance(cloud[:, :3], cloud[qi, :3].astype(np.float64), order)
    thr = np.sort(d)[knn_k] if knn_k >= 0 else r2
    return np.nonzero(d <= thr)[0][:n_sample]


def rsmix_sets(points, cut_rad, perm, i1, i2, n_sample, knn, order="reference"):
    B = points.shape[0]
    knn_k = min(int(np.ceil(cut_rad * n_sample)), n_sample) if knn else -1
    r2 = np.float64(cut_rad) ** 2
    E = [rsmix_select(points[c], int(i1[c]), r2, knn_k, n_sample, order) for c in range(B)]
    A = [rsmix_select(points[perm[c]], int(i2[c]), r2, knn_k, n_sample, order) for c in range(B)]
    return E, A


def rsmix_np(points, label, beta=1.0, n_sample=512, knn=False, draws=None):
    """rsmix_provider.rsmix restated: points (B,N,C) float32 numpy, label (B,) -> (mixed (B,N,C) float32, lam (B,)
    float32, label_a, label_b, counts (2B,)).  Draws from numpy's global RandomState in the reference's order."""
    points = np.asarray(points, np.float32)
    B, N, C = points.shape
    if draws is None:
        cut_rad = np.random.beta(beta, beta)
        perm = np.random.choice(B, B, replace=False)
        i1 = np.random.randint(0, N, (B, 1))[:, 0]
        i2 = np.random.randint(0, N, (B, 1))[:, 0]
    else:
        cut_rad, perm, i1, i2 = draws
    E, A = rsmix_sets(points, cut_rad, perm, i1, i2, n_sample, knn)
    out = np.empty_like(points)
    lam = np.zeros(B, np.float32)
    for c in range(B):
        e, a = E[c], A[c]
        if len(e) == 0:
            out[c] = points[c]
            continue
        kept = np.delete(points[c], e, axis=0)
        if len(a) == 0:
            add = points[c][np.random.randint(0, N - len(e), size=len(e))]
        else:
            if len(e) > len(a):
                a = np.append(a, a[np.random.randint(0, len(a), size=len(e) - len(a))])
            elif len(e) < len(a):
                a = np.sort(np.random.choice(a, size=len(e), replace=False))
            add = points[perm[c]][a].copy()
            off = points[c, i1[c], :3].astype(np.float64) - points[perm[c], i2[c], :3].astype(np.float64)
            add[:, :3] = (off + add[:, :3].astype(np.float64)).astype(np.float32)
            lam[c] = np.float32(len(e) / N)
        out[c] = np.concatenate([kept, add], 0)
    label = np.asarray(label).reshape(B)
    counts = np.array([len(e) for e in E] + [len(a) for a in A])
    return out, lam, label, label[np.asarray(perm)], counts


def golden_points(seed, B=8, N=2048):
    """The golden's input: a unit-sphere cloud plus a height channel (C = 4), regenerated from its seed."""
    from adaptpoint_amd.synthetic import unit_sphere_cloud
    xyz = unit_sphere_cloud(B, N, seed)
    h = xyz[:, :, 1:2] - xyz[:, :, 1:2].min(1, keepdims=True)
    return np.ascontiguousarray(np.concatenate([xyz, h], -1).astype(np.float32))


def rsmix_reconstruct(points, erased, appended, counts_e):
    """A mixed batch from its compact golden form: per cloud the points not erased, in order, then its appended rows."""
    out = np.empty_like(points)
    at = 0
    for c in range(points.shape[0]):
        e = int(counts_e[c])
        out[c] = np.concatenate([points[c][~erased[c]], appended[at:at + e]], 0) if e else points[c]
        at += e
    return out
