"""Numpy statements of SimpleView's depth rasteriser (tests/test_simpleview_cpu.py, tests/test_gpu_simpleview.py,
tests/golden/make_golden_simpleview.py), stated once more from the formulas of `points2depth` / `distribute`
(openpoints/models/backbone/simpleview_util.py:60-171):

    transform  q_c = ((p0 R[0][c] + p1 R[1][c]) + p2 R[2][c]) - t[c]        left to right, no fma -- csrc/depth_views.hip's order
    project    _x = (((x / (z + eps)) * (W / H) + 1) * H) / 2,  _y = (((y / (z + eps)) + 1) * W) / 2,  eps = 1e-12
    splats     ex = ceil(_x + oi), ey = ceil(_y + oj), oi in linspace(-sx/2, sx/2 - 1, sx); valid = 0 <= ex <= H-1 and
               0 <= ey <= W-1 and 0 <= z < inf;  pixel = ex W + ey;  w = 1 / (z + eps), wv = z w
    sums       np.add.at over the valid splats in ascending (point, i, j) order: sw, sv
    finish     img = sv / (sw + (sw == 0))

in float32 (what the kernel is bit-equal to) or float64; the analytic gradient of sum(g * img) through the depth; the
exact lattice; the margin-checked clouds; the narrow model and its float64 run."""
import copy

import numpy as np
import torch

from invres_reference import rel, sample_index  # noqa: F401
from pointmlp_reference import no_dropout  # noqa: F401

NARROW_B, NARROW_N, NARROW_RES = 4, 64, 32
MARGIN = 1e-3                       # pixels: how far every pixel decision of `clouds` stays from an integer
# (H, W, size_x, size_y, N) of the fixture's random camera-frame cases, B = 3
RANDOM_SHAPES = ((8, 8, 1, 1, 40), (16, 16, 4, 4, 64), (128, 128, 1, 1, 1024), (12, 20, 2, 4, 50))
RANDOM_B = 3
GRAD_SHAPE = 1                      # the fixture holds the reference's x.grad for RANDOM_SHAPES[GRAD_SHAPE]


def narrow(**over):
    """The fixture's model: channels 4, 32 x 32 images."""
    args = dict(channels=4, resolution=NARROW_RES, num_classes=15)
    args.update(over)
    return args


def view_matrices():
    """(rot (6,3,3), trans (6,3)) float32 numpy: `PCViews`' own."""
    from adaptpoint_amd.simpleview import PCViews
    v = PCViews()
    return v.rot_mat.numpy().copy(), v.translation.numpy().reshape(-1, 3).copy()


def transform(points, rot, trans, dtype=np.float32):
    """points (B,N,3), rot (V,3,3), trans (V,3) -> (B*V,N,3), image b*V + v, in `dtype`, summed left to right."""
    p, R, T = (np.asarray(a).astype(dtype) for a in (points, rot, trans))
    p = p[:, None, :, :, None]                                            # (B,1,N,3,1)
    R = R[None, :, None, :, :]                                            # (1,V,1,3,3)
    q = ((p[..., 0, :] * R[..., 0, :] + p[..., 1, :] * R[..., 1, :]) + p[..., 2, :] * R[..., 2, :]) - T[None, :, None, :]
    return q.reshape(-1, q.shape[2], 3)


def _offsets(size, dtype):
    return np.linspace(-size / 2, size / 2 - 1, size).astype(dtype)


def _splats(q, H, W, sx, sy, dtype):
    """-> valid (B,N,sx,sy) bool, pixel (B,N,sx,sy) int64 (0 where invalid), z, w (B,N)"""
    q = np.asarray(q).astype(dtype)
    f = dtype
    x, y, z = q[..., 0], q[..., 1], q[..., 2]
    with np.errstate(all='ignore'):
        d = z + f(1e-12)
        fx = (((x / d) * f(W / H) + f(1)) * f(H)) / f(2)
        fy = (((y / d) + f(1)) * f(W)) / f(2)
        ex = np.ceil(fx[..., None] + _offsets(sx, dtype))[..., :, None]
        ey = np.ceil(fy[..., None] + _offsets(sy, dtype))[..., None, :]
        zz = z[..., None, None]
        valid = (ex >= 0) & (ex <= H - 1) & (ey >= 0) & (ey <= W - 1) & (zz >= 0) & np.isfinite(zz)
        pixel = np.where(valid, ex * W + ey, 0).astype(np.int64)
        w = f(1) / d
    return valid, pixel, z, w


def points2depth(q, H, W, sx=4, sy=4, dtype=np.float32):
    """camera-frame q (B,N,3) -> img, sw (B,H,W) in `dtype`; sw is the weight sum BEFORE its zeros become ones."""
    valid, pixel, z, w = _splats(q, H, W, sx, sy, dtype)
    B = valid.shape[0]
    sw, sv = np.zeros((B, H * W), dtype), np.zeros((B, H * W), dtype)
    with np.errstate(all='ignore'):
        wv = z * w
        for b in range(B):
            n, i, j = np.nonzero(valid[b])                                 # ascending (point, i, j)
            np.add.at(sw[b], pixel[b, n, i, j], w[b, n])
            np.add.at(sv[b], pixel[b, n, i, j], wv[b, n])
    img = sv / (sw + (sw == 0).astype(dtype))
    return img.reshape(B, H, W), sw.reshape(B, H, W)


def depth_views(points, rot, trans, H, W, sx=1, sy=1, dtype=np.float32):
    return points2depth(transform(points, rot, trans, dtype), H, W, sx, sy, dtype)


def points2depth_grad(q, g, H, W, sx=4, sy=4, dtype=np.float64):
    """d sum(g * img) / dq (B,N,3): zero in x and y; in z, per valid splat at pixel p with a = g_p / sw'_p:
    a w - (a z - a img_p) w^2   (wv = z w, w = 1 / (z + eps), img = sv / sw')."""
    valid, pixel, z, w = _splats(q, H, W, sx, sy, dtype)
    img, sw = points2depth(q, H, W, sx, sy, dtype)
    B = valid.shape[0]
    g = np.asarray(g).astype(dtype).reshape(B, -1)
    img, sw = img.reshape(B, -1), sw.reshape(B, -1)
    sw = sw + (sw == 0).astype(dtype)
    out = np.zeros(z.shape + (3,), dtype)
    with np.errstate(all='ignore'):
        for b in range(B):
            a = g[b][pixel[b]] / sw[b][pixel[b]]                           # (N,sx,sy)
            gw = -(a * img[b][pixel[b]])
            zz, ww = z[b][:, None, None], w[b][:, None, None]
            t = np.where(valid[b], a * ww - (a * zz + gw) * (ww * ww), 0)
            gz = np.zeros(z.shape[1], dtype)
            for i in range(sx):
                for j in range(sy):
                    gz = gz + t[:, i, j]
            out[b, :, 2] = gz
    return out


def depth_views_grad(points, rot, trans, g, H, W, sx=1, sy=1, dtype=np.float64):
    """d sum(g * img) / dpoints (B,N,3): dq_z of every view times R_v[:, 2], views ascending."""
    B, V = np.asarray(points).shape[0], np.asarray(rot).shape[0]
    dq = points2depth_grad(transform(points, rot, trans, dtype), g, H, W, sx, sy, dtype).reshape(B, V, -1, 3)
    R = np.asarray(rot).astype(dtype)
    out = np.zeros(np.asarray(points).shape, dtype)
    for v in range(V):
        out = out + dq[:, v, :, 2:3] * R[v, :, 2][None, None, :]
    return out


def lattice(B=3, N=48, H=8, W=8, seed=5):
    """Camera-frame points (B,N,3) float32 on which every weight, product and sum of the s = 1 rasteriser is exact:
    z in {1/2, 1, 2, 4} (some negated), _x and _y on integers and half-integers from -2 to H + 2, x = (_x 2 / H - 1) z.
    Points 0, 1, 2 of every cloud share a pixel at three depths; some points fall outside the image."""
    assert H == W and (H & (H - 1)) == 0
    rng = np.random.default_rng(seed)
    z = rng.choice(np.array([0.5, 1.0, 2.0, 4.0]), size=(B, N))
    fx = rng.integers(-4, 2 * H + 5, size=(B, N)) / 2.0
    fy = rng.integers(-4, 2 * W + 5, size=(B, N)) / 2.0
    fx[:, :3], fy[:, :3] = 3.0, 5.5
    z[:, :3] = np.array([0.5, 2.0, 4.0])
    z[:, 3::7] *= -1.0                                                    # negative depth: masked out
    fx[:, 4], fy[:, 4] = -2.0, 3.0                                        # outside, whatever the draw
    fx[:, 5], fy[:, 5] = 4.0, W + 1.5
    x, y = (fx * 2 / H - 1) * z, (fy * 2 / W - 1) * z
    q = np.stack([x, y, z], -1).astype(np.float32)
    assert np.array_equal(q.astype(np.float64), np.stack([x, y, z], -1))
    return q


def camera_points(B, N, seed):
    """Random camera-frame points (B,N,3) float32: depth in 0.3 .. 2.5 with one in ten negated, x / z and y / z in
    -1.2 .. 1.2 (a sixth of the splat centres outside the image)."""
    rng = np.random.default_rng(3000 + seed)
    z = rng.uniform(0.3, 2.5, size=(B, N))
    x, y = z * rng.uniform(-1.2, 1.2, size=(B, N)), z * rng.uniform(-1.2, 1.2, size=(B, N))
    z = np.where(rng.uniform(size=(B, N)) < 0.1, -z, z)
    return np.stack([x, y, z], -1).astype(np.float32)


def decision_margin(points, H, W):
    """(B,N): the smallest distance, in pixels, of a point's twelve view coordinates _x - 1/2, _y - 1/2 (float64) from an
    integer -- how far the s = 1 pixel decisions ceil(_x - 1/2), ceil(_y - 1/2) are from changing."""
    rot, trans = view_matrices()
    B, N = points.shape[:2]
    q = transform(points, rot, trans, np.float64).reshape(B, rot.shape[0], N, 3)
    d = q[..., 2] + 1e-12
    c = np.stack([(((q[..., 0] / d) * (W / H) + 1) * H) / 2 - 0.5, (((q[..., 1] / d) + 1) * W) / 2 - 0.5], -1)
    return np.abs(c - np.round(c)).min(axis=(1, 3))


def clouds(B, N, seed, H, W):
    """Clouds (B,N,3) float32 in the unit ball; every point whose margin (`decision_margin`) is below MARGIN is redrawn."""
    rng = np.random.default_rng(2000 + seed)

    def draw(k):
        p = rng.normal(size=(k, 3))
        p /= np.linalg.norm(p, axis=-1, keepdims=True)
        return (p * rng.uniform(0.2, 1.0, size=(k, 1))).astype(np.float32)
    pts = draw(B * N).reshape(B, N, 3)
    for _ in range(64):
        bad = decision_margin(pts, H, W) < MARGIN
        if not bad.any():
            return pts
        pts[bad] = draw(int(bad.sum()))
    raise RuntimeError("clouds: no margin after 64 redraws")


def classifier_inputs(seed=0, B=NARROW_B, N=NARROW_N, res=NARROW_RES):
    """pos (B,N,3) with the margin at `res`, labels (B,) -- from a seed."""
    pos = torch.from_numpy(clouds(B, N, seed, res, res))
    gt = torch.from_numpy(np.random.default_rng(2500 + seed).integers(0, 15, size=B))
    return pos, gt


def train_step(model, pos, gt):
    """One forward / backward of a classifier (get_logits_loss) -> logits, loss, grads {name: dL/dparam}, dpos; the
    model's BatchNorm buffers are advanced."""
    pos = pos.detach().clone().requires_grad_(True)
    model.zero_grad(set_to_none=True)
    logits, loss = model.get_logits_loss({'pos': pos}, gt)
    loss.backward()
    return {'logits': logits.detach(), 'loss': loss.detach(), 'dpos': pos.grad,
            'grads': {n: q.grad for n, q in model.named_parameters()}}


def run64(model, pos, gt=None, training=True):
    """The classifier run in float64 (a copy: the composition, every layer in double) on pos -> as `train_step`."""
    m = copy.deepcopy(model).double()
    m.encoder.set_fused(False)
    m.train(training)
    if gt is None:
        with torch.no_grad():
            return {'logits': m({'pos': pos.detach().double()})}
    return train_step(m, pos.double(), gt)
