"""CPU restatements of adaptpoint_amd.transforms.CloudTransform with given draws (the tests' yardstick).

`restate(..., dtype=np.float64)`: the chain in float64 from the float32 clouds and the float32 parameters the
reference used, every step elementwise and the mean by math.fsum, so the result is the same on every machine.
`restate(..., dtype=np.float32)`: the kernel's own arithmetic (csrc/cloud_transform.hip): float32 scale, heights,
subtraction, norms, IEEE square root and division; the mean summed in float64 and rounded once; each rotated coordinate
summed in float64 from exact products and rounded once.
`device_params`: the kernel's mapping of device-drawn uniforms onto the permutation, scale and rotation.
"""
import math

import numpy as np

N_CLOUD_UNIFORMS = 10


def golden_clouds(seed, batch, n):
    """Seeded stand-ins for stored ScanObjectNN clouds: anisotropic, off-centre, float32 (batch, n, 3)."""
    rs = np.random.RandomState(seed)
    spread = rs.uniform(0.2, 0.8, (batch, 1, 3))
    centre = rs.uniform(-0.3, 0.3, (batch, 1, 3))
    return (rs.randn(batch, n, 3) * spread + centre).astype(np.float32)


def axis_rotation(axis, theta):
    c, s = math.cos(theta), math.sin(theta)
    i, j = (axis + 1) % 3, (axis + 2) % 3
    m = np.zeros((3, 3))
    m[axis, axis] = 1.0
    m[i, i] = m[j, j] = c
    m[i, j], m[j, i] = -s, s
    return m


def matmul3(a, b):
    """3x3 float64 product with each entry summed as (a0 b0 + a1 b1) + a2 b2 (the kernel's order)."""
    c = np.empty((3, 3))
    for r in range(3):
        for q in range(3):
            c[r, q] = (a[r, 0] * b[0, q] + a[r, 1] * b[1, q]) + a[r, 2] * b[2, q]
    return c


def device_params(u_cloud, u_point, scale=(2. / 3, 3. / 2), anisotropic=True, scale_xyz=(True, True, True),
                  mirror=None, angle=(0, 0, 0), n=None):
    """The kernel's device-draw mapping.  u_cloud (B,10) float32, u_point (B,n) float32 ->
    perm (B,n) int64, params (B,12) float32.  angle: the cfg's bounds in units of pi (None = no draw)."""
    B = u_cloud.shape[0]
    lo, hi = np.array(scale).astype(np.float32)
    d = np.float32(hi - lo)
    params = np.zeros((B, 12), np.float32)
    for b in range(B):
        u = u_cloud[b]
        sc = np.empty(3, np.float32)
        for c in range(3):
            sc[c] = (u[c] if anisotropic else u[0]) * d + lo
            if mirror is not None:
                sc[c] *= np.float32(1.0 if float(u[3 + c]) > float(mirror[c]) else -1.0)
            if not scale_xyz[c]:
                sc[c] = 1.0
        th = [0.0 if a is None else -(a * np.pi) + (a * np.pi + a * np.pi) * float(u[6 + c]) for c, a in enumerate(angle)]
        k = min(int(np.float32(u[9]) * np.float32(6.0)), 5)
        orders = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]
        m = [axis_rotation(a, th[a]) for a in orders[k]]
        params[b, :3] = sc
        params[b, 3:] = matmul3(matmul3(m[0], m[1]), m[2]).astype(np.float32).reshape(-1)
    perm = np.argsort(u_point, axis=1, kind="stable")
    return perm, params


def restate(raw, perm, params, n, *, scale=True, heights_scaled=True, center=True, normalize=True, rotate=True,
            gravity_dim=1, rows=None, dtype=np.float64):
    """raw (S, N_raw, 3) float32; perm (B,n) or None; params (B,12) float32 -> (B, n, 4) of `dtype`."""
    B = params.shape[0]
    out = np.empty((B, n, 4), dtype)
    for b in range(B):
        src = raw[b if rows is None else rows[b], :n]
        p32 = src[perm[b]] if perm is not None else src.copy()
        g_unscaled = p32[:, gravity_dim]
        s32, R32 = params[b, :3], params[b, 3:].reshape(3, 3)
        if dtype == np.float64:
            p = p32.astype(np.float64)
            if scale:
                p = p * s32.astype(np.float64)
            g = p[:, gravity_dim] if heights_scaled else g_unscaled.astype(np.float64)
            h = g - g.min()
            if center:
                p = p - np.array([math.fsum(p[:, c]) / n for c in range(3)])
            if normalize:
                p = p / np.sqrt((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2]).max()
            if rotate:
                p = _rotate64(p, R32.astype(np.float64))
        else:
            p = p32.copy()
            if scale:
                p = p * s32
            g = p[:, gravity_dim] if heights_scaled else g_unscaled
            h = g - g.min()
            if center:
                p = p - (p.astype(np.float64).sum(0) / n).astype(np.float32)
            if normalize:
                m = np.sqrt((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2]).max()
                p = p / m
            if rotate:
                p = _rotate64(p.astype(np.float64), R32.astype(np.float64)).astype(np.float32)
        out[b, :, :3] = p
        out[b, :, 3] = h
    return out


def _rotate64(p, R):
    o = np.empty_like(p)
    for r in range(3):
        o[:, r] = (p[:, 0] * R[r, 0] + p[:, 1] * R[r, 1]) + p[:, 2] * R[r, 2]
    return o


# ---- a lossless compact form of a float32 array near a float64 one: the ulp offsets of the float32 rounding
def _ordered(x32):
    b = x32.view(np.int32).astype(np.int64)
    return np.where(b >= 0, b, -(b & 0x7fffffff))


def ulp_offsets(x32, f64):
    return _ordered(np.ascontiguousarray(x32, np.float32)) - _ordered(f64.astype(np.float32))


def from_ulp_offsets(off, f64):
    o = _ordered(f64.astype(np.float32)) + off
    b = np.where(o >= 0, o, (-o) | 0x80000000).astype(np.uint32)
    return b.view(np.float32).reshape(f64.shape)
