"""Regenerates tests/golden/chamfer_golden.npz (run in the BUILD container only).

    python tests/golden/make_golden_chamfer.py

The reference's own `openpoints/cpp/chamfer_dist/__init__.py` classes (ChamferFunction, ChamferDistanceL1 / L2 /
L2_split) are imported in memory through `make_golden.import_reference()` -- nothing is copied -- with the compiled
`chamfer` module they call replaced by the float64 statement of tests/chamfer_reference.py, and run in float64 on the
seeded inputs of `chamfer_reference.GOLDEN_CASES`.  Recorded per case: the three losses, d loss / d xyz1 and
d loss / d xyz2 for each, and the nearest indices.

Asserted here, so that an fp32 kernel cannot legitimately differ: for every point the second-smallest float64 distance
exceeds the smallest by more than 100 tau relative (tau = 6 x 2^-24), and no two points coincide (sqrt at distance 0
gives the reference's NaN gradient)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as MG  # noqa: E402
import chamfer_reference as CR  # noqa: E402


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _forward(xyz1, xyz2):
    return tuple(_t(a) for a in CR.forward64(xyz1.detach().numpy(), xyz2.detach().numpy()))


def _backward(xyz1, xyz2, idx1, idx2, grad_dist1, grad_dist2):
    (g1, _, _), (g2, _, _) = CR.backward64(xyz1.numpy(), xyz2.numpy(), idx1.numpy(), idx2.numpy(),
                                           grad_dist1.contiguous().numpy(), grad_dist2.contiguous().numpy())
    return _t(g1), _t(g2)


def _gap(a, b):
    """The smallest relative gap between the nearest and the second nearest b over the points of a, in units of tau."""
    d = np.sort(CR.dist2_64(b, a), axis=-1)
    assert (d[..., 0] > 0).all(), "coincident points: sqrt would give the reference's NaN gradient"
    if d.shape[-1] == 1:
        return np.inf
    return ((d[..., 1] - d[..., 0]) / d[..., 0]).min() / CR.TAU


def main():
    MG.import_reference()
    sys.modules["chamfer"].forward = _forward
    sys.modules["chamfer"].backward = _backward
    import openpoints.cpp.chamfer_dist as ref
    assert ref.chamfer is sys.modules["chamfer"]
    out = {}
    for name, (B, n, m, seed, ignore, _, _) in CR.GOLDEN_CASES.items():
        xyz1, xyz2, (_, keep1, keep2) = CR.golden_inputs(name)
        gap = min(_gap(xyz1[:, keep1], xyz2[:, keep2]), _gap(xyz2[:, keep2], xyz1[:, keep1]))
        assert gap > 100, f"{name}: nearest / second nearest only {gap:.0f} tau apart: reject the seed"
        print(f"{name}: (B,n,m) = {(B, n, m)}, seed {seed}, worst gap {gap:.0f} tau")
        out[f"{name}_seed"] = np.int64(seed)
        _, _, i1, i2 = CR.forward64(xyz1[:, keep1], xyz2[:, keep2])
        out[f"{name}_idx1"], out[f"{name}_idx2"] = i1, i2
        for loss, cls in zip(CR.LOSSES, (ref.ChamferDistanceL1, ref.ChamferDistanceL2, ref.ChamferDistanceL2_split)):
            a, b = _t(xyz1).double().requires_grad_(True), _t(xyz2).double().requires_grad_(True)
            value = cls(ignore_zeros=ignore)(a, b)
            pair = torch.stack(list(value)) if isinstance(value, tuple) else value
            pair.sum().backward()
            out[f"{name}_{loss}"] = pair.detach().numpy()
            out[f"{name}_{loss}_g1"], out[f"{name}_{loss}_g2"] = a.grad.numpy(), b.grad.numpy()
            assert np.isfinite(out[f"{name}_{loss}_g1"]).all() and np.isfinite(out[f"{name}_{loss}_g2"]).all()
    path = os.path.join(HERE, "chamfer_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
