"""Regenerates tests/golden/emd_golden.npz (run in the BUILD container only).

    python tests/golden/make_golden_emd.py

The reference's own `openpoints/cpp/emd/emd.py` (EarthMoverDistanceFunction, earth_mover_distance) is imported in memory
through `make_golden.import_reference()` -- nothing is copied -- with the compiled `emd_cuda` module it calls replaced by
the float64 statement of tests/emd_reference.py, and run in float64 on the seeded inputs of `emd_reference.GOLDEN_CASES`.
Recorded per case: the module's loss, d loss / d xyz1 and d loss / d xyz2.

The reference's Function asserts `is_cuda` on its inputs; the tensors handed to it are CPU tensors of a subclass that
answers True, which changes nothing it computes."""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as MG  # noqa: E402
import emd_reference as ER  # noqa: E402


class _OnDevice(torch.Tensor):
    is_cuda = True


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _np(t):
    return t.detach().as_subclass(torch.Tensor).numpy()


def _approxmatch_forward(xyz1, xyz2):
    return _t(ER.match64(_np(xyz1), _np(xyz2)))


def _matchcost_forward(xyz1, xyz2, match):
    return _t(ER.cost64(_np(xyz1), _np(xyz2), _np(match)))


def _matchcost_backward(grad_cost, xyz1, xyz2, match):
    return tuple(_t(g) for g in ER.grad64(_np(grad_cost), _np(xyz1), _np(xyz2), _np(match)))


def main():
    MG.import_reference()
    stand_in = types.ModuleType("emd_cuda")
    stand_in.approxmatch_forward = _approxmatch_forward
    stand_in.matchcost_forward = _matchcost_forward
    stand_in.matchcost_backward = _matchcost_backward
    sys.modules["emd_cuda"] = stand_in
    ref = importlib.import_module("openpoints.cpp.emd.emd")
    assert ref.emd_cuda is stand_in
    out = {}
    for name, (B, n, m, seed) in ER.GOLDEN_CASES.items():
        xyz1, xyz2 = ER.golden_inputs(name)
        a = _t(xyz1).double().as_subclass(_OnDevice).requires_grad_(True)
        b = _t(xyz2).double().as_subclass(_OnDevice).requires_grad_(True)
        loss = ref.earth_mover_distance()(a, b, transpose=False)
        loss.backward()
        out[f"{name}_seed"] = np.int64(seed)
        out[f"{name}_loss"] = _np(loss)
        out[f"{name}_g1"], out[f"{name}_g2"] = _np(a.grad), _np(b.grad)
        assert np.isfinite(out[f"{name}_g1"]).all() and np.isfinite(out[f"{name}_g2"]).all()
        print(f"{name}: (B,n,m) = {(B, n, m)}, seed {seed}, loss {float(out[f'{name}_loss']):.6f}, "
              f"max |g1| {np.abs(out[f'{name}_g1']).max():.3e}, max |g2| {np.abs(out[f'{name}_g2']).max():.3e}")
    path = os.path.join(HERE, "emd_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
