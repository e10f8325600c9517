"""Regenerates tests/golden/voxelize_golden.npz (run in the BUILD container only):

    python tests/golden/make_golden_voxelize.py

The reference's own `voxelize` (openpoints/dataset/data_util.py, loaded in memory from its file; nothing copied) runs on
the three clouds of voxel_grid_reference.golden_scene, one call per cloud, with both hash types.  The module imports h5py
at its top and never uses it for this: an empty stand-in module is registered first.

Recorded, per cloud c (the reference orders voxels by hash key and rows by an unstable argsort, so only what does not
depend on an order is kept):
  label_c    every point's smallest same-voxel row (cloud-local) under voxelize(mode=1)
  counts_c   the sorted voxel counts
  next_c     the value of np.random.randint(0, 2**31 - 1) right after voxelize(mode=0) under np.random.seed(SEED + c):
             what a seeded script sees next -- the device form must consume the host stream in the same way
Asserted here: the two hash types give the same partition; at least 100 face points get another cell under a float32
division (so the double division is a visible part of the contract).
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402
import voxel_grid_reference as VR  # noqa: E402

OUT = os.path.join(HERE, "voxelize_golden.npz")
SEED = 31


def reference_module():
    sys.modules.setdefault("h5py", types.ModuleType("h5py"))
    spec = importlib.util.spec_from_file_location(
        "ref_data_util", os.path.join(MG.REF, "openpoints", "dataset", "data_util.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ref = reference_module()
    coord, offset = VR.golden_scene()
    out = {"voxel": np.float64(VR.VOXEL), "seed": np.int64(SEED), "offset": offset}
    moved = 0
    for c, (lo, hi) in enumerate(zip(np.concatenate([[0], offset[:-1]]), offset)):
        cloud = coord[lo:hi]
        assert cloud.dtype == np.float32 and (cloud.min(0) == 0).all()
        labels = {}
        for hash_type in ("fnv", "ravel"):
            idx_sort, voxel_idx, count = ref.voxelize(cloud.copy(), VR.VOXEL, hash_type=hash_type, mode=1)
            labels[hash_type] = (VR.partition_labels(voxel_idx, idx_sort), np.sort(count))
        assert np.array_equal(labels["fnv"][0], labels["ravel"][0]), "the two hash types disagree on the partition"
        assert np.array_equal(labels["fnv"][1], labels["ravel"][1])
        np.random.seed(SEED + c)
        picked = ref.voxelize(cloud.copy(), VR.VOXEL, mode=0)
        nxt = np.random.randint(0, 2 ** 31 - 1)
        assert len(picked) == len(labels["fnv"][1])
        f32 = np.floor(cloud / np.float32(VR.VOXEL))
        f64 = np.floor(cloud / np.array(VR.VOXEL))
        moved += int((f32 != f64).any(1).sum())
        out[f"label_{c}"] = labels["fnv"][0].astype(np.int32)
        out[f"counts_{c}"] = labels["fnv"][1].astype(np.int32)
        out[f"next_{c}"] = np.int64(nxt)
        print(f"cloud {c}: {hi - lo} points, {len(picked)} voxels, count max {labels['fnv'][1].max()}")
    assert moved >= 100, f"only {moved} face points change cell under float32 division"
    out["moved_f32"] = np.int64(moved)
    print(f"{moved} points get another cell under float32 division")
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
