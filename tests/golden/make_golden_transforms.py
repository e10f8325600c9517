"""Regenerates tests/golden/transforms_golden.npz (run in the BUILD container only):

    python tests/golden/make_golden_transforms.py

The reference's own `build_transforms_from_cfg` chains (openpoints/transforms/, imported in memory through make_golden's
stubs; nothing copied) run on CPU under fixed seeds.  h5py is not needed: the lines of ScanObjectNNHardest.__getitem__
and ScanObjectNNC.__getitem__ around the chain (slice, train shuffle, height channel) are restated here, over seeded
stand-in clouds (transforms_reference.golden_clouds).  Python >= 3.10 needs `collections.Iterable` back for
PointCloudRotation.

Cases, B = 8 clouds each, cfgs/scanobjectnn/default.yaml's kwargs (scale [0.9, 1.1], angle [0, 1, 0], gravity_dim 1):
  train   N=2048 of 2048, [PointsToTensor, PointCloudScaling, PointCloudCenterAndNormalize, PointCloudRotation], shuffled
  val     N=1024 of 1024, [PointsToTensor, PointCloudCenterAndNormalize]
  c       ScanObjectNN-C: N=2048 of 2048, the val chain
  vote    N=1024 of 1024, [PointCloudRotation] on the cloud as a tensor; heights from the dataset's fallback

Per case: the cloud seed, the numpy and torch seeds, the draws as the reference made them (perm: the rows its shuffle
took; params: the scale it multiplied by and the float32 R it rotated by), its heights (exact), its pos as ulp offsets
from the float64 restatement fed those draws (lossless: this script checks the round trip bit for bit), and the largest
distance of its pos to that restatement (`dist32`).
"""
import collections
import collections.abc
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402
import transforms_reference as R  # noqa: E402

collections.Iterable = collections.abc.Iterable          # PointCloudRotation's isinstance check (Python >= 3.10)

OUT = os.path.join(HERE, "transforms_golden.npz")
B = 8
DT = {'train': ['PointsToTensor', 'PointCloudScaling', 'PointCloudCenterAndNormalize', 'PointCloudRotation'],
      'vote': ['PointCloudRotation'],
      'val': ['PointsToTensor', 'PointCloudCenterAndNormalize'],
      'kwargs': {'scale': [0.9, 1.1], 'angle': [0.0, 1.0, 0.0], 'gravity_dim': 1}}
CASES = {  # name: (split of the chain, shuffle split, N, cloud seed, numpy seed, torch seed)
    'train': ('train', 'train', 2048, 101, 7, 11),
    'val': ('val', 'val', 1024, 102, 8, 12),
    'c': ('val', 'clean', 2048, 103, 9, 13),
    'vote': ('vote', 'val', 1024, 104, 10, 14),
}
GRAVITY = 1                                               # ScanObjectNNHardest.gravity_dim


class _Recorder:
    """Stands in for the transform module's `torch`: records what torch.rand and torch.tensor return."""

    def __init__(self):
        self.rand, self.tensor = [], []

    def __getattr__(self, k):
        return getattr(torch, k)

    def rand_(self, *a, **k):
        out = torch.rand(*a, **k)
        self.rand.append(out.clone())
        return out


def run_case(name, build, gpu_mod):
    chain_split, split, n, cloud_seed, np_seed, torch_seed = CASES[name]
    stored = R.golden_clouds(cloud_seed, B, n)
    points = stored.copy()                                # the dataset's array (the reference shuffles it in place)
    tf = build(chain_split, DT)
    rec = _Recorder()
    rec_torch = type("T", (), {"__getattr__": lambda self, k: getattr(torch, k),
                               "rand": staticmethod(rec.rand_),
                               "tensor": staticmethod(lambda *a, **k: rec.tensor.append(torch.tensor(*a, **k)) or
                                                      rec.tensor[-1].clone())})()
    gpu_mod.torch = rec_torch
    np.random.seed(np_seed)
    torch.manual_seed(torch_seed)
    perm = np.zeros((B, n), np.int64)
    out = np.empty((B, n, 4), np.float32)
    params = np.zeros((B, 12), np.float32)
    params[:, :3] = 1.0
    params[:, 3:] = np.eye(3, dtype=np.float32).reshape(-1)
    try:
        for b in range(B):
            cp = points[b][:n]                            # ScanObjectNNHardest.__getitem__ :80
            perm[b] = np.arange(n)
            if split == 'train':
                # record the shuffle's permutation: the same draws on arange(n) from the same state (and the same state
                # after), then the reference's own call on the rows
                st = np.random.get_state()
                order = np.arange(n)
                np.random.shuffle(order)
                after = np.random.get_state()
                np.random.set_state(st)
                np.random.shuffle(cp)
                assert np.array_equal(cp, stored[b][:n][order]), "arange shuffle != row shuffle"
                assert all(np.array_equal(x, y) for x, y in zip(after[1:], np.random.get_state()[1:]))
                perm[b] = order
            n_rand, n_tensor = len(rec.rand), len(rec.tensor)
            data = {'pos': cp, 'y': np.int64(0)} if chain_split != 'vote' else {'pos': torch.from_numpy(cp.copy())}
            data = tf(data)
            if len(rec.rand) > n_rand:                    # PointCloudScaling's draw, as the reference forms the scale
                sc_t = [t for t in tf.transforms if type(t).__name__ == 'PointCloudScaling'][0]
                r = rec.rand[n_rand]
                params[b, :3] = (r * (sc_t.scale_max - sc_t.scale_min) + sc_t.scale_min).expand(3).numpy()
            if len(rec.tensor) > n_tensor:                # PointCloudRotation's rot_mat
                params[b, 3:] = rec.tensor[n_tensor].numpy().reshape(-1)
            if 'heights' in data.keys():                  # :88-95 (ScanObjectNNC :84-87 has the same first branch)
                x = torch.cat((data['pos'], data['heights']), dim=1)
            else:
                x = torch.cat((data['pos'], torch.from_numpy(cp[:, GRAVITY:GRAVITY + 1]
                                                             - cp[:, GRAVITY:GRAVITY + 1].min())), dim=1)
            out[b] = x.numpy()
    finally:
        gpu_mod.torch = torch
    has_cn = 'PointCloudCenterAndNormalize' in DT[chain_split]
    kw = dict(scale='PointCloudScaling' in DT[chain_split], heights_scaled=has_cn, center=has_cn, normalize=has_cn,
              rotate='PointCloudRotation' in DT[chain_split], gravity_dim=GRAVITY)
    f64 = R.restate(stored, perm if split == 'train' else None, params, n, dtype=np.float64, **kw)
    f32 = R.restate(stored, perm if split == 'train' else None, params, n, dtype=np.float32, **kw)
    assert np.array_equal(out[:, :, 3], f32[:, :, 3]), "heights are exact float32 arithmetic"
    off = R.ulp_offsets(out[:, :, :3], f64[:, :, :3])
    assert np.abs(off).max() < 2 ** 31, np.abs(off).max()
    back = R.from_ulp_offsets(off.astype(np.int32).astype(np.int64), f64[:, :, :3])
    assert np.array_equal(back.view(np.int32), out[:, :, :3].view(np.int32)), "ulp form is not lossless"
    dist = float(np.abs(out[:, :, :3].astype(np.float64) - f64[:, :, :3]).max())
    print(f"{name}: n={n} dist32={dist:.3e} ulp offsets: max {np.abs(off).max()}, "
          f"99.9% {np.quantile(np.abs(off), 0.999):.0f}")
    res = {f"{name}_cloud_seed": cloud_seed, f"{name}_np_seed": np_seed, f"{name}_torch_seed": torch_seed,
           f"{name}_n": n, f"{name}_params": params, f"{name}_heights": out[:, :, 3].copy(),
           f"{name}_pos_ulps": off.astype(np.int32), f"{name}_dist32": dist}
    if split == 'train':
        res[f"{name}_perm"] = perm.astype(np.int16)
    return res


def main():
    MG.import_reference()
    import openpoints.transforms.point_transformer_gpu as gpu_mod
    from openpoints.transforms import build_transforms_from_cfg

    def build(split, cfg):
        tf = build_transforms_from_cfg(split, cfg)
        if not hasattr(tf, 'transforms'):                # a one-element list builds the transform itself
            tf = type("C", (), {"transforms": [tf], "__call__": lambda self, d: self.transforms[0](d)})()
        return tf
    out = {}
    for name in CASES:
        out.update(run_case(name, build, gpu_mod))
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
