"""The ScanObjectNN dataset side of a training batch on the GPU.

Per sample the reference's loader (openpoints/dataset/scanobjectnn/scanobjectnn.py:79-97) slices the stored cloud to
`num_points`, shuffles its rows on the train split, runs the cfg's transform chain (cfgs/scanobjectnn/default.yaml:18-25;
the classes in openpoints/transforms/point_transformer_gpu.py) and appends the height channel.  `CloudTransform` does
that for a whole batch in one launch of `apn_cloud_transform` (csrc/cloud_transform.hip) and writes (B, N, 4) =
[pos, heights], the layout `gan.ClassifierStep` and `gan.GanStep` take.

Chains: ordered subsequences of PointsToTensor, PointCloudScaling, PointCloudCenterAndNormalize, PointCloudRotation --
the train, val and vote chains of the ScanObjectNN cfgs.  Anything else is refused with NotImplementedError.

Random draws.  By default they are the reference's calls in its order, sample by sample (`draw_params`): a seeded call
reproduces the permutation, scale and rotation a single-process loader would use.  `device_draws=True` draws the same
distributions from the device generator instead (the permutation is the sorted order of per-point uniforms): no host
copy, so the call can be captured in a hipGraph.
"""
import math

import numpy as np
import torch

from .fused import _call

MAX_POINTS = 8192               # the largest resampling input gan.resample knows
CHAIN = ("PointsToTensor", "PointCloudScaling", "PointCloudCenterAndNormalize", "PointCloudRotation")
N_PARAMS = 12                   # per cloud: scale (3) | R row-major (9)
N_CLOUD_UNIFORMS = 10           # per cloud, device draws: scale (3) | mirror (3) | angle (3) | axis order (1)

# flags of apn_cloud_transform (include/adaptpoint_amd.h)
PERMUTE, SCALE, HEIGHTS_SCALED, CENTER, NORMALIZE, ROTATE, UNIFORM, ANISOTROPIC, MIRROR = (1 << k for k in range(9))


def axis_rotation(axis, theta):
    """PointCloudRotation.M(e_axis, theta) = expm(cross(eye(3), e_axis * theta)) in closed form (float64)."""
    c, s = math.cos(theta), math.sin(theta)
    i, j = (axis + 1) % 3, (axis + 2) % 3
    m = np.zeros((3, 3))
    m[axis, axis] = 1.0
    m[i, i] = m[j, j] = c
    m[i, j], m[j, i] = -s, s
    return m


class CloudTransform:
    """A ScanObjectNN cfg chain for whole batches.  `names`: the cfg list; `split`: 'train' shuffles the rows;
    `num_points`: the dataset's slice (None: all stored points); `dataset_gravity_dim`: the axis of the dataset's own
    height fallback (ScanObjectNNHardest.gravity_dim); kwargs: the cfg's `datatransforms.kwargs`, each transform taking
    the arguments it knows, as the reference's registry does."""

    def __init__(self, names, split, num_points=None, dataset_gravity_dim=1, **kwargs):
        names = list(names)
        last = -1
        for name in names:
            if name not in CHAIN:
                raise NotImplementedError(f"CloudTransform: transform {name!r} is not supported on the device (the "
                                          f"chain must be an ordered subsequence of {', '.join(CHAIN)})")
            if CHAIN.index(name) <= last:
                raise NotImplementedError(f"CloudTransform: transform {name!r} out of order (the chain must be an "
                                          f"ordered subsequence of {', '.join(CHAIN)})")
            last = CHAIN.index(name)
        self.names, self.split = names, split
        self.num_points, self.dataset_gravity_dim = num_points, int(dataset_gravity_dim)
        self.shuffle = split == 'train'
        self.scaling = "PointCloudScaling" in names
        self.center_normalize = "PointCloudCenterAndNormalize" in names
        self.rotation = "PointCloudRotation" in names
        # PointCloudScaling (point_transformer_gpu.py:136-160)
        self.scale_min, self.scale_max = np.array(kwargs.get('scale', [2. / 3, 3. / 2])).astype(np.float32)
        self.anisotropic = kwargs.get('anisotropic', True)
        self.scale_xyz = list(kwargs.get('scale_xyz', [True, True, True]))
        self.mirror = torch.from_numpy(np.array(kwargs.get('mirror', [0, 0, 0])))
        self.use_mirroring = bool(torch.sum(self.mirror > 0) != 0)
        if self.scaling and self.use_mirroring and not self.anisotropic:
            raise ValueError("PointCloudScaling: mirroring needs anisotropic=True (the reference asserts it)")
        # PointCloudCenterAndNormalize (:36-68)
        if self.center_normalize and kwargs.get('append_xyz', False):
            raise NotImplementedError("CloudTransform: PointCloudCenterAndNormalize(append_xyz=True) is not supported")
        self.centering = kwargs.get('centering', True)
        self.normalize = kwargs.get('normalize', True)
        self.gravity_dim = int(kwargs.get('gravity_dim', 2))
        # PointCloudRotation (:268-310)
        self.angle = [None if a is None else float(a) * np.pi for a in kwargs.get('angle', [0, 0, 0])]
        if len(self.angle) != 3:
            raise ValueError("PointCloudRotation: angle must hold three bounds")
        self._cfg = {}

    # ------------------------------------------------------------------------------------------------ host draws
    def draw_params(self, batch, n):
        """The reference's draws for `batch` samples of `n` points, sample by sample in its order: the row shuffle
        (train; shuffling arange(n) consumes the same numpy stream as shuffling the (n,3) rows), PointCloudScaling's
        torch.rand calls, PointCloudRotation's np.random.uniform per bounded axis and its shuffle of the three matrices.
        -> (perm (B,n) int32 or None, params (B,12) float32 = scale | R row-major), CPU tensors."""
        perm = np.empty((batch, n), np.int32) if self.shuffle else None
        params = np.zeros((batch, N_PARAMS), np.float32)
        for b in range(batch):
            if self.shuffle:
                order = np.arange(n)
                np.random.shuffle(order)
                perm[b] = order
            params[b, :3] = self._draw_scale() if self.scaling else 1.0
            params[b, 3:] = (self._draw_rotation() if self.rotation else np.eye(3, dtype=np.float32)).reshape(-1)
        return (None if perm is None else torch.from_numpy(perm)), torch.from_numpy(params)

    def _draw_scale(self):
        scale = torch.rand(3 if self.anisotropic else 1, dtype=torch.float32) * (
            self.scale_max - self.scale_min) + self.scale_min
        if self.use_mirroring:
            mirror = (torch.rand(3) > self.mirror).to(torch.float32) * 2 - 1
            scale *= mirror
        for i, s in enumerate(self.scale_xyz):
            if not s:
                scale[i] = 1
        return scale.expand(3).numpy()

    def _draw_rotation(self):
        mats = []
        for axis, bound in enumerate(self.angle):
            theta = 0
            if bound is not None:
                theta = np.random.uniform(-bound, bound)
            mats.append(axis_rotation(axis, theta))
        np.random.shuffle(mats)
        return (mats[0] @ mats[1] @ mats[2]).astype(np.float32)

    # ------------------------------------------------------------------------------------------------------ apply
    def flags(self, device_draws=False):
        f = PERMUTE if self.shuffle else 0
        if self.scaling:
            f |= SCALE | (ANISOTROPIC if self.anisotropic else 0) | (MIRROR if self.use_mirroring else 0)
        if self.center_normalize:
            f |= HEIGHTS_SCALED | (CENTER if self.centering else 0) | (NORMALIZE if self.normalize else 0)
        if self.rotation:
            f |= ROTATE
        return f | (UNIFORM if device_draws else 0)

    def heights_dim(self):
        """The gravity axis of the height channel: CenterAndNormalize's when it is in the chain, else the dataset's."""
        return self.gravity_dim if self.center_normalize else self.dataset_gravity_dim

    def __call__(self, raw, rows=None, device_draws=False, draws=None, record=False):
        """raw (S, N_raw, 3) float32 CUDA, the stored clouds (never written); rows (B,) integer CUDA tensor of clouds to
        take (None: all S, in order).  -> out (B, N, 4) = [pos, heights], N = num_points (or N_raw).
        device_draws: the draws from the device generator (capturable); draws: (perm, params) in `draw_params`'
        layout to use instead (tests); record: also return the permutation (B,N) int32 and parameters (B,12) used."""
        if not (torch.is_tensor(raw) and raw.is_cuda and raw.dtype == torch.float32 and raw.dim() == 3
                and raw.shape[2] == 3):
            raise ValueError("CloudTransform: raw must be an (S, N_raw, 3) float32 CUDA tensor")
        S, n_raw, _ = raw.shape
        n = n_raw if self.num_points is None else int(self.num_points)
        if not 0 < n <= min(n_raw, MAX_POINTS):
            raise ValueError(f"CloudTransform: needs 0 < num_points <= min(N_raw, {MAX_POINTS}) "
                             f"(got num_points={n}, N_raw={n_raw})")
        dev = raw.device
        raw = raw.contiguous()
        if rows is not None:
            if not (torch.is_tensor(rows) and rows.device == dev and rows.dim() == 1
                    and rows.dtype in (torch.int32, torch.int64)):
                raise ValueError("CloudTransform: rows must be a 1-D integer tensor on raw's device")
            rows = rows.to(torch.int32).contiguous()
            B = rows.numel()
        else:
            B = S
        if S == 0 or B == 0:
            raise ValueError("CloudTransform: needs at least one stored cloud and one row")
        flags = self.flags(device_draws and draws is None)
        perm = params = uniforms = cfg = None
        if flags & UNIFORM:
            uniforms = torch.rand(B * N_CLOUD_UNIFORMS + B * n, device=dev)
            cfg = self._cfg_on(dev)
        else:
            perm, params = self.draw_params(B, n) if draws is None else draws
            if self.shuffle:
                perm = torch.as_tensor(perm)
                if perm.shape != (B, n):
                    raise ValueError(f"CloudTransform: perm must be ({B}, {n})")
                perm = perm.to(dev, torch.int32).contiguous()
            params = torch.as_tensor(params)
            if params.shape != (B, N_PARAMS):
                raise ValueError(f"CloudTransform: params must be ({B}, {N_PARAMS})")
            params = params.to(dev, torch.float32).contiguous()
        out = torch.empty(B, n, 4, device=dev)
        perm_out = torch.empty(B, n, dtype=torch.int32, device=dev) if record else None
        params_out = torch.empty(B, N_PARAMS, device=dev) if record else None
        ptr = lambda t: None if t is None else t.data_ptr()            # noqa: E731
        _call("apn_cloud_transform", dev, B, n, n_raw, S, raw.data_ptr(), ptr(rows), flags, self.heights_dim(),
              ptr(cfg), ptr(perm), ptr(params), ptr(uniforms), ptr(perm_out), ptr(params_out), out.data_ptr())
        if record:
            return out, perm_out, params_out
        return out

    def _cfg_on(self, dev):
        """The device-draw settings, uploaded once per device (no copy inside a capture)."""
        if dev not in self._cfg:
            nan = float('nan')
            c = [float(self.scale_min), float(self.scale_max)] + [float(m) for m in self.mirror.reshape(-1)[:3]]
            c += [1.0 if s else 0.0 for s in self.scale_xyz] + [nan if a is None else a for a in self.angle]
            self._cfg[dev] = torch.tensor(c, dtype=torch.float64, device=dev)
        return self._cfg[dev]

    def __repr__(self):
        return f"CloudTransform({self.names}, split={self.split!r}, num_points={self.num_points})"


def build_transforms_from_cfg(split, datatransforms_cfg, **dataset_kwargs):
    """openpoints/transforms/transforms_factory.py:build_transforms_from_cfg on the device: the split's chain with the
    cfg's kwargs as a `CloudTransform`, or None for a missing or empty list.  dataset_kwargs: `num_points`,
    `dataset_gravity_dim` (the dataset's side of the batch)."""
    names = datatransforms_cfg.get(split, None)
    if names is None or len(names) == 0:
        return None
    kwargs = dict(datatransforms_cfg.get('kwargs', None) or {})
    return CloudTransform(names, split, **{**kwargs, **dataset_kwargs})


__all__ = ["CloudTransform", "build_transforms_from_cfg", "axis_rotation", "MAX_POINTS"]
