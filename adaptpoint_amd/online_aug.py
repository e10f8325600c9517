"""The reference's two non-learned point-cloud augmenters (openpoints/online_aug/) on the GPU.

`PointWOLF`   pointwolf.py:14-179 (`PointWOLF_classversion`): per cloud, M furthest-point anchors each apply a random
              rotation / scaling / translation, the moved copies are blended by a Gaussian kernel of the distance to
              the anchors along a random axis set, and the result is scaled into the unit sphere.  Three launches:
              FPS (with the anchors' coordinates), `apn_pointwolf_params` (csrc/online_aug.hip: the draws -> one affine
              map per anchor), and `apn_deform_forward` through `augmentor.deform_normalise_mask` (the kernel the
              AdaptPoint imitator's learned version of the same deformation runs on).
`rsmix`       rsmix_provider.py:161-222: per cloud, a ball (or k-nearest set) around a random point is cut out and
              replaced by as many points of a ball around a random point of a partner cloud, moved onto the cut; the
              labels mix by the replaced fraction.  Two launches (`apn_rsmix_select`, `apn_rsmix_mix`) and ONE host sync
              (the 2B set sizes, which the count-dependent draws need) where the reference copies the whole batch to
              the host and back.

Random draws.  Both reproduce the reference's random streams where those live on the host: PointWOLF's draws are the
same torch calls on the CPU default generator in the same order (`draw_params`), RSMix's the same numpy calls on the
global RandomState (`rsmix`).  `PointWOLF(..., device_draws=True)` draws the same distributions from the device
generator instead: no host copy, so the call can be captured in a hipGraph.
"""
import numpy as np
import torch

from .augmentor import deform_normalise_mask
from .fused import _call

RSMIX_MAX_POINTS = 8192


class PointWOLF:
    """pointwolf.py:14-25 / 27-54.  Calling it on xyz (B,N,3) (CUDA, float32) returns (xyz, xyz_new)."""

    def __init__(self, w_num_anchor=4, w_sigma=0.5, w_R_range=10, w_S_range=3, w_T_range=0.25):
        self.num_anchor = w_num_anchor
        self.sigma = w_sigma
        self.R_range = (-abs(w_R_range), abs(w_R_range))
        self.S_range = (1., w_S_range)
        self.T_range = (-abs(w_T_range), abs(w_T_range))
        self.w_R_range, self.w_S_range, self.w_T_range = w_R_range, w_S_range, w_T_range
        self._ones = {}

    def draw_params(self, batch):
        """The reference's CPU-generator calls of one call, in its order (pointwolf.py:119-131, then :93 / :160):
        dropout uniforms -> bernoulli, per-anchor axis codes, degrees, scales, translations, the kernel's axis code.
        Returns them packed as `apn_pointwolf_params` reads them (float32, on the CPU)."""
        B, M = batch, self.num_anchor
        keep = torch.bernoulli(torch.Tensor(B, M, 3).uniform_(0, 1))
        code = torch.randint(1, 8, (B, M))
        deg = torch.FloatTensor(B, M, 3).uniform_(*self.R_range)
        scale = torch.FloatTensor(B, M, 3).uniform_(*self.S_range)
        trl = torch.FloatTensor(B, M, 3).uniform_(*self.T_range)
        kcode = torch.randint(1, 8, (B, 1))
        return torch.cat([keep.reshape(-1), code.reshape(-1).float(), deg.reshape(-1), scale.reshape(-1), trl.reshape(-1),
                          kcode.reshape(-1).float()])

    def params_numel(self, batch):
        return batch * (self.num_anchor * 13 + 1)

    def __call__(self, xyz, device_draws=False, draws=None):
        """xyz (B,N,3) -> (xyz, xyz_new (B,N,3)).  device_draws: the draws from the device generator (capturable);
        draws: a packed draw tensor of `draw_params`' layout to use instead (tests)."""
        if not (xyz.is_cuda and xyz.dtype == torch.float32 and xyz.dim() == 3 and xyz.shape[2] == 3):
            raise ValueError("PointWOLF: xyz must be a (B,N,3) float32 CUDA tensor (the augmenter runs on the GPU only)")
        B, N, _ = xyz.shape
        M = self.num_anchor
        if not 1 <= M <= 8 or M > N or N > 4096:
            raise ValueError(f"PointWOLF: needs 1 <= w_num_anchor <= 8 (got {M}), w_num_anchor <= N and N <= 4096 "
                             f"(got N={N}): the limits of apn_deform_forward")
        dev = xyz.device
        xyz = xyz.contiguous()
        uniform = 0
        if draws is None and device_draws:
            draws, uniform = torch.rand(self.params_numel(B), device=dev), 1
        elif draws is None:
            draws = self.draw_params(B)
        if draws.numel() != self.params_numel(B):
            raise ValueError(f"PointWOLF: draws must hold {self.params_numel(B)} numbers")
        draws = draws.to(dev, torch.float32).contiguous()
        _, anchors = self.anchors(xyz)
        lin = torch.empty(B, M, 3, 3, device=dev)
        off = torch.empty(B, M, 3, device=dev)
        kaxes = torch.empty(B, 1, 3, device=dev)
        _call("apn_pointwolf_params", dev, B, M, draws.data_ptr(), uniform, float(self.w_R_range),
              float(self.w_S_range), float(self.w_T_range), lin.data_ptr(), off.data_ptr(), kaxes.data_ptr())
        out = deform_normalise_mask(xyz, anchors, lin, off, kaxes, self._mask_of_ones(B, N, dev), self.sigma)
        return xyz, out

    def anchors(self, xyz):
        """The anchors: FPS's first `w_num_anchor` picks (the sampler behind ops.furthest_point_sampling_wrapper, one
        launch that also gathers their coordinates) -> (idx (B,M) int32, anchors (B,M,3))."""
        B, N, _ = xyz.shape
        M = self.num_anchor
        idx = torch.empty(B, M, dtype=torch.int32, device=xyz.device)
        anchors = torch.empty(B, M, 3, device=xyz.device)
        _call("apn_furthest_point_sampling_xyz", xyz.device, B, N, M, xyz.data_ptr(), None, idx.data_ptr(),
              anchors.data_ptr())
        return idx, anchors

    def _mask_of_ones(self, B, N, dev):
        key = (B, N, dev)
        if key not in self._ones:
            self._ones[key] = torch.ones(B, N, device=dev)
        return self._ones[key]


PointWOLF_classversion = PointWOLF          # the reference's name


def rsmix_draws(batch, n_points, beta):
    """The count-independent draws of rsmix_provider.rsmix (:162-174), numpy's global RandomState, its order."""
    cut_rad = np.random.beta(beta, beta)
    perm = np.random.choice(batch, batch, replace=False)
    i1 = np.random.randint(0, n_points, (batch, 1))
    i2 = np.random.randint(0, n_points, (batch, 1))
    return cut_rad, perm, i1[:, 0], i2[:, 0]


def rsmix_picks(counts, batch, n_points, n_sample):
    """The count-dependent draws (:196-206 and pts_num_ctrl :143-158), cloud by cloud in the reference's order, as
    positions: pick (B, n_sample) int32 -- into the add list, or with an empty add list into the cloud itself."""
    pick = np.zeros((batch, n_sample), np.int32)
    for c in range(batch):
        ne, na = int(counts[c]), int(counts[batch + c])
        if ne == 0:
            continue
        if na == 0:
            pick[c, :ne] = np.random.randint(0, n_points - ne, size=ne)
        elif ne > na:
            pick[c, :na] = np.arange(na)
            pick[c, na:ne] = np.random.randint(0, na, size=ne - na)
        elif ne < na:
            # np.random.choice(array of na, ne, replace=False) draws permutation(na)[:ne]: the same stream as on na
            pick[c, :ne] = np.sort(np.random.choice(na, size=ne, replace=False))
        else:
            pick[c, :ne] = np.arange(ne)
    return pick


def rsmix(points, label, beta=1.0, n_sample=512, knn=False, draws=None):
    """rsmix_provider.rsmix on the device.  points (B,N,C) float32 CUDA with xyz first, C >= 3; label (B,) or (B,1).
    -> (mixed (B,N,C), lam (B,) float32, label_a, label_b), all on the device.  draws: (cut_rad, perm, i1, i2) to use
    instead of drawing them (tests); the count-dependent draws are always made from numpy's global RandomState."""
    if not (points.is_cuda and points.dtype == torch.float32 and points.dim() == 3):
        raise ValueError("rsmix: points must be a (B,N,C) float32 CUDA tensor")
    B, N, C = points.shape
    if C < 3:
        raise ValueError(f"rsmix: needs C >= 3 channels with xyz first (got C={C})")
    if N > RSMIX_MAX_POINTS:
        raise ValueError(f"rsmix: N <= {RSMIX_MAX_POINTS} points per cloud (got N={N})")
    if not 0 < n_sample < N:
        raise ValueError(f"rsmix: needs 0 < n_sample < N (got n_sample={n_sample}, N={N})")
    dev = points.device
    points = points.contiguous()
    cut_rad, perm, i1, i2 = rsmix_draws(B, N, beta) if draws is None else draws
    perm, i1, i2 = (np.asarray(a, np.int64).reshape(B) for a in (perm, i1, i2))
    if sorted(perm.tolist()) != list(range(B)) or i1.min() < 0 or i2.min() < 0 or max(i1.max(), i2.max()) >= N:
        raise ValueError("rsmix: perm must be a permutation of the batch and i1 / i2 indices in [0, N)")
    knn_k = min(int(np.ceil(cut_rad * n_sample)), n_sample) if knn else -1
    r2 = float(np.float64(cut_rad) ** 2)
    dr = torch.from_numpy(np.concatenate([perm, i1, i2]).astype(np.int32)).to(dev)
    members = torch.empty(2 * B, n_sample, dtype=torch.int32, device=dev)
    counts = torch.empty(2 * B, dtype=torch.int32, device=dev)
    _call("apn_rsmix_select", dev, B, N, C, points.data_ptr(), dr.data_ptr(), r2, knn_k, n_sample, members.data_ptr(),
          counts.data_ptr())
    cnt = counts.cpu().numpy()                        # the one host sync: the draws below depend on the set sizes
    pick = torch.from_numpy(rsmix_picks(cnt, B, N, n_sample)).to(dev)
    mixed = torch.empty_like(points)
    lam = torch.empty(B, device=dev)
    _call("apn_rsmix_mix", dev, B, N, C, n_sample, points.data_ptr(), dr.data_ptr(), members.data_ptr(),
          counts.data_ptr(), pick.data_ptr(), mixed.data_ptr(), lam.data_ptr())
    label = label.reshape(B)
    label_b = label.index_select(0, dr[:B].long()) if label.is_cuda else label[torch.from_numpy(perm)]
    return mixed, lam, label, label_b.to(dev)


def mixed_loss(criterion, logits, label_a, label_b, lam):
    """train_pointwolf_utils.py:149-155, the per-sample loop as one expression: mean_i (1 - lam_i) L(l_i, a_i) +
    lam_i L(l_i, b_i), with `criterion` applied to each sample alone (for SmoothCrossEntropy: per-row losses)."""
    la = _per_sample(criterion, logits, label_a.long())
    lb = _per_sample(criterion, logits, label_b.long())
    return ((1 - lam) * la + lam * lb).mean()


def _per_sample(criterion, logits, gt):
    from .pointnext import SmoothCrossEntropy
    if isinstance(criterion, SmoothCrossEntropy):
        eps, n_class = criterion.label_smoothing, logits.size(1)
        one_hot = torch.zeros_like(logits).scatter(1, gt.view(-1, 1), 1)
        one_hot = one_hot * (1 - eps) + (1 - one_hot) * eps / (n_class - 1)
        return -(one_hot * torch.log_softmax(logits, dim=1)).sum(dim=1)
    return torch.stack([criterion(logits[i:i + 1], gt[i:i + 1]) for i in range(logits.shape[0])])


__all__ = ["PointWOLF", "PointWOLF_classversion", "rsmix", "rsmix_draws", "rsmix_picks", "mixed_loss"]
