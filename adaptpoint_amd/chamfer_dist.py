"""Chamfer distance on the device: the reference's compiled `chamfer` module and the classes of its
`openpoints/cpp/chamfer_dist/__init__.py` over csrc/chamfer.hip.

`forward` / `backward` have the signatures and return order of the reference's extension (chamfer_cuda.cpp):

    forward(xyz1 (B,n,3), xyz2 (B,m,3))                      -> dist1 (B,n), dist2 (B,m), idx1 (B,n), idx2 (B,m)
    backward(xyz1, xyz2, idx1, idx2, grad_dist1, grad_dist2) -> grad_xyz1 (B,n,3), grad_xyz2 (B,m,3)

with squared distances, int32 indices (the smallest index among equally near points) and a gradient that is summed in
one fixed order without float atomics (include/adaptpoint_amd.h states both exactly): two runs give the same bits.  One
launch each, both directions; no (B,n,m) tensor exists.  `ChamferFunction` and the three modules keep the reference's
names, constructor argument and arithmetic; their reductions (sqrt, mean) stay on PyTorch.

The top-level `chamfer.py` of the repository is still the inert stand-in.
"""
import torch
from torch.autograd.function import once_differentiable

CHAMFER_MAX_POINTS = 65536          # = apn_chamfer_max_points()
_MAX_ROWS = 2 ** 24                 # B * max(n, m) stays below this


def _shape_problem(xyz1, xyz2):
    """Why the kernels do not take clouds of these shapes (None: they do).  Device and dtype are checked elsewhere."""
    if xyz1.dim() != 3 or xyz2.dim() != 3 or xyz1.shape[2] != 3 or xyz2.shape[2] != 3:
        return f"clouds must be (B,n,3) and (B,m,3), got {tuple(xyz1.shape)} and {tuple(xyz2.shape)}"
    if xyz1.shape[0] != xyz2.shape[0]:
        return f"batch sizes differ: {tuple(xyz1.shape)} and {tuple(xyz2.shape)}"
    B, n, m = xyz1.shape[0], xyz1.shape[1], xyz2.shape[1]
    if not (1 <= n <= CHAMFER_MAX_POINTS and 1 <= m <= CHAMFER_MAX_POINTS):
        return f"n = {n} and m = {m} must lie in 1 .. CHAMFER_MAX_POINTS = {CHAMFER_MAX_POINTS}"
    if B * max(n, m) >= _MAX_ROWS:
        return f"B * max(n, m) = {B * max(n, m)} must stay below 2^24"
    return None


def chamfer_covers(xyz1, xyz2):
    """Whether `forward` takes these tensors: CUDA float32 (B,n,3) / (B,m,3) within the kernels' limits."""
    return bool(torch.is_tensor(xyz1) and torch.is_tensor(xyz2) and xyz1.is_cuda and xyz2.is_cuda
                and xyz1.dtype == torch.float32 and xyz2.dtype == torch.float32 and _shape_problem(xyz1, xyz2) is None)


def _check(what, floats, ints=()):
    for name, t in floats:
        if t.dtype != torch.float32:
            raise RuntimeError(f"chamfer_dist.{what}: {name} must be float32 (got {t.dtype})")
    for name, t in ints:
        if t.dtype != torch.int32:
            raise RuntimeError(f"chamfer_dist.{what}: {name} must be int32 (got {t.dtype})")
    problem = _shape_problem(floats[0][1], floats[1][1])
    if problem:
        raise RuntimeError(f"chamfer_dist.{what}: {problem}")
    for name, t in (*floats, *ints):
        if not t.is_cuda:
            raise RuntimeError(f"chamfer_dist.{what}: {name} must be a CUDA/HIP tensor (got {t.device}); "
                               "the extension has no CPU path")
        if t.device != floats[0][1].device:
            raise RuntimeError(f"chamfer_dist.{what}: {name} is on {t.device}, expected {floats[0][1].device}")
        if not t.is_contiguous():
            raise RuntimeError(f"chamfer_dist.{what}: {name} must be contiguous (the extension reads raw rows)")


@torch.no_grad()
def forward(xyz1, xyz2):
    """-> (dist1 (B,n), dist2 (B,m), idx1 (B,n) int32, idx2 (B,m) int32): squared distance to, and index of, the
    nearest point of the other cloud."""
    from .fused import _call
    _check("forward", (("xyz1", xyz1), ("xyz2", xyz2)))
    B, n, m = xyz1.shape[0], xyz1.shape[1], xyz2.shape[1]
    dev = xyz1.device
    dist1 = torch.empty(B, n, dtype=torch.float32, device=dev)
    dist2 = torch.empty(B, m, dtype=torch.float32, device=dev)
    idx1 = torch.empty(B, n, dtype=torch.int32, device=dev)
    idx2 = torch.empty(B, m, dtype=torch.int32, device=dev)
    _call("apn_chamfer_forward", dev, B, n, m, xyz1.data_ptr(), xyz2.data_ptr(), dist1.data_ptr(), dist2.data_ptr(),
          idx1.data_ptr(), idx2.data_ptr())
    return dist1, dist2, idx1, idx2


@torch.no_grad()
def backward(xyz1, xyz2, idx1, idx2, grad_dist1, grad_dist2):
    """-> (grad_xyz1 (B,n,3), grad_xyz2 (B,m,3)) of sum(grad_dist1 * dist1) + sum(grad_dist2 * dist2), the indices held
    fixed."""
    from .fused import _call
    _check("backward", (("xyz1", xyz1), ("xyz2", xyz2), ("grad_dist1", grad_dist1), ("grad_dist2", grad_dist2)),
           (("idx1", idx1), ("idx2", idx2)))
    B, n, m = xyz1.shape[0], xyz1.shape[1], xyz2.shape[1]
    for name, t, rows in (("idx1", idx1, n), ("grad_dist1", grad_dist1, n), ("idx2", idx2, m), ("grad_dist2", grad_dist2, m)):
        if tuple(t.shape) != (B, rows):
            raise RuntimeError(f"chamfer_dist.backward: {name} must be {(B, rows)}, got {tuple(t.shape)}")
    grad_xyz1 = torch.empty_like(xyz1)
    grad_xyz2 = torch.empty_like(xyz2)
    _call("apn_chamfer_backward", xyz1.device, B, n, m, xyz1.data_ptr(), xyz2.data_ptr(), idx1.data_ptr(), idx2.data_ptr(),
          grad_dist1.data_ptr(), grad_dist2.data_ptr(), grad_xyz1.data_ptr(), grad_xyz2.data_ptr())
    return grad_xyz1, grad_xyz2


def _module():
    import sys
    return sys.modules[__name__]


class ChamferFunction(torch.autograd.Function):
    """The reference's Function: saves (xyz1, xyz2, idx1, idx2), returns the two squared-distance rows.  `forward` and
    `backward` are looked up on this module at call time, so a test can stand the numpy statement in for the kernels."""

    @staticmethod
    def forward(ctx, xyz1, xyz2):
        xyz1, xyz2 = xyz1.contiguous(), xyz2.contiguous()
        dist1, dist2, idx1, idx2 = _module().forward(xyz1, xyz2)
        ctx.save_for_backward(xyz1, xyz2, idx1, idx2)
        return dist1, dist2

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_dist1, grad_dist2):
        xyz1, xyz2, idx1, idx2 = ctx.saved_tensors
        grad_xyz1, grad_xyz2 = _module().backward(xyz1, xyz2, idx1, idx2, grad_dist1.contiguous(), grad_dist2.contiguous())
        return grad_xyz1, grad_xyz2


class _ChamferDistance(torch.nn.Module):
    def __init__(self, ignore_zeros=False):
        super().__init__()
        self.ignore_zeros = ignore_zeros

    def distances(self, xyz1, xyz2):
        if xyz1.size(0) == 1 and self.ignore_zeros:        # rows whose coordinates sum to zero are padding
            xyz1 = xyz1[torch.sum(xyz1, dim=2).ne(0)].unsqueeze(dim=0)
            xyz2 = xyz2[torch.sum(xyz2, dim=2).ne(0)].unsqueeze(dim=0)
        return ChamferFunction.apply(xyz1, xyz2)


class ChamferDistanceL2(_ChamferDistance):
    """mean(dist1) + mean(dist2), squared distances."""

    def forward(self, xyz1, xyz2):
        dist1, dist2 = self.distances(xyz1, xyz2)
        return torch.mean(dist1) + torch.mean(dist2)


class ChamferDistanceL2_split(_ChamferDistance):
    """(mean(dist1), mean(dist2)), squared distances."""

    def forward(self, xyz1, xyz2):
        dist1, dist2 = self.distances(xyz1, xyz2)
        return torch.mean(dist1), torch.mean(dist2)


class ChamferDistanceL1(_ChamferDistance):
    """(mean(sqrt(dist1)) + mean(sqrt(dist2))) / 2."""

    def forward(self, xyz1, xyz2):
        dist1, dist2 = self.distances(xyz1, xyz2)
        return (torch.mean(torch.sqrt(dist1)) + torch.mean(torch.sqrt(dist2))) / 2
