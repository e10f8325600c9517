"""Earth mover's distance on the device: the reference's compiled `emd_cuda` module and the classes of its
`openpoints/cpp/emd/emd.py` over csrc/emd.hip.

The three extension functions keep the reference's names, argument order and return order (emd.cpp):

    approxmatch_forward(xyz1 (B,n,3), xyz2 (B,m,3))        -> match (B,m,n)
    matchcost_forward(xyz1, xyz2, match)                   -> cost (B,)
    matchcost_backward(grad_cost (B,), xyz1, xyz2, match)  -> grad1 (B,n,3), grad2 (B,m,3)

`match` is a sum over ten annealing levels of rank-structured weights, so two small tables, ratio_l (B,10,n) and
ratio_r (B,10,m), determine it (include/adaptpoint_amd.h states the contract exactly).  `emd_ratios` runs the iteration
that makes them; `approxmatch_forward` then writes `match` once.  `EarthMoverDistanceFunction` never allocates (B,m,n):
its forward runs the iteration and takes the cost from the tables, its backward takes both gradients from the tables,
each match[l,k] recomputed in registers -- bit for bit what the materialised `match` gives.  All sums run in an order
fixed by the shapes, without float atomics: two runs give the same bits.  `match` is a constant in the gradient, as in
the reference.
"""
import torch
from torch.autograd.function import once_differentiable

EMD_MAX_POINTS = 8192               # = apn_emd_max_points()
EMD_ONE_LAUNCH_MAX = 128            # = apn_emd_one_launch_max(): max(n, m) up to here runs the iteration in one launch
EMD_LEVELS = 10
_MAX_ROWS = 2 ** 24                 # B * max(n, m) stays below this
_TILE = 64                          # rows per workgroup: apn_emd_cost_parts(n) = ceil(n / 64)


def _shape_problem(xyz1, xyz2):
    """Why the kernels do not take clouds of these shapes (None: they do).  Device and dtype are checked elsewhere."""
    if xyz1.dim() != 3 or xyz2.dim() != 3 or xyz1.shape[2] != 3 or xyz2.shape[2] != 3:
        return f"clouds must be (B,n,3) and (B,m,3), got {tuple(xyz1.shape)} and {tuple(xyz2.shape)}"
    if xyz1.shape[0] != xyz2.shape[0]:
        return f"batch sizes differ: {tuple(xyz1.shape)} and {tuple(xyz2.shape)}"
    B, n, m = xyz1.shape[0], xyz1.shape[1], xyz2.shape[1]
    if not (1 <= n <= EMD_MAX_POINTS and 1 <= m <= EMD_MAX_POINTS):
        return f"n = {n} and m = {m} must lie in 1 .. EMD_MAX_POINTS = {EMD_MAX_POINTS}"
    if B * max(n, m) >= _MAX_ROWS:
        return f"B * max(n, m) = {B * max(n, m)} must stay below 2^24"
    return None


def emd_covers(xyz1, xyz2):
    """Whether the kernels take these tensors: CUDA float32 (B,n,3) / (B,m,3) within their limits."""
    return bool(torch.is_tensor(xyz1) and torch.is_tensor(xyz2) and xyz1.is_cuda and xyz2.is_cuda
                and xyz1.dtype == torch.float32 and xyz2.dtype == torch.float32 and _shape_problem(xyz1, xyz2) is None)


def _check(what, tensors, shapes=()):
    for name, t in tensors:
        if t.dtype != torch.float32:
            raise RuntimeError(f"emd.{what}: {name} must be float32 (got {t.dtype})")
    problem = _shape_problem(tensors[0][1], tensors[1][1])
    if problem:
        raise RuntimeError(f"emd.{what}: {problem}")
    for name, t in tensors:
        if not t.is_cuda:
            raise RuntimeError(f"emd.{what}: {name} must be a CUDA/HIP tensor (got {t.device}); "
                               "the extension has no CPU path")
        if t.device != tensors[0][1].device:
            raise RuntimeError(f"emd.{what}: {name} is on {t.device}, expected {tensors[0][1].device}")
        if not t.is_contiguous():
            raise RuntimeError(f"emd.{what}: {name} must be contiguous (the extension reads raw rows)")
    for name, t, shape in shapes:
        if tuple(t.shape) != tuple(shape):
            raise RuntimeError(f"emd.{what}: {name} must be {tuple(shape)}, got {tuple(t.shape)}")


def _dims(xyz1, xyz2):
    return xyz1.shape[0], xyz1.shape[1], xyz2.shape[1]


@torch.no_grad()
def emd_ratios(xyz1, xyz2):
    """-> (ratio_l (B,10,n), ratio_r (B,10,m)): the iteration; level 0 is the reference's j = 7, level 9 its j = -2."""
    from .fused import _call
    _check("emd_ratios", (("xyz1", xyz1), ("xyz2", xyz2)))
    B, n, m = _dims(xyz1, xyz2)
    dev = xyz1.device
    ratio_l = torch.empty(B, EMD_LEVELS, n, dtype=torch.float32, device=dev)
    ratio_r = torch.empty(B, EMD_LEVELS, m, dtype=torch.float32, device=dev)
    state = torch.empty(B, n + m, dtype=torch.float32, device=dev)
    _call("apn_emd_ratios", dev, B, n, m, xyz1.data_ptr(), xyz2.data_ptr(), ratio_l.data_ptr(), ratio_r.data_ptr(),
          state.data_ptr())
    return ratio_l, ratio_r


@torch.no_grad()
def match_from_ratios(xyz1, xyz2, ratio_l, ratio_r):
    """-> match (B,m,n), every element written once from the tables."""
    from .fused import _call
    _check("match_from_ratios", (("xyz1", xyz1), ("xyz2", xyz2)))
    B, n, m = _dims(xyz1, xyz2)
    _check("match_from_ratios", (("xyz1", xyz1), ("xyz2", xyz2), ("ratio_l", ratio_l), ("ratio_r", ratio_r)),
           (("ratio_l", ratio_l, (B, EMD_LEVELS, n)), ("ratio_r", ratio_r, (B, EMD_LEVELS, m))))
    match = torch.empty(B, m, n, dtype=torch.float32, device=xyz1.device)
    _call("apn_emd_match", xyz1.device, B, n, m, xyz1.data_ptr(), xyz2.data_ptr(), ratio_l.data_ptr(), ratio_r.data_ptr(),
          match.data_ptr())
    return match


def _sources(what, xyz1, xyz2, match, ratios):
    """The (name, tensor) pairs and shapes of whichever source of `match` the caller gave, after the clouds' own check."""
    if (match is None) == (ratios is None):
        raise RuntimeError(f"emd.{what}: give either match or the two ratio tables")
    _check(what, (("xyz1", xyz1), ("xyz2", xyz2)))             # the other shapes follow from the clouds'
    B, n, m = _dims(xyz1, xyz2)
    if match is not None:
        return (("match", match),), (("match", match, (B, m, n)),)
    ratio_l, ratio_r = ratios
    return ((("ratio_l", ratio_l), ("ratio_r", ratio_r)),
            (("ratio_l", ratio_l, (B, EMD_LEVELS, n)), ("ratio_r", ratio_r, (B, EMD_LEVELS, m))))


@torch.no_grad()
def cost(xyz1, xyz2, match=None, ratios=None):
    """-> cost (B,) = sum_{k,l} d[l,k] match[l,k], `match` read from memory or recomputed from `ratios` = (ratio_l, ratio_r)."""
    from .fused import _call, _ptr
    named, shapes = _sources("cost", xyz1, xyz2, match, ratios)
    _check("cost", (("xyz1", xyz1), ("xyz2", xyz2), *named), shapes)
    B, n, m = _dims(xyz1, xyz2)
    dev = xyz1.device
    part = torch.empty(B, (n + _TILE - 1) // _TILE, dtype=torch.float32, device=dev)
    out = torch.empty(B, dtype=torch.float32, device=dev)
    ratio_l, ratio_r = ratios if ratios is not None else (None, None)
    _call("apn_emd_cost", dev, B, n, m, xyz1.data_ptr(), xyz2.data_ptr(), _ptr(match), _ptr(ratio_l), _ptr(ratio_r),
          part.data_ptr(), out.data_ptr())
    return out


@torch.no_grad()
def cost_grad(grad_cost, xyz1, xyz2, match=None, ratios=None):
    """-> (grad1 (B,n,3), grad2 (B,m,3)) of sum(grad_cost * cost), `match` held fixed and taken as in `cost`."""
    from .fused import _call, _ptr
    named, shapes = _sources("cost_grad", xyz1, xyz2, match, ratios)
    _check("cost_grad", (("xyz1", xyz1), ("xyz2", xyz2), ("grad_cost", grad_cost), *named),
           (("grad_cost", grad_cost, (xyz1.shape[0],)), *shapes))
    B, n, m = _dims(xyz1, xyz2)
    grad1, grad2 = torch.empty_like(xyz1), torch.empty_like(xyz2)
    ratio_l, ratio_r = ratios if ratios is not None else (None, None)
    _call("apn_emd_cost_grad", xyz1.device, B, n, m, grad_cost.data_ptr(), xyz1.data_ptr(), xyz2.data_ptr(), _ptr(match),
          _ptr(ratio_l), _ptr(ratio_r), grad1.data_ptr(), grad2.data_ptr())
    return grad1, grad2


def _module():
    import sys
    return sys.modules[__name__]


def approxmatch_forward(xyz1, xyz2):
    """The extension's function: match (B,m,n), match[b,l,k] the weight between xyz2[b,l] and xyz1[b,k]."""
    mod = _module()
    return mod.match_from_ratios(xyz1, xyz2, *mod.emd_ratios(xyz1, xyz2))


def matchcost_forward(xyz1, xyz2, match):
    """The extension's function: cost (B,)."""
    return _module().cost(xyz1, xyz2, match=match)


def matchcost_backward(grad_cost, xyz1, xyz2, match):
    """The extension's function: (grad1 (B,n,3), grad2 (B,m,3))."""
    return _module().cost_grad(grad_cost, xyz1, xyz2, match=match)


class EarthMoverDistanceFunction(torch.autograd.Function):
    """The reference's Function without its (B,m,n) tensor: saves (xyz1, xyz2, ratio_l, ratio_r), returns cost (B,).
    `emd_ratios`, `cost` and `cost_grad` are looked up on this module at call time, so a test can stand the numpy
    statement in for the kernels."""

    @staticmethod
    def forward(ctx, xyz1, xyz2):
        xyz1, xyz2 = xyz1.contiguous(), xyz2.contiguous()
        mod = _module()
        ratio_l, ratio_r = mod.emd_ratios(xyz1, xyz2)
        ctx.save_for_backward(xyz1, xyz2, ratio_l, ratio_r)
        return mod.cost(xyz1, xyz2, ratios=(ratio_l, ratio_r))

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_cost):
        xyz1, xyz2, ratio_l, ratio_r = ctx.saved_tensors
        return _module().cost_grad(grad_cost.contiguous(), xyz1, xyz2, ratios=(ratio_l, ratio_r))


class earth_mover_distance(torch.nn.Module):
    """The reference's module: mean over the batch of cost / n, n the size of xyz1.  `transpose` is accepted and
    ignored, as the reference ignores it: the clouds are (B,n,3) and (B,m,3)."""

    def forward(self, xyz1, xyz2, transpose=False):
        cost = EarthMoverDistanceFunction.apply(xyz1, xyz2)
        cost = cost / xyz1.size(1)
        return cost.mean()
