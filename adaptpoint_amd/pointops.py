"""The stacked-cloud operators on the device: the reference's compiled `pointops_cuda` module and the Functions of its
`openpoints/cpp/pointops/functions/pointops.py` over csrc/pointops.hip.

Layout: points (n,3), features (n,c) and an int32 `offset` (b) of cumulative END rows, so that every cloud has its own
size; queries (m,...) come with their own `new_offset` (b).  include/adaptpoint_amd.h states every operation exactly.

The eleven `*_cuda` functions keep the reference's names, argument order and in-place outputs (pointops_api.cpp); the
root module `pointops_cuda.py` re-exports them, so the reference's `functions/pointops.py` runs unmodified.  The
Functions and functions below keep the reference's public names, signatures and return values, with these differences:

  * outputs are `torch.empty` -- every kernel writes every element, no `.zero_()`: a captured graph holds no memset node;
  * the four backward passes walk reverse-neighbour lists in a fixed order instead of float atomicAdd: two runs give
    the same bits.  The lists (`PoCSR`) of an index tensor are built ONCE and cached ON THE TENSOR OBJECT
    (`idx._apn_po_csr`, keyed by the row count and the tensor's version counter), so the Functions that share one
    `idx` in a step -- grouping of xyz and of features, subtraction, aggregation -- share one build.  The Functions keep
    the Python object of `idx` on their ctx for this;
  * only `FurthestSampling` reads offsets on the host (to size its output and find n_max), as the reference does;
  * kNN orders equal distances by index; a cloud with fewer than k points pads with (start of the cloud, 1e10 -> 1e5
    after the sqrt), the reference's quirk; an empty output range of the sampler writes nothing;
  * `queryandgroup` / `querygroup` gather with `grouping` (deterministic gradient for xyz as well) instead of advanced
    indexing; `interpolation` and `interpolation2` both run the fused kernel, in the arithmetic order of the
    reference's Python loop.
"""
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

PO_K_MAX = 100                      # kNN: the reference's array bound
_MAX_ROWS = 2 ** 24                 # n, m stay below this
_MAX_POS = 2 ** 31                  # m * k stays below this


def _call(name, dev, *args):
    from .fused import _call as call
    call(name, dev, *args)


def pointops_covers(xyz, offset, new_xyz=None, new_offset=None):
    """Whether the kernels take these tensors: CUDA float32 contiguous (n,3) / (m,3) rows below 2^24 with int32
    contiguous offsets (b) on the same device."""
    new_xyz = xyz if new_xyz is None else new_xyz
    new_offset = offset if new_offset is None else new_offset
    ts = (xyz, new_xyz, offset, new_offset)
    if not all(torch.is_tensor(t) and t.is_cuda and t.is_contiguous() and t.device == xyz.device for t in ts):
        return False
    if xyz.dtype != torch.float32 or new_xyz.dtype != torch.float32:
        return False
    if offset.dtype != torch.int32 or new_offset.dtype != torch.int32:
        return False
    if xyz.dim() != 2 or new_xyz.dim() != 2 or xyz.shape[1] != 3 or new_xyz.shape[1] != 3:
        return False
    if offset.dim() != 1 or offset.shape != new_offset.shape or offset.shape[0] < 1:
        return False
    return xyz.shape[0] < _MAX_ROWS and new_xyz.shape[0] < _MAX_ROWS


def _check(what, floats=(), ints=()):
    """dtype, device and contiguity of the raw entries' tensors (the library checks sizes and returns APN_EINVAL)."""
    ts = (*floats, *ints)
    for name, t in floats:
        if t.dtype != torch.float32:
            raise RuntimeError(f"pointops.{what}: {name} must be float32 (got {t.dtype})")
    for name, t in ints:
        if t.dtype != torch.int32:
            raise RuntimeError(f"pointops.{what}: {name} must be int32 (got {t.dtype})")
    for name, t in ts:
        if not t.is_cuda:
            raise RuntimeError(f"pointops.{what}: {name} must be a CUDA/HIP tensor (got {t.device}); "
                               "the extension has no CPU path")
        if t.device != ts[0][1].device:
            raise RuntimeError(f"pointops.{what}: {name} is on {t.device}, expected {ts[0][1].device}")
        if not t.is_contiguous():
            raise RuntimeError(f"pointops.{what}: {name} must be contiguous (the extension reads raw rows)")


def _numel(what, name, t, count):
    if t.numel() != count:
        raise RuntimeError(f"pointops.{what}: {name} must hold {count} elements, got {tuple(t.shape)}")


# ----------------------------------------------------------------------------------------------- reverse lists
class PoCSR:
    """The reverse lists of an (m,k) index into n rows: pcnt_poff (2,n) int32 and plist (m*k) int32 (apn_po_csr)."""
    __slots__ = ("n", "m", "k", "pcnt_poff", "plist")

    def __init__(self, n, m, k, pcnt_poff, plist):
        self.n, self.m, self.k, self.pcnt_poff, self.plist = n, m, k, pcnt_poff, plist

    @property
    def pcnt(self):
        return self.pcnt_poff[0]

    @property
    def poff(self):
        return self.pcnt_poff[1]


@torch.no_grad()
def build_csr(idx, n):
    """-> PoCSR of idx (m,k) int32 into n rows; indices are clamped into [0, n) as every kernel clamps them."""
    _check("build_csr", ints=(("idx", idx),))
    m, k = idx.shape[0], idx.shape[-1] if idx.dim() > 1 else 1
    dev = idx.device
    pcnt_poff = torch.empty(2, n, dtype=torch.int32, device=dev)
    plist = torch.empty(m * k, dtype=torch.int32, device=dev)
    scratch = torch.empty(n + m * k, dtype=torch.int32, device=dev)
    _call("apn_po_csr", dev, n, m, k, idx.data_ptr(), pcnt_poff.data_ptr(), plist.data_ptr(), scratch.data_ptr())
    return PoCSR(n, m, k, pcnt_poff, plist)


def csr_of(idx, n):
    """The PoCSR of `idx` into n rows, built once per tensor object and version: cached as `idx._apn_po_csr`."""
    hit = getattr(idx, "_apn_po_csr", None)
    if hit is not None and hit[0] == (n, idx._version, idx.data_ptr(), tuple(idx.shape)):
        return hit[1]
    csr = build_csr(idx, n)
    idx._apn_po_csr = ((n, idx._version, idx.data_ptr(), tuple(idx.shape)), csr)
    return csr


# ------------------------------------------------------------------- the extension's eleven functions (in-place)
@torch.no_grad()
def knnquery_cuda(m, nsample, xyz, new_xyz, offset, new_offset, idx, dist2):
    _check("knnquery_cuda", (("xyz", xyz), ("new_xyz", new_xyz), ("dist2", dist2)),
           (("offset", offset), ("new_offset", new_offset), ("idx", idx)))
    m = int(m)
    _numel("knnquery_cuda", "new_xyz", new_xyz, m * 3)
    _numel("knnquery_cuda", "idx", idx, m * nsample)
    _numel("knnquery_cuda", "dist2", dist2, m * nsample)
    _call("apn_po_knn_query", xyz.device, offset.shape[0], xyz.shape[0], m, int(nsample), xyz.data_ptr(),
          new_xyz.data_ptr(), offset.data_ptr(), new_offset.data_ptr(), idx.data_ptr(), dist2.data_ptr())


@torch.no_grad()
def ballquery_cuda(m, radius, nsample, xyz, new_xyz, offset, new_offset, idx):
    _check("ballquery_cuda", (("xyz", xyz), ("new_xyz", new_xyz)),
           (("offset", offset), ("new_offset", new_offset), ("idx", idx)))
    m = int(m)
    _numel("ballquery_cuda", "new_xyz", new_xyz, m * 3)
    _numel("ballquery_cuda", "idx", idx, m * nsample)
    _call("apn_po_ball_query", xyz.device, offset.shape[0], xyz.shape[0], m, float(radius), int(nsample), xyz.data_ptr(),
          new_xyz.data_ptr(), offset.data_ptr(), new_offset.data_ptr(), idx.data_ptr())


@torch.no_grad()
def furthestsampling_cuda(b, n_max, xyz, offset, new_offset, tmp, idx):
    _check("furthestsampling_cuda", (("xyz", xyz), ("tmp", tmp)),
           (("offset", offset), ("new_offset", new_offset), ("idx", idx)))
    b = int(b)
    if offset.shape[0] < b or new_offset.shape[0] < b:
        raise RuntimeError(f"pointops.furthestsampling_cuda: offsets must hold b = {b} entries")
    _numel("furthestsampling_cuda", "tmp", tmp, xyz.shape[0])
    _call("apn_po_furthest_sampling", xyz.device, b, int(n_max), xyz.data_ptr(), offset.data_ptr(),
          new_offset.data_ptr(), tmp.data_ptr(), idx.data_ptr())


@torch.no_grad()
def grouping_forward_cuda(m, nsample, c, input, idx, output):
    _check("grouping_forward_cuda", (("input", input), ("output", output)), (("idx", idx),))
    _numel("grouping_forward_cuda", "idx", idx, m * nsample)
    _numel("grouping_forward_cuda", "output", output, m * nsample * c)
    _numel("grouping_forward_cuda", "input", input, input.shape[0] * c)
    _call("apn_po_grouping_fwd", input.device, input.shape[0], m, nsample, c, input.data_ptr(), idx.data_ptr(),
          output.data_ptr())


@torch.no_grad()
def grouping_backward_cuda(m, nsample, c, grad_output, idx, grad_input):
    _check("grouping_backward_cuda", (("grad_output", grad_output), ("grad_input", grad_input)), (("idx", idx),))
    _numel("grouping_backward_cuda", "idx", idx, m * nsample)
    _numel("grouping_backward_cuda", "grad_output", grad_output, m * nsample * c)
    n = grad_input.shape[0]
    _numel("grouping_backward_cuda", "grad_input", grad_input, n * c)
    csr = csr_of(idx, n)
    _call("apn_po_grouping_bwd", idx.device, n, m, nsample, c, grad_output.data_ptr(), csr.pcnt_poff.data_ptr(),
          csr.plist.data_ptr(), grad_input.data_ptr())


@torch.no_grad()
def interpolation_forward_cuda(n, c, k, input, idx, weight, output):
    """The reference's argument names: n outputs from the rows of input (m,c)."""
    _check("interpolation_forward_cuda", (("input", input), ("weight", weight), ("output", output)), (("idx", idx),))
    _numel("interpolation_forward_cuda", "idx", idx, n * k)
    _numel("interpolation_forward_cuda", "weight", weight, n * k)
    _numel("interpolation_forward_cuda", "output", output, n * c)
    _numel("interpolation_forward_cuda", "input", input, input.shape[0] * c)
    _call("apn_po_interpolation_fwd", input.device, input.shape[0], n, k, c, input.data_ptr(), idx.data_ptr(),
          weight.data_ptr(), output.data_ptr())


@torch.no_grad()
def interpolation_backward_cuda(n, c, k, grad_output, idx, weight, grad_input):
    _check("interpolation_backward_cuda", (("grad_output", grad_output), ("weight", weight), ("grad_input", grad_input)),
           (("idx", idx),))
    _numel("interpolation_backward_cuda", "idx", idx, n * k)
    _numel("interpolation_backward_cuda", "weight", weight, n * k)
    _numel("interpolation_backward_cuda", "grad_output", grad_output, n * c)
    rows = grad_input.shape[0]
    _numel("interpolation_backward_cuda", "grad_input", grad_input, rows * c)
    csr = csr_of(idx, rows)
    _call("apn_po_interpolation_bwd", idx.device, rows, n, k, c, grad_output.data_ptr(), weight.data_ptr(),
          csr.pcnt_poff.data_ptr(), csr.plist.data_ptr(), grad_input.data_ptr())


@torch.no_grad()
def subtraction_forward_cuda(n, nsample, c, input1, input2, idx, output):
    _check("subtraction_forward_cuda", (("input1", input1), ("input2", input2), ("output", output)), (("idx", idx),))
    _numel("subtraction_forward_cuda", "idx", idx, n * nsample)
    _numel("subtraction_forward_cuda", "input1", input1, n * c)
    _numel("subtraction_forward_cuda", "input2", input2, input2.shape[0] * c)
    _numel("subtraction_forward_cuda", "output", output, n * nsample * c)
    _call("apn_po_subtraction_fwd", idx.device, input2.shape[0], n, nsample, c, input1.data_ptr(), input2.data_ptr(),
          idx.data_ptr(), output.data_ptr())


@torch.no_grad()
def subtraction_backward_cuda(n, nsample, c, idx, grad_output, grad_input1, grad_input2):
    _check("subtraction_backward_cuda", (("grad_output", grad_output), ("grad_input1", grad_input1),
                                         ("grad_input2", grad_input2)), (("idx", idx),))
    _numel("subtraction_backward_cuda", "idx", idx, n * nsample)
    _numel("subtraction_backward_cuda", "grad_output", grad_output, n * nsample * c)
    _numel("subtraction_backward_cuda", "grad_input1", grad_input1, n * c)
    rows = grad_input2.shape[0]
    _numel("subtraction_backward_cuda", "grad_input2", grad_input2, rows * c)
    csr = csr_of(idx, rows)
    _call("apn_po_subtraction_bwd", idx.device, rows, n, nsample, c, grad_output.data_ptr(), csr.pcnt_poff.data_ptr(),
          csr.plist.data_ptr(), grad_input1.data_ptr(), grad_input2.data_ptr())


@torch.no_grad()
def aggregation_forward_cuda(n, nsample, c, w_c, input, position, weight, idx, output):
    _check("aggregation_forward_cuda", (("input", input), ("position", position), ("weight", weight),
                                        ("output", output)), (("idx", idx),))
    _numel("aggregation_forward_cuda", "idx", idx, n * nsample)
    _numel("aggregation_forward_cuda", "input", input, input.shape[0] * c)
    _numel("aggregation_forward_cuda", "position", position, n * nsample * c)
    _numel("aggregation_forward_cuda", "weight", weight, n * nsample * w_c)
    _numel("aggregation_forward_cuda", "output", output, n * c)
    _call("apn_po_aggregation_fwd", idx.device, input.shape[0], n, nsample, c, w_c, input.data_ptr(), position.data_ptr(),
          weight.data_ptr(), idx.data_ptr(), output.data_ptr())


@torch.no_grad()
def aggregation_backward_cuda(n, nsample, c, w_c, input, position, weight, idx, grad_output, grad_input, grad_position,
                              grad_weight):
    _check("aggregation_backward_cuda", (("input", input), ("position", position), ("weight", weight),
                                         ("grad_output", grad_output), ("grad_input", grad_input),
                                         ("grad_position", grad_position), ("grad_weight", grad_weight)), (("idx", idx),))
    rows = input.shape[0]
    _numel("aggregation_backward_cuda", "idx", idx, n * nsample)
    _numel("aggregation_backward_cuda", "input", input, rows * c)
    _numel("aggregation_backward_cuda", "position", position, n * nsample * c)
    _numel("aggregation_backward_cuda", "weight", weight, n * nsample * w_c)
    _numel("aggregation_backward_cuda", "grad_output", grad_output, n * c)
    _numel("aggregation_backward_cuda", "grad_input", grad_input, rows * c)
    _numel("aggregation_backward_cuda", "grad_position", grad_position, n * nsample * c)
    _numel("aggregation_backward_cuda", "grad_weight", grad_weight, n * nsample * w_c)
    csr = csr_of(idx, rows)
    _call("apn_po_aggregation_bwd", idx.device, rows, n, nsample, c, w_c, input.data_ptr(), position.data_ptr(),
          weight.data_ptr(), idx.data_ptr(), grad_output.data_ptr(), csr.pcnt_poff.data_ptr(), csr.plist.data_ptr(),
          grad_input.data_ptr(), grad_position.data_ptr(), grad_weight.data_ptr())


# -------------------------------------------------------------------------- the reference's Functions and functions
def _f32(dev, *shape):
    return torch.empty(*shape, dtype=torch.float32, device=dev)


def _i32(dev, *shape):
    return torch.empty(*shape, dtype=torch.int32, device=dev)


class FurthestSampling(Function):
    @staticmethod
    def forward(ctx, xyz, offset, new_offset):
        """input: xyz (n,3), offset (b), new_offset (b); output: idx (m).  Reads both offsets on the host."""
        assert xyz.is_contiguous()
        n, b = xyz.shape[0], offset.shape[0]
        ends = offset.tolist()
        n_max = max(e - s for s, e in zip([0] + ends[:-1], ends))
        m = int(new_offset[b - 1].item())
        idx = _i32(xyz.device, m)
        tmp = torch.full((n,), 1e10, dtype=torch.float32, device=xyz.device)
        furthestsampling_cuda(b, n_max, xyz, offset, new_offset, tmp, idx)
        ctx.mark_non_differentiable(idx)
        return idx


furthestsampling = FurthestSampling.apply


class KNNQuery(Function):
    @staticmethod
    def forward(ctx, nsample, xyz, new_xyz, offset, new_offset):
        """input: xyz (n,3), new_xyz (m,3), offset (b), new_offset (b); output: idx (m,nsample), dist (m,nsample)."""
        if new_xyz is None:
            new_xyz = xyz
        assert xyz.is_contiguous() and new_xyz.is_contiguous()
        m = new_xyz.shape[0]
        idx = _i32(xyz.device, m, nsample)
        dist2 = _f32(xyz.device, m, nsample)
        knnquery_cuda(m, nsample, xyz, new_xyz, offset, new_offset, idx, dist2)
        dist = torch.sqrt(dist2)
        ctx.mark_non_differentiable(idx, dist)
        return idx, dist


knnquery = KNNQuery.apply


class BallQuery(Function):
    @staticmethod
    def forward(ctx, radius, nsample, xyz, new_xyz, offset, new_offset):
        """input: xyz (n,3), new_xyz (m,3), offset (b), new_offset (b); output: idx (m,nsample)."""
        if new_xyz is None:
            new_xyz = xyz
        assert xyz.is_contiguous() and new_xyz.is_contiguous()
        m = new_xyz.shape[0]
        idx = _i32(xyz.device, m, nsample)
        ballquery_cuda(m, radius, nsample, xyz, new_xyz, offset, new_offset, idx)
        ctx.mark_non_differentiable(idx)
        return idx


ballquery = BallQuery.apply


class Grouping(Function):
    @staticmethod
    def forward(ctx, input, idx):
        """input: input (n,c), idx (m,nsample); output: (m,nsample,c)."""
        assert input.is_contiguous() and idx.is_contiguous()
        m, nsample, n, c = idx.shape[0], idx.shape[1], input.shape[0], input.shape[1]
        output = _f32(input.device, m, nsample, c)
        grouping_forward_cuda(m, nsample, c, input, idx, output)
        ctx.n = n
        ctx.po_idx = idx                    # the Python object: its reverse lists are cached on it (csr_of)
        return output

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        n, idx = ctx.n, ctx.po_idx
        m, nsample, c = grad_output.shape
        grad_input = _f32(grad_output.device, n, c)
        grouping_backward_cuda(m, nsample, c, grad_output.contiguous(), idx, grad_input)
        return grad_input, None


grouping = Grouping.apply


def querygroup(nsample, xyz, new_xyz, feat, offset, new_offset, radius=None, query_method='knn', normalize_dp=False,
               idx=None):
    """The reference's query-and-group over kNN or the ball query: (grouped_xyz (m,nsample,3), grouped_feat (m,nsample,c))."""
    if new_xyz is None:
        new_xyz = xyz
    assert xyz.is_contiguous() and new_xyz.is_contiguous() and (feat is None or feat.is_contiguous())
    if idx is None:
        if nsample is not None:
            if query_method in ['knn', 'knnquery']:
                idx, _ = knnquery(nsample, xyz, new_xyz, offset, new_offset)
            else:
                idx = ballquery(radius, nsample, xyz, new_xyz, offset, new_offset)
            grouped_xyz = grouping(xyz, idx) - new_xyz.unsqueeze(1)
            if normalize_dp:
                max_dist = grouped_xyz.norm(dim=-1, p=2, keepdim=True).max(dim=-1, keepdim=True)[
                    0] + 1.0e-8 if query_method == 'knn' else radius
                grouped_xyz = grouped_xyz / max_dist
            grouped_feat = grouping(feat, idx) if feat is not None else None
        else:
            grouped_xyz = xyz.transpose(1, 2).unsqueeze(2)
            grouped_feat = feat.unsqueeze(2) if feat is not None else None
        return grouped_xyz, grouped_feat


def queryandgroup(nsample, xyz, new_xyz, feat, idx, offset, new_offset, use_xyz=True):
    """input: xyz (n,3), new_xyz (m,3), feat (n,c), idx (m,nsample) or None; output: (m,nsample,3+c) or (m,nsample,c)."""
    if new_xyz is None:
        new_xyz = xyz
    assert xyz.is_contiguous() and new_xyz.is_contiguous() and feat.is_contiguous()
    if idx is None:
        idx, _ = knnquery(nsample, xyz, new_xyz, offset, new_offset)
    grouped_feat = grouping(feat, idx)
    if use_xyz:
        grouped_xyz = grouping(xyz, idx) - new_xyz.unsqueeze(1)
        return torch.cat((grouped_xyz, grouped_feat), -1)
    return grouped_feat


class Subtraction(Function):
    @staticmethod
    def forward(ctx, input1, input2, idx):
        """input: input1 (n,c), input2 (n,c), idx (n,nsample); output: (n,nsample,c)."""
        assert input1.is_contiguous() and input2.is_contiguous()
        n, c = input1.shape
        nsample = idx.shape[-1]
        output = _f32(input1.device, n, nsample, c)
        subtraction_forward_cuda(n, nsample, c, input1, input2, idx, output)
        ctx.rows = input2.shape[0]
        ctx.po_idx = idx
        return output

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        idx = ctx.po_idx
        n, nsample, c = grad_output.shape
        grad_input1 = _f32(grad_output.device, n, c)
        grad_input2 = _f32(grad_output.device, ctx.rows, c)
        subtraction_backward_cuda(n, nsample, c, idx, grad_output.contiguous(), grad_input1, grad_input2)
        return grad_input1, grad_input2, None


subtraction = Subtraction.apply


class Aggregation(Function):
    @staticmethod
    def forward(ctx, input, position, weight, idx):
        """input: input (n,c), position (n,nsample,c), weight (n,nsample,c'), idx (n,nsample); output: (n,c)."""
        assert input.is_contiguous() and position.is_contiguous() and weight.is_contiguous()
        n, nsample, c = position.shape
        w_c = weight.shape[-1]
        output = _f32(input.device, n, c)
        aggregation_forward_cuda(n, nsample, c, w_c, input, position, weight, idx, output)
        ctx.save_for_backward(input, position, weight)
        ctx.po_idx = idx
        return output

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        input, position, weight = ctx.saved_tensors
        idx = ctx.po_idx
        n, nsample, c = position.shape
        w_c = weight.shape[-1]
        grad_input = torch.empty_like(input)
        grad_position = torch.empty_like(position)
        grad_weight = torch.empty_like(weight)
        aggregation_backward_cuda(n, nsample, c, w_c, input, position, weight, idx, grad_output.contiguous(), grad_input,
                                  grad_position, grad_weight)
        return grad_input, grad_position, grad_weight, None


aggregation = Aggregation.apply


class Interpolation(Function):
    @staticmethod
    def forward(ctx, xyz, new_xyz, input, offset, new_offset, k=3):
        """input: xyz (m,3), new_xyz (n,3), input (m,c), offset (b), new_offset (b); output: (n,c)."""
        assert xyz.is_contiguous() and new_xyz.is_contiguous() and input.is_contiguous()
        idx, dist = knnquery(k, xyz, new_xyz, offset, new_offset)
        dist_recip = 1.0 / (dist + 1e-8)
        norm = torch.sum(dist_recip, dim=1, keepdim=True)
        weight = (dist_recip / norm).contiguous()
        n, c, m = new_xyz.shape[0], input.shape[1], input.shape[0]
        output = _f32(input.device, n, c)
        interpolation_forward_cuda(n, c, k, input, idx, weight, output)
        ctx.m, ctx.k = m, k
        ctx.save_for_backward(weight)
        ctx.po_idx = idx
        return output

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        m, k = ctx.m, ctx.k
        weight, = ctx.saved_tensors
        n, c = grad_output.shape
        grad_input = _f32(grad_output.device, m, c)
        interpolation_backward_cuda(n, c, k, grad_output.contiguous(), ctx.po_idx, weight, grad_input)
        return None, None, grad_input, None, None, None


interpolation2 = Interpolation.apply


def interpolation(xyz, new_xyz, feat, offset, new_offset, k=3):
    """The reference's composed form (a Python loop over the k neighbours), here the fused kernel: the same products
    added in the same order."""
    return Interpolation.apply(xyz, new_xyz, feat, offset, new_offset, k)


__all__ = ["knnquery_cuda", "ballquery_cuda", "furthestsampling_cuda", "grouping_forward_cuda", "grouping_backward_cuda",
           "interpolation_forward_cuda", "interpolation_backward_cuda", "subtraction_forward_cuda",
           "subtraction_backward_cuda", "aggregation_forward_cuda", "aggregation_backward_cuda",
           "FurthestSampling", "KNNQuery", "BallQuery", "Grouping", "Subtraction", "Aggregation", "Interpolation",
           "furthestsampling", "knnquery", "ballquery", "grouping", "querygroup", "queryandgroup", "subtraction",
           "aggregation", "interpolation", "interpolation2", "pointops_covers", "PoCSR", "build_csr", "csr_of"]
