"""Voxel-grid subsampling on the device (csrc/voxel_grid.hip): the reference's host-side `voxelize` (openpoints/dataset/
data_util.py) and the barycentres / feature means of its compiled `subsampling` module (openpoints/cpp/subsampling).

Layout: `coord` (n,3) float32 or float64, optionally an int32 `offset` (b) of cumulative END rows (pointops.py's
convention; no offset = one cloud; empty clouds are allowed).  Per axis

    cell(i) = floor((double)coord[i] / (double)voxel_size)

which is what the reference computes under numpy 2 (`coord / np.array(voxel_size)` promotes float32 to float64); a
float32 division puts points on cell faces into other cells.  A voxel is a set of rows with equal (cloud, cell).
Coordinates may be negative: nothing needs the shift to min = 0 that the reference's hashes need.

`voxel_grid` returns a `VoxelGrid`:

    voxel_of (n) int32   voxels numbered 0..m-1 by their smallest member row, so a cloud's voxels are contiguous
    count, start (m)     voxel v's rows are idx_sort[start[v] : start[v] + count[v]]
    idx_sort (n)         rows grouped by voxel, ascending row inside a voxel: the stable argsort of voxel_of
    new_offset (b)       cumulative voxel ends per cloud (an empty cloud repeats the previous end)
    m, count_max         Python ints;  first = idx_sort[start]

Every field is a pure function of the inputs (two runs give the same bits).  The call reads one small stats tensor
{m, count_max, bad} on the host -- its only synchronisation -- so it is eager and not capturable, like
`pointops.FurthestSampling`.  A non-finite coordinate or a cell outside int32 raises ValueError.

Differences from the reference: it orders voxels by hash key and the rows of a voxel by numpy's unstable argsort, an
order nobody can match, so only its PARTITION and COUNTS are reproduced; `hash_type` is accepted and ignored (an FNV
collision, which merges two cells there, cannot happen here).  `VoxelGrid.mean` divides once by the count; the
reference's C++ grid subsampling places its grid at floor(min / dl) * dl in float32 and also votes a majority label:
neither is built.
"""
import numpy as np
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

_MAX_ROWS = 2 ** 27
_MAX_CHANNELS = 65536


def _call(name, dev, *args):
    from .fused import _call as call
    call(name, dev, *args)


def _sizes(voxel_size):
    vs = np.asarray(voxel_size, dtype=np.float64).reshape(-1)
    if vs.size == 1:
        vs = np.repeat(vs, 3)
    if vs.size != 3 or not np.all(np.isfinite(vs)) or not np.all(vs > 0):
        raise ValueError(f"voxel_grid: voxel_size must be one or three finite positive numbers, got {voxel_size!r}")
    return [float(v) for v in vs]


class _Mean(Function):
    @staticmethod
    def forward(ctx, values, grid):
        n, c = values.shape
        out = torch.empty(grid.m, c, dtype=torch.float32, device=values.device)
        _call("apn_vg_mean_fwd", values.device, n, grid.m, c, values.data_ptr(), grid.idx_sort.data_ptr(),
              grid.start.data_ptr(), grid.count.data_ptr(), out.data_ptr())
        ctx.grid = grid
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        grid = ctx.grid
        grad_out = grad_out.contiguous()
        c = grad_out.shape[1]
        grad = torch.empty(grid.n, c, dtype=torch.float32, device=grad_out.device)
        _call("apn_vg_mean_bwd", grad_out.device, grid.n, grid.m, c, grad_out.data_ptr(), grid.voxel_of.data_ptr(),
              grid.count.data_ptr(), grad.data_ptr())
        return grad, None


class VoxelGrid:
    """The partition of n stacked rows into m voxels (see the module's docstring for the fields)."""

    def __init__(self, n, m, count_max, voxel_of, count, start, idx_sort, new_offset):
        self.n, self.m, self.count_max = n, m, count_max
        self.voxel_of, self.count, self.start, self.idx_sort, self.new_offset = voxel_of, count, start, idx_sort, new_offset
        self._first = None

    @property
    def first(self):
        """(m) int32: every voxel's smallest row, idx_sort[start]."""
        if self._first is None:
            self._first = self.idx_sort[self.start.long()]
        return self._first

    def pick(self, draws):
        """idx_sort[start + draws % count] for non-negative integer draws (m): one row per voxel."""
        draws = torch.as_tensor(draws, device=self.count.device)
        if draws.dtype.is_floating_point or draws.dtype == torch.bool or draws.shape != (self.m,):
            raise ValueError(f"VoxelGrid.pick: draws must be ({self.m},) integers, got {tuple(draws.shape)} {draws.dtype}")
        return self.idx_sort[self.start.long() + draws.long() % self.count.long()]

    def part(self, i):
        """idx_sort[start + i % count]: the i-th of the count_max sub-clouds of the reference's test loop (`load_data`);
        the parts 0..count_max-1 together cover every row."""
        i = int(i)
        if i < 0:
            raise ValueError("VoxelGrid.part: i must not be negative")
        return self.idx_sort[self.start.long() + i % self.count.long()]

    def mean(self, values):
        """(m,c) per-voxel means of values (n,c) float32, 1 <= c <= 65536: sequential fp32 adds over a voxel's rows in
        ascending row, then one correctly rounded division by the count.  mean(coord) are grid subsampling's
        barycentres.  The backward is the gather grad_out[voxel_of[i]] / count: no atomics."""
        if not (torch.is_tensor(values) and values.is_cuda and values.dtype == torch.float32 and values.dim() == 2):
            raise ValueError("VoxelGrid.mean: values must be a (n,c) float32 tensor on the device")
        if values.shape[0] != self.n or not 1 <= values.shape[1] <= _MAX_CHANNELS or values.device != self.count.device:
            raise ValueError(f"VoxelGrid.mean: values {tuple(values.shape)} on {values.device} do not fit {self.n} rows, "
                             f"1 <= c <= {_MAX_CHANNELS}, on {self.count.device}")
        return _Mean.apply(values.contiguous(), self)


@torch.no_grad()
def voxel_grid(coord, voxel_size, offset=None):
    """-> VoxelGrid of coord (n,3) float32 / float64 on the device under voxel_size (a float or three) and the int32
    cumulative `offset` (b) of the clouds (None: one cloud)."""
    if not (torch.is_tensor(coord) and coord.is_cuda and coord.dim() == 2 and coord.shape[1] == 3
            and coord.dtype in (torch.float32, torch.float64) and coord.is_contiguous()):
        raise ValueError("voxel_grid: coord must be a contiguous (n,3) float32 or float64 tensor on the device "
                         "(the extension has no CPU path)")
    n, dev = coord.shape[0], coord.device
    if n >= _MAX_ROWS:
        raise ValueError(f"voxel_grid: {n} rows, the kernels take fewer than 2^27")
    vs = _sizes(voxel_size)
    if offset is None:
        offset = torch.full((1,), n, dtype=torch.int32, device=dev)
    if not (torch.is_tensor(offset) and offset.dtype == torch.int32 and offset.dim() == 1 and offset.shape[0] >= 1
            and offset.device == dev and offset.is_contiguous()):
        raise ValueError("voxel_grid: offset must be a contiguous int32 (b) tensor, b >= 1, on coord's device")
    b = offset.shape[0]
    i32 = dict(dtype=torch.int32, device=dev)
    if n == 0:
        empty = torch.empty(0, **i32)
        return VoxelGrid(0, 0, 0, empty, empty.clone(), empty.clone(), empty.clone(), torch.zeros(b, **i32))
    from . import _lib
    scratch = torch.empty(_lib.load().apn_vg_scratch_ints(n), **i32)
    voxel_of, idx_sort = torch.empty(n, **i32), torch.empty(n, **i32)
    count_start = torch.empty(2, n, **i32)                  # sized for the worst case, sliced to m below
    new_offset, stats = torch.empty(b, **i32), torch.empty(3, **i32)
    _call("apn_vg_voxelize", dev, b, n, int(coord.dtype == torch.float64), coord.data_ptr(), *vs, offset.data_ptr(),
          scratch.data_ptr(), voxel_of.data_ptr(), count_start[0].data_ptr(), count_start[1].data_ptr(),
          idx_sort.data_ptr(), new_offset.data_ptr(), stats.data_ptr())
    m, count_max, bad = stats.tolist()                      # the one host read of the operation
    if bad > 0:
        raise ValueError(f"voxel_grid: {bad} rows have a non-finite coordinate or a cell outside int32 "
                         f"(voxel_size {vs})")
    return VoxelGrid(n, m, count_max, voxel_of, count_start[0, :m], count_start[1, :m], idx_sort, new_offset)


@torch.no_grad()
def voxelize(coord, voxel_size=0.05, hash_type='fnv', mode=0, *, offset=None, draws=None):
    """The reference's `voxelize` on the device, int64 tensors out.  mode 1 -> (idx_sort, voxel_idx, count) with
    voxel_idx[j] the voxel of idx_sort[j] (non-decreasing).  mode 0 -> one row per voxel, idx_sort[start + draws % count]:
    draws=None makes the reference's own host call np.random.randint(0, count_max, m), so a seeded script consumes the
    same host stream; draws='device' draws with torch.randint on the device; a tensor is used as given.  `hash_type` is
    ignored: no hash decides the partition here."""
    grid = voxel_grid(coord, voxel_size, offset)
    if mode != 0:
        order = grid.idx_sort.long()
        return order, grid.voxel_of.long()[order], grid.count.long()
    if draws is None:
        draws = torch.from_numpy(np.random.randint(0, max(grid.count_max, 1), grid.m)).to(coord.device)
    elif isinstance(draws, str):
        if draws != 'device':
            raise ValueError(f"voxelize: draws must be None, 'device' or a tensor, got {draws!r}")
        draws = torch.randint(0, max(grid.count_max, 1), (grid.m,), device=coord.device)
    return grid.pick(draws).long()
