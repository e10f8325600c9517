"""Part-segmentation metrics on the device (csrc/part_metrics.hip): instance and category mIoU without a host loop.

The reference (`examples/shapenetpart/train_adapt.py`) computes `get_ins_mious` (:77-107) in Python, shape by shape and
part by part, with three host reads per (shape, part), then adds every shape's value to its category's cell one
`.cpu()` at a time (`validate`, :576-580): about 25,000 synchronisations over ShapeNetPart's 2,874 test shapes.  Here a
batch is ONE call of `apn_part_ious` -- the argmax over the part logits, per-part intersection and union by integer LDS
atomics, the shape's mean IoU, and the running totals added in ascending shape order -- and `PartMetrics.result` is the
one host read, followed by the reference's closing arithmetic (:582-592):

    cls_mious[k] = cls_sum[k] / cls_num[k]  where cls_num[k] > 0, else the 0 it was initialised with
    ins_miou = ins_sum / ins_num,   cls_miou = mean(cls_mious)          -- a category without a shape contributes 0

`PartSegEvaluator.validate` is `validate` (:536-598) over clouds already on the device: one hipGraph per batch shape,
the last batch padded and masked, the logits averaged over `num_votes + 1` forward passes before the metric.
"""
import numpy as np
import torch

from . import graphs
from .fused import _call

# ShapeNetPart's categories and their part labels (openpoints/dataset/shapenetpart/shapenetpart.py: cls2parts)
SHAPENETPART_CLS2PARTS = ((0, 1, 2, 3), (4, 5), (6, 7), (8, 9, 10, 11), (12, 13, 14, 15), (16, 17, 18), (19, 20, 21),
                          (22, 23), (24, 25, 26, 27), (28, 29), (30, 31, 32, 33, 34, 35), (36, 37), (38, 39, 40),
                          (41, 42, 43), (44, 45, 46), (47, 48, 49))
MAX_PARTS = 64


def csr_table(cls2parts):
    """cls2parts (a list of part-label lists, one per category, in the order the mean runs) -> (offset (S + 1,), ids)
    int32 numpy arrays."""
    offset = np.zeros(len(cls2parts) + 1, np.int32)
    offset[1:] = np.cumsum([len(p) for p in cls2parts])
    ids = np.asarray([int(v) for p in cls2parts for v in p], np.int32)
    return offset, ids


class PartMetrics:
    """The accumulators of one evaluation pass.  `update` takes the LOGITS (the reference's callers pass
    `logits.max(dim=1)[1]`) and makes no host read; `result` makes one."""

    def __init__(self, cls2parts=SHAPENETPART_CLS2PARTS, num_parts=50, device="cuda"):
        cls2parts = [list(p) for p in cls2parts]
        if not cls2parts or any(len(p) == 0 or len(p) > MAX_PARTS for p in cls2parts):
            raise ValueError(f"PartMetrics: every category needs between 1 and {MAX_PARTS} parts")
        if not 1 <= num_parts <= MAX_PARTS or any(not 0 <= v < num_parts for p in cls2parts for v in p):
            raise ValueError(f"PartMetrics: part labels must lie in [0, num_parts), num_parts <= {MAX_PARTS}")
        self.num_parts, self.num_classes = int(num_parts), len(cls2parts)
        offset, ids = csr_table(cls2parts)
        dev = torch.device(device)
        self.offset, self.ids = torch.from_numpy(offset).to(dev), torch.from_numpy(ids).to(dev)
        S = self.num_classes
        self.cls_sum = torch.zeros(S, dtype=torch.float32, device=dev)
        self.cls_num = torch.zeros(S, dtype=torch.int32, device=dev)
        self.ins_sum = torch.zeros(1, dtype=torch.float64, device=dev)
        self.counts = torch.zeros(2, dtype=torch.int32, device=dev)          # {shapes counted, shapes rejected}

    def reset(self):
        for t in (self.cls_sum, self.cls_num, self.ins_sum, self.counts):
            t.zero_()

    @torch.no_grad()
    def update(self, logits, target, cls, valid=None, ious=None):
        """logits (B, num_parts, N) float32 CUDA; target (B, N) and cls (B,) or (B, 1), int32 or int64; valid (B,) int32
        or None: shapes with 0 are padding; ious: an optional (B,) float32 tensor to write into.  -> ious: the shapes'
        mean IoUs (-1 padding, -2 rejected: a class outside the table)."""
        dev = self.cls_sum.device
        if not (logits.dim() == 3 and logits.shape[1] == self.num_parts and logits.dtype == torch.float32
                and logits.device == dev):
            raise ValueError(f"PartMetrics.update: logits must be (B, {self.num_parts}, N) float32 on {dev}")
        B, C, N = logits.shape
        cls = cls.reshape(-1)
        if target.shape != (B, N) or cls.shape != (B,) or target.device != dev or cls.device != dev:
            raise ValueError(f"PartMetrics.update: target must be ({B}, {N}) and cls ({B},) on {dev}")

        def int32(t, bound):
            if t.dtype == torch.int64:
                return t.clamp(-1, bound).to(torch.int32).contiguous()       # out of range stays out of range
            if t.dtype != torch.int32:
                raise ValueError("PartMetrics.update: target and cls must be int32 or int64")
            return t.contiguous()
        target, cls = int32(target, C), int32(cls, self.num_classes)
        if valid is not None and not (valid.dtype == torch.int32 and valid.shape == (B,) and valid.device == dev
                                      and valid.is_contiguous()):
            raise ValueError(f"PartMetrics.update: valid must be a contiguous ({B},) int32 tensor on {dev}")
        if ious is None:
            ious = torch.empty(B, dtype=torch.float32, device=dev)
        elif not (ious.dtype == torch.float32 and ious.shape == (B,) and ious.device == dev and ious.is_contiguous()):
            raise ValueError(f"PartMetrics.update: ious must be a contiguous ({B},) float32 tensor on {dev}")
        _call("apn_part_ious", dev, B, C, N, self.num_classes, self.ids.numel(), logits.contiguous().data_ptr(),
              target.data_ptr(), cls.data_ptr(), self.offset.data_ptr(), self.ids.data_ptr(),
              None if valid is None else valid.data_ptr(), ious.data_ptr(), self.cls_sum.data_ptr(),
              self.cls_num.data_ptr(), self.ins_sum.data_ptr(), self.counts.data_ptr(), self.counts.data_ptr() + 4)
        return ious

    def all_reduce(self):
        """validate :583-584 for a sharded pass: the totals summed over the process group."""
        from .dp import all_reduce_sum_
        for t in (self.cls_sum, self.cls_num, self.ins_sum, self.counts):
            all_reduce_sum_(t)

    def result(self):
        """validate :582-592 -> (ins_miou, cls_miou, cls_mious (S,) float32 numpy).  The one host read."""
        host = torch.cat([self.cls_sum.double(), self.cls_num.double(), self.ins_sum, self.counts.double()]).cpu().numpy()
        S = self.num_classes
        return finish(host[:S].astype(np.float32), host[S:2 * S].astype(np.int32), host[2 * S], int(host[2 * S + 1]),
                      int(host[2 * S + 2]))


def finish(cls_sum, cls_num, ins_sum, ins_num, rejected=0):
    """The closing arithmetic of validate (:586-592) on host numbers: float32 divisions as the reference's tensors do."""
    if rejected:
        raise ValueError(f"PartMetrics: {rejected} shape(s) had a class outside the part table")
    if ins_num == 0:
        raise ValueError("PartMetrics: no shape was counted")
    cls_mious = torch.from_numpy(np.array(cls_sum, np.float32))
    cls_nums = torch.from_numpy(np.array(cls_num, np.int32))
    for k in range(cls_mious.numel()):
        if cls_nums[k] > 0:
            cls_mious[k] = cls_mious[k] / cls_nums[k]
    ins_miou = torch.tensor(float(ins_sum), dtype=torch.float32) / torch.tensor(int(ins_num))
    return ins_miou.item(), torch.mean(cls_mious).item(), cls_mious.numpy()


class _Static:
    """What one captured graph reads and writes: the split (copied in once, outside the graph), the batch's padded rows
    and its valid flags, the accumulators (inside `metrics`), the batch's IoUs."""

    def __init__(self, dev, B, S, n, cx, metrics_args):
        self.S = S
        self.points = torch.zeros(S, n, 3, device=dev)
        self.x = torch.zeros(S, cx, n, device=dev)
        self.y = torch.zeros(S, n, dtype=torch.int32, device=dev)
        self.cls = torch.zeros(S, dtype=torch.int32, device=dev)
        self.rows = torch.zeros(B, dtype=torch.int64, device=dev)
        self.valid = torch.ones(B, dtype=torch.int32, device=dev)
        self.ious = torch.zeros(B, dtype=torch.float32, device=dev)
        self.metrics = PartMetrics(*metrics_args, device=dev)
        self.graph = None
        self.census = None


class PartSegEvaluator:
    """`validate` (train_adapt.py:536-598) over clouds already on the device.

    model: `forward({'pos', 'x', 'cls'})` -> logits (B, num_parts, N), run under eval() and no_grad(), its training flag
    restored afterwards.  The batch body: gather the batch's rows -> for v in 0..num_votes: pos = vote_transform(pos)
    for v > 0 (the reference transforms the already transformed positions; 'x' keeps its first value, as there),
    logits += model(...) -> logits / (num_votes + 1) -> `PartMetrics.update`.  `vote_transform` must be capturable (it
    draws on the device or not at all).  capture: one hipGraph per (batch_size, N, channels, num_votes) replays that
    body; False runs it eagerly.  keep_ious: keep every shape's IoU in `self.ious` ((nb, batch_size), padding -1)."""

    def __init__(self, model, batch_size=32, cls2parts=SHAPENETPART_CLS2PARTS, num_parts=50, capture=True, keep_ious=False):
        self.model, self.batch_size = model, int(batch_size)
        self.metrics_args = (cls2parts, num_parts)
        self.capture, self.keep_ious = bool(capture), bool(keep_ious)
        self.graphs = {}
        self.captures = 0
        self.ious = None

    def _body(self, points, x, y, cls, rows, valid, metrics, ious, num_votes, vote_transform):
        pos = points.index_select(0, rows)
        feat = x.index_select(0, rows)
        label = cls.index_select(0, rows)
        logits = None
        for v in range(num_votes + 1):
            if v > 0:
                pos = vote_transform(pos)
            out = self.model({'pos': pos.contiguous(), 'x': feat, 'cls': label.long().unsqueeze(-1)})
            logits = out if logits is None else logits + out
        if num_votes:
            logits = logits / (num_votes + 1)
        metrics.update(logits, y.index_select(0, rows), label, valid, ious)

    def _check(self, points, x, y, cls):
        ok = (torch.is_tensor(points) and points.is_cuda and points.dtype == torch.float32 and points.dim() == 3
              and points.shape[2] == 3 and points.shape[0] > 0)
        if not ok:
            raise ValueError("PartSegEvaluator: points must be a non-empty (S, N, 3) float32 CUDA tensor")
        S, n, _ = points.shape
        dev = points.device
        if not (torch.is_tensor(x) and x.device == dev and x.dtype == torch.float32 and x.dim() == 3 and x.shape[0] == S
                and x.shape[2] == n):
            raise ValueError(f"PartSegEvaluator: x must be an ({S}, C, {n}) float32 tensor on the points' device")
        cls = cls.reshape(-1)
        integer = (torch.int32, torch.int64)
        if not (y.shape == (S, n) and cls.shape == (S,) and y.device == dev and cls.device == dev and y.dtype in integer
                and cls.dtype in integer):
            raise ValueError(f"PartSegEvaluator: y must be ({S}, {n}) and cls ({S},), integer, on the points' device")
        return S, n, x.shape[1], cls

    def _labels32(self, t, bound):
        return (t.clamp(-1, bound) if t.dtype == torch.int64 else t).to(torch.int32).contiguous()

    def _graph_for(self, dev, S, n, cx, num_votes, vote_transform):
        key = (self.batch_size, n, cx, num_votes)
        st = self.graphs.get(key)
        if st is not None and st.S >= S and st.vote_transform is vote_transform:
            return st
        B = self.batch_size
        st = _Static(dev, B, S, n, cx, self.metrics_args)
        st.vote_transform = vote_transform
        st.rows.copy_(torch.arange(B, device=dev) % S)

        def body():
            self._body(st.points, st.x, st.y, st.cls, st.rows, st.valid, st.metrics, st.ious, num_votes, vote_transform)

        side = torch.cuda.Stream(dev)                  # warm-up (lazy allocations, kernel attributes) off the capture
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            body()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        st.graph, _, st.census = graphs.capture(body, what=f"the part-segmentation evaluation batch (B={B}, N={n})")
        self.captures += 1
        self.graphs[key] = st
        return st

    @torch.no_grad()
    def _run(self, points, x, y, cls, num_votes, vote_transform):
        from .evaluate import batch_plan
        S, n, cx, cls = self._check(points, x, y, cls)
        dev = points.device
        B = self.batch_size
        rows, count = batch_plan(np.arange(S), B)
        nb = rows.shape[0]
        rows_d = torch.from_numpy(rows).to(dev)
        valid_d = torch.from_numpy((np.arange(B)[None, :] < count[:, None]).astype(np.int32)).to(dev)
        num_parts = self.metrics_args[1]
        y32, cls32 = self._labels32(y, num_parts), self._labels32(cls, len(self.metrics_args[0]))
        self.ious = torch.empty(nb, B, dtype=torch.float32, device=dev) if self.keep_ious else None
        if self.capture:
            st = self._graph_for(dev, S, n, cx, num_votes, vote_transform)
            st.points[:S].copy_(points)
            st.x[:S].copy_(x)
            st.y[:S].copy_(y32)
            st.cls[:S].copy_(cls32)
            st.metrics.reset()
            for i in range(nb):
                st.rows.copy_(rows_d[i])
                st.valid.copy_(valid_d[i])
                st.graph.replay()
                if self.ious is not None:
                    self.ious[i].copy_(st.ious)
            return st.metrics
        metrics = PartMetrics(*self.metrics_args, device=dev)
        points, x = points.contiguous(), x.contiguous()
        for i in range(nb):
            self._body(points, x, y32, cls32, rows_d[i], valid_d[i], metrics, None if self.ious is None else self.ious[i],
                       num_votes, vote_transform)
        return metrics

    def validate(self, points, x, y, cls, num_votes=0, vote_transform=None):
        """points (S, N, 3), x (S, C, N), y (S, N) part labels, cls (S,) or (S, 1) categories, all on the device ->
        (ins_miou, cls_miou, cls_mious); the one host read is at the end."""
        if num_votes and vote_transform is None:
            raise ValueError("PartSegEvaluator.validate: num_votes > 0 needs a vote_transform")
        was = self.model.training
        self.model.eval()
        try:
            metrics = self._run(points, x, y, cls, int(num_votes), vote_transform)
        finally:
            self.model.train(was)
        return metrics.result()


__all__ = ["PartMetrics", "PartSegEvaluator", "SHAPENETPART_CLS2PARTS", "csr_table", "finish"]
