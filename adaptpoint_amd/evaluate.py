"""The evaluation half of a training epoch on the GPU: `validate` and the ScanObjectNN-C corruption sweep.

The reference evaluates with examples/classification/train_autoaug.py:528-549 (`validate`, every epoch and twice at the
end) and with `eval_corrupt_wrapper_scanobjectnnc` over `validate_scanobjectnnc` (openpoints/dataset/scanobjectnn_c/
scanobjectnn_c.py:92-167, train_autoaug.py:551-574: 1 clean split + 7 corruptions x 5 levels, every 10 epochs and twice
at the end).  Per batch: the val transform chain, the `[:num_points]` slice, an eval-mode forward, `cm.update(
logits.argmax(dim=1), target)` -- a bincount that reads the host once per batch.

`ConfusionMatrix` is the reference's class (openpoints/utils/metrics.py:51-146, what the trainers call) on the device:
`update` takes LOGITS and is one launch of `apn_cls_confusion` (csrc/cls_metrics.hip: argmax + masked count), no host
read.  `Evaluator` runs the reference's batch body over clouds uploaded once, pads the last batch with copies of its
first row (masked by a device-side valid count), and with `capture=True` replays one hipGraph per (batch, N_raw).
`corruption_summary` is the wrapper's arithmetic on the host, rounding where it rounds.
"""
import math

import numpy as np
import torch

from . import graphs
from .fused import _call
from .transforms import N_PARAMS

# eval_corrupt_wrapper_scanobjectnnc's order (scanobjectnn_c.py:103-112) and the DGCNN overall accuracies its CE / RCE are
# relative to (scanobjectnn_c.py:113-122)
CORRUPTIONS = ('clean', 'scale', 'jitter', 'rotate', 'dropout_global', 'dropout_local', 'add_global', 'add_local')
LEVELS = 5
DGCNN_OA = {
    'clean': 0.858,
    'scale': 0.578,
    'jitter': 0.456,
    'rotate': 0.733,
    'dropout_global': 0.622,
    'dropout_local': 0.697,
    'add_global': 0.540,
    'add_local': 0.773,
}


def split_names():
    """The 36 split names in the wrapper's order: clean, scale_0 .. scale_4, ..., add_local_4."""
    return ['clean'] + [f"{c}_{lv}" for c in CORRUPTIONS[1:] for lv in range(LEVELS)]


def corruption_summary(acc_by_split):
    """The arithmetic of eval_corrupt_wrapper_scanobjectnnc (scanobjectnn_c.py:123-166) over the accuracies of the 36
    splits ({split name: acc}) -> (records, summary): `records` the dicts the wrapper pprints and writes, in its order and
    with its keys (per level {'acc', 'corruption', 'level'}; per corruption {'OA', 'CE', 'RCE', 'corruption', 'level':
    'Overall'}), `summary` = {'mCE', 'RmCE', 'mOA'}.  Every round(..., 3) is where the wrapper has it, CE and RCE included
    (computed from the already rounded OAs)."""
    records = []
    oa_clean = None
    perf_all = {'OA': [], 'CE': [], 'RCE': []}
    for corruption in CORRUPTIONS:
        perf = {'OA': []}
        for level in range(LEVELS):
            split = 'clean' if corruption == 'clean' else f"{corruption}_{level}"
            rec = {'acc': acc_by_split[split]}
            perf['OA'].append(rec['acc'])
            rec['corruption'] = corruption
            if corruption != 'clean':
                rec['level'] = level
            records.append(rec)
            if corruption == 'clean':
                oa_clean = round(rec['acc'], 3)
                break
        perf['OA'] = round(sum(perf['OA']) / len(perf['OA']), 3)
        if corruption != 'clean':
            perf['CE'] = (1 - perf['OA']) / (1 - DGCNN_OA[corruption])
            perf['RCE'] = (oa_clean - perf['OA']) / (DGCNN_OA['clean'] - DGCNN_OA[corruption])
            for k in perf_all:
                perf[k] = round(perf[k], 3)
                perf_all[k].append(perf[k])
        perf['corruption'] = corruption
        perf['level'] = 'Overall'
        records.append(perf)
    for k in perf_all:
        perf_all[k] = round(sum(perf_all[k]) / len(perf_all[k]), 3)
    summary = {'mCE': perf_all.pop('CE'), 'RmCE': perf_all.pop('RCE'), 'mOA': perf_all.pop('OA')}
    return records, summary


def distributed_indices(S, world=1, rank=0):
    """torch.utils.data.DistributedSampler(range(S), num_replicas=world, rank=rank, shuffle=False) (the reference's val
    sampler, openpoints/dataset/build.py:77-95): the index list padded by wrapping to ceil(S / world) * world, then every
    world-th index from rank on."""
    if world < 1 or not 0 <= rank < world:
        raise ValueError(f"distributed_indices: needs world >= 1 and 0 <= rank < world (got {world}, {rank})")
    idx = list(range(S))
    total = int(math.ceil(S / world)) * world
    pad = total - S
    if pad <= len(idx):
        idx += idx[:pad]
    else:
        idx += (idx * int(math.ceil(pad / len(idx))))[:pad]
    return idx[rank:total:world]


def batch_plan(order, batch_size):
    """The batches of an index list: rows (nb, batch_size) int64, each batch's rows with the last batch padded by copies
    of its first row, and valid (nb,) int64, how many rows of each batch count."""
    order = np.asarray(order, np.int64).reshape(-1)
    nb = -(-order.size // batch_size)
    rows = np.empty((nb, batch_size), np.int64)
    valid = np.empty(nb, np.int64)
    for i in range(nb):
        part = order[i * batch_size:(i + 1) * batch_size]
        rows[i, :part.size] = part
        rows[i, part.size:] = part[0]
        valid[i] = part.size
    return rows, valid


class ConfusionMatrix:
    """openpoints/utils/metrics.py:51-146 on the device, for what the trainers call.  `update` takes the LOGITS (the
    reference's callers pass `logits.argmax(dim=1)`) and is one launch with no host read.  The counters are k*k + 1
    int64 cells: `value` is a (k, k) view of the first k*k, the last counts rows whose label lies outside [0, k) --
    where the reference's `view(K, K)` raises, `all_acc` raises."""

    def __init__(self, num_classes, device, counts=None):
        self.num_classes = int(num_classes)
        k = self.num_classes
        if counts is None:
            counts = torch.zeros(k * k + 1, dtype=torch.int64, device=device)
        if counts.dtype != torch.int64 or counts.shape != (k * k + 1,):
            raise ValueError(f"ConfusionMatrix: counts must be ({k * k + 1},) int64")
        self.counts = counts

    @torch.no_grad()
    def update(self, logits, target, valid=None, pred=None):
        """logits (B, k) float32 CUDA (rows may be strided); target (B,) int32 or int64; valid: a device int32 scalar,
        only rows below it count (None: all); pred: an optional (B,) int32 tensor for the argmax of every row."""
        k = self.num_classes
        dev = self.counts.device
        if not (logits.dim() == 2 and logits.shape[1] == k and logits.dtype == torch.float32 and logits.device == dev):
            raise ValueError(f"ConfusionMatrix.update: logits must be (B, {k}) float32 on {dev}")
        if logits.stride(1) != 1 or logits.stride(0) < k:
            logits = logits.contiguous()
        B = logits.shape[0]
        if target.shape != (B,) or target.device != dev:
            raise ValueError(f"ConfusionMatrix.update: target must be ({B},) on {dev}")
        if target.dtype == torch.int64:
            target = target.clamp(-1, k).to(torch.int32)          # out-of-range labels stay out of range, no host read
        elif target.dtype != torch.int32:
            raise ValueError("ConfusionMatrix.update: target must be int32 or int64")
        target = target.contiguous()
        if valid is not None and not (valid.dtype == torch.int32 and valid.numel() == 1 and valid.device == dev):
            raise ValueError("ConfusionMatrix.update: valid must be a one-element int32 tensor on the logits' device")
        if pred is not None and not (pred.dtype == torch.int32 and pred.shape == (B,) and pred.is_contiguous()
                                     and pred.device == dev):
            raise ValueError(f"ConfusionMatrix.update: pred must be a contiguous ({B},) int32 tensor")
        _call("apn_cls_confusion", dev, B, k, logits.data_ptr(), logits.stride(0), target.data_ptr(),
              None if valid is None else valid.data_ptr(), self.counts.data_ptr(),
              None if pred is None else pred.data_ptr())
        return pred

    def reset(self):
        self.counts.zero_()

    @property
    def value(self):
        k = self.num_classes
        return self.counts[:k * k].view(k, k)

    @property
    def rejected(self):
        """The number of counted rows whose label was outside [0, k) (a device scalar)."""
        return self.counts[-1]

    @property
    def tp(self):
        return self.value.diag()

    @property
    def count(self):
        return self.value.sum(dim=1)

    @property
    def total(self):
        return self.value.sum()

    @property
    def overall_accuray(self):
        return self.tp.sum() / self.total

    def all_acc(self):
        bad = int(self.rejected.item())
        if bad:
            raise ValueError(f"ConfusionMatrix: {bad} counted row(s) had a label outside [0, {self.num_classes})")
        return self.cal_acc(self.tp, self.count)

    @staticmethod
    def cal_acc(tp, count):
        """metrics.py:141-146: the same float32 torch ops on the same int64 tensors."""
        acc_per_cls = tp / count.clamp(min=1) * 100
        over_all_acc = tp.sum() / count.sum() * 100
        macc = torch.mean(acc_per_cls)
        return macc.item(), over_all_acc.item(), acc_per_cls.cpu().numpy()


class _Static:
    """What one captured graph reads and writes: the split's clouds and labels (copied in once per split, outside the
    graph), the batch's padded rows + valid count, the counters, the batch's predictions."""

    def __init__(self, dev, B, S, n_raw, k):
        self.S = S
        self.raw = torch.zeros(S, n_raw, 3, device=dev)
        self.labels = torch.zeros(S, dtype=torch.int32, device=dev)
        self.batch = torch.zeros(B + 1, dtype=torch.int32, device=dev)
        self.counts = torch.zeros(k * k + 1, dtype=torch.int64, device=dev)
        self.pred = torch.zeros(B, dtype=torch.int32, device=dev)
        self.graph = None
        self.census = None


class Evaluator:
    """`validate` (train_autoaug.py:528-549) and `corruption_sweep` (scanobjectnn_c.py:92-167 over
    validate_scanobjectnnc, train_autoaug.py:551-574) over clouds already on the device.

    model: the classifier (`forward({'pos', 'x'})` -> logits), run under eval() and no_grad(), its training flag restored
    afterwards.  transform: a `transforms.CloudTransform` with num_points=None and a chain that draws nothing (the val
    and ScanObjectNN-C chains).  The batch body: transform -> [:, :num_points] -> pos = [..., :3], x = [...,
    :in_channels]^T -> model -> `ConfusionMatrix.update`.  capture: one hipGraph per (batch_size, N_raw) replays that
    body; False runs it eagerly (the test reference of the captured path).  keep_pred: keep every batch's predictions
    in `self.pred` ((nb, batch_size) int32, padding rows included)."""

    def __init__(self, model, transform, batch_size=64, num_points=1024, in_channels=4, capture=True, num_classes=15,
                 keep_pred=False):
        if transform.shuffle or transform.scaling or transform.rotation:
            raise ValueError("Evaluator: the transform must draw nothing (the val / ScanObjectNN-C chains)")
        if transform.num_points is not None:
            raise ValueError("Evaluator: the transform must keep every stored point (num_points=None); the evaluator "
                             "slices [:num_points] after it")
        self.model, self.transform = model, transform
        self.batch_size, self.num_points, self.in_channels = int(batch_size), int(num_points), int(in_channels)
        self.capture, self.num_classes, self.keep_pred = bool(capture), int(num_classes), bool(keep_pred)
        self.graphs = {}               # (batch_size, N_raw) -> _Static
        self.captures = 0
        self.pred = None
        self._identity = {}

    # ------------------------------------------------------------------------------------------------ batch body
    def _params(self, dev):
        """The identity parameter block (B, 12) on the device: the transform then makes no host-to-device copy."""
        if dev not in self._identity:
            p = np.zeros((self.batch_size, N_PARAMS), np.float32)
            p[:, :3] = 1.0
            p[:, 3:] = np.eye(3, dtype=np.float32).reshape(-1)
            self._identity[dev] = torch.from_numpy(p).to(dev)
        return self._identity[dev]

    def _body(self, raw, labels, rows, valid, counts, pred):
        B = self.batch_size
        x = self.transform(raw, rows, draws=(None, self._params(raw.device)))
        x = x[:, :self.num_points]
        pos = x[:, :, :3].contiguous()
        feat = x[:, :, :self.in_channels].transpose(1, 2).contiguous()
        logits = self.model({'pos': pos, 'x': feat})
        target = labels.index_select(0, rows)
        ConfusionMatrix(self.num_classes, raw.device, counts).update(logits.view(B, -1), target, valid, pred)

    # ----------------------------------------------------------------------------------------------------- a split
    def _check(self, points, labels):
        if not (torch.is_tensor(points) and points.is_cuda and points.dtype == torch.float32 and points.dim() == 3
                and points.shape[2] == 3):
            raise ValueError("Evaluator: points must be an (S, N_raw, 3) float32 CUDA tensor")
        S, n_raw, _ = points.shape
        if not (torch.is_tensor(labels) and labels.device == points.device and labels.shape == (S,)
                and labels.dtype in (torch.int32, torch.int64)):
            raise ValueError(f"Evaluator: labels must be an ({S},) integer tensor on the points' device")
        if S == 0:
            raise ValueError("Evaluator: the split holds no cloud")
        if not 0 < self.num_points <= n_raw:
            raise ValueError(f"Evaluator: num_points={self.num_points} needs N_raw >= num_points (got {n_raw})")
        return S, n_raw

    def _labels32(self, labels):
        k = self.num_classes
        return (labels.clamp(-1, k) if labels.dtype == torch.int64 else labels).to(torch.int32).contiguous()

    def _graph_for(self, dev, S, n_raw):
        """The captured body for (batch_size, n_raw); recaptured only if a split holds more clouds than its buffers."""
        key = (self.batch_size, n_raw)
        st = self.graphs.get(key)
        if st is not None and st.S >= S:
            return st
        st = _Static(dev, self.batch_size, S, n_raw, self.num_classes)
        B = self.batch_size
        st.batch[:B] = torch.arange(B, dtype=torch.int32, device=dev) % S
        st.batch[B] = B

        def body():
            self._body(st.raw, st.labels, st.batch[:B], st.batch[B:], st.counts, st.pred)

        side = torch.cuda.Stream(dev)                  # warm-up (lazy allocations, kernel attributes) off the capture
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            body()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        st.graph, _, st.census = graphs.capture(body, what=f"the evaluation batch (B={B}, N_raw={n_raw})")
        self.captures += 1
        self.graphs[key] = st
        return st

    @torch.no_grad()
    def _run(self, points, labels, order):
        dev = points.device
        S, n_raw = self._check(points, labels)
        B = self.batch_size
        rows, valid = batch_plan(order, B)
        nb = rows.shape[0]
        plan = torch.from_numpy(np.concatenate([rows, valid[:, None]], 1).astype(np.int32)).to(dev)
        self.pred = torch.empty(nb, B, dtype=torch.int32, device=dev) if self.keep_pred else None
        if self.capture:
            st = self._graph_for(dev, S, n_raw)
            st.raw[:S].copy_(points)
            st.labels[:S].copy_(self._labels32(labels))
            st.counts.zero_()
            for i in range(nb):
                st.batch.copy_(plan[i])
                st.graph.replay()
                if self.pred is not None:
                    self.pred[i].copy_(st.pred)
            counts = st.counts.clone()
        else:
            points, labels32 = points.contiguous(), self._labels32(labels)
            counts = torch.zeros(self.num_classes ** 2 + 1, dtype=torch.int64, device=dev)
            for i in range(nb):
                self._body(points, labels32, plan[i, :B], plan[i, B:], counts, None if self.pred is None else self.pred[i])
        return ConfusionMatrix(self.num_classes, dev, counts)

    def _eval_mode(self):
        was = self.model.training
        self.model.eval()
        return was

    def validate(self, points, labels, rank=0, world=1):
        """train_autoaug.py:528-549 over points (S, N_raw, 3) and labels (S,), both on the device.  rank / world: the
        reference's DistributedSampler(shuffle=False) share; the counters are then summed over the process group (when
        one is initialised and world > 1).  -> (macc, oa, accs, cm); the one host read is at the end."""
        S, _ = self._check(points, labels)
        was = self._eval_mode()
        try:
            cm = self._run(points, labels, distributed_indices(S, world, rank))
        finally:
            self.model.train(was)
        if world > 1:
            import torch.distributed as dist
            if dist.is_available() and dist.is_initialized():
                from .dp import all_reduce_sum_
                all_reduce_sum_(cm.counts)
        macc, oa, accs = cm.all_acc()
        return macc, oa, accs, cm

    def corruption_sweep(self, splits):
        """eval_corrupt_wrapper_scanobjectnnc over validate_scanobjectnnc: `splits` maps the 36 split names (`clean`,
        `scale_0` ... `add_local_4`) to (points, labels) on the device; each split's accuracy is oa / 100.  Not sharded.
        -> (records, summary) as `corruption_summary` gives them."""
        missing = [s for s in split_names() if s not in splits]
        if missing:
            raise KeyError(f"corruption_sweep: split(s) missing: {', '.join(missing)}")
        acc = {}
        for name in split_names():
            _, oa, _, _ = self.validate(*splits[name])
            acc[name] = oa / 100
        return corruption_summary(acc)


__all__ = ["ConfusionMatrix", "Evaluator", "corruption_summary", "distributed_indices", "batch_plan", "split_names",
           "DGCNN_OA", "CORRUPTIONS"]
