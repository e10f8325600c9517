"""Scene segmentation (S3DIS-style): `BaseSeg`, its loss, metric, training step, validation, the whole-scene test loop
and the training crop, with the per-point work outside the network on the device (csrc/scene_seg.hip).

Host-side mirror of the reference's PointNeXt scene-segmentation stack:

  `BaseSeg`             openpoints/models/segmentation/base_seg.py:14-50 over `pointnext.PointNextEncoder`,
                        `pointnext.PointNextDecoder` and `partseg.SegHead` (which already has `global_feat`)
  `SmoothCrossEntropy`  openpoints/loss/build.py:12-63 with `ignore_index`: the valid-row selection and the
                        `reducing_list` remap, statement for statement
  `SegMetrics`          openpoints/utils/metrics.py:51-166 (`ConfusionMatrix`) and `get_mious` (:169-176) over
                        `apn_ss_confusion`: `update` takes the LOGITS (B,C,N) and makes no host read
  `SegStep`             one iteration of `train_one_epoch` (examples/segmentation/main.py:334-385), step_per_update = 1
  `validate`            main.py:389-430
  `SceneTester`         `test` (main.py:507-668) and `load_data` (:64-109) for a scene already on the device
  `SceneSampler`        `crop_pc` (openpoints/dataset/data_util.py:146-174) for split='train', variable=False, and the
                        heights of openpoints/dataset/s3dis/s3dis.py:140-141

Classes, parameters and buffers carry the reference's names (`encoder.encoder.<i>...`, `decoder.decoder.<i>.0.convs...`,
`head.head.<i>...`): a reference `state_dict` loads with strict=True.

The vote merge.  The reference concatenates every sub-cloud's logits and calls torch_scatter's `scatter(..., 'mean')`,
float atomics in an order nobody can restate.  `Votes` streams instead: `add` after every forward does
acc[rows] += logits.T with plain loads and stores -- a sub-cloud's rows are distinct, which the kernel proves with a
stamp exchange -- so a point's sum is the sequence of fp32 adds in CALL ORDER; `finish` divides once by max(cnt, 1)
(torch_scatter's clamp_(1) and true_divide_), takes the argmax and adds the confusion counters.  The host reads
{duplicates, rejected} once per scene, after `finish`, and raises ValueError if either is non-zero.

The crop.  The reference's voxel order (a hash key, then numpy's unstable argsort) is unmatchable, as voxel_grid.py
explains, so row numbers after the voxel pick differ from the reference's and `SceneSampler` is `crop_pc`'s analogue, not
its twin: the same partition, the same draws from the same host stream in the same order (draws=None), the same
nearest-`voxel_max` SET around the drawn centre (`crop_nearest`: numpy's float32 distance, ties by ascending row), the
same shuffle and shifts.

Composed fall-backs -- CPU tensors, other dtypes, more than 64 classes -- are plain torch, counted by reason in
COMPOSED_CALLS, and are what the tests compare the kernels against.

Outside this module's scope: the colour and geometry training transforms (`ChromaticAutoContrast`, `ColorDrop`, ...),
`validate_sphere`, `VariableSeg` and the stacked-layout encoders, ScanNet / SemanticKITTI file handling, fused loss
kernels.
"""
import numpy as np
import torch
import torch.nn as nn

from . import partseg
from .partseg import SegHead
from .pointnext import PointNextDecoder, PointNextEncoder
from .voxel_grid import VoxelGrid, _sizes

# cfgs/s3dis/pointnext-s.yaml of the PointNeXt release: BaseSeg = PointNextEncoder + PointNextDecoder + SegHead
POINTNEXT_S_ENCODER = dict(blocks=(1, 1, 1, 1, 1), strides=(1, 4, 4, 4, 4), width=32, in_channels=4, sa_layers=2,
                           sa_use_res=True, radius=0.1, nsample=32, expansion=4,
                           aggr_args={'feature_type': 'dp_fj', 'reduction': 'max'},
                           group_args={'NAME': 'ballquery', 'normalize_dp': True}, conv_args={'order': 'conv-norm-act'},
                           act_args={'act': 'relu'}, norm_args={'norm': 'bn'})
POINTNEXT_S_DECODER = dict()
POINTNEXT_S_HEAD = dict(num_classes=13, norm_args={'norm': 'bn'})

MAX_CLASSES = 64           # apn_ss_max_classes(): the LDS histogram of the counting kernels
_MAX_ROWS = 2 ** 27

# calls that ran the composition instead of a kernel, by reason
COMPOSED_CALLS = {}


def _call(name, dev, *args):
    from .fused import _call as call
    call(name, dev, *args)


def _composed(why):
    COMPOSED_CALLS[why] = COMPOSED_CALLS.get(why, 0) + 1


def _why_composed(values, num_classes, fused=True):
    """Why these float values (logits / coordinates) cannot take the kernels (None: they can)."""
    if not fused:
        return "fused=False"
    if not values.is_cuda:
        return "CPU tensor"
    if values.dtype != torch.float32:
        return f"dtype {values.dtype}"
    if num_classes is not None and num_classes > MAX_CLASSES:
        return f"more than {MAX_CLASSES} classes"
    return None


def _labels32(t, bound):
    """int32 labels for a kernel: int64 ones clamped to [-1 - 2^30, 2^30] first, so that no label changes its meaning
    (in range, the ignored label, out of range) -- `bound` is the largest value that must survive."""
    if t.dtype == torch.int64:
        lim = max(int(bound), 0) + 2 ** 30
        return t.clamp(-lim, lim).to(torch.int32).contiguous()
    if t.dtype != torch.int32:
        raise ValueError("labels must be int32 or int64")
    return t.contiguous()


# ------------------------------------------------------------------------------------------------------------- model
class BaseSeg(nn.Module):
    """base_seg.py:14-50: `encoder`, `decoder`, `head`; the decoder's arguments are the encoder's updated by
    `decoder_args`.  Defaults: PointNeXt-S for S3DIS (13 classes, 4 input channels).  fused: the encoder's blocks and the
    head on the fused kernels; hoisted: every propagation block in `adaptpoint_amd.propagation`'s form; sync_bn: the
    encoder's BatchNorm statistics over the process group.  forward(data) with {'pos' (B,N,3), 'x' (B,C,N)} (or
    forward(pos, x)) -> logits (B, num_classes, N)."""

    def __init__(self, encoder_args=None, decoder_args=None, cls_args=None, fused=False, hoisted=False, sync_bn=False):
        super().__init__()
        encoder_args = dict(POINTNEXT_S_ENCODER if encoder_args is None else encoder_args)
        decoder_args = dict(POINTNEXT_S_DECODER if decoder_args is None else decoder_args)
        cls_args = dict(POINTNEXT_S_HEAD if cls_args is None else cls_args)
        for d in (encoder_args, decoder_args, cls_args):
            d.pop('NAME', None)
        self.encoder = PointNextEncoder(fused=fused, sync_bn=sync_bn, **encoder_args)
        merged = dict(encoder_args)
        merged.update(decoder_args)
        taken = {k: merged[k] for k in ('decoder_layers', 'decoder_stages', 'in_channels') if k in merged}
        self.decoder = PointNextDecoder(self.encoder.channel_list, hoisted=hoisted, **taken)
        cls_args['in_channels'] = self.decoder.out_channels
        self.head = SegHead(fused=fused, **cls_args)

    def forward(self, data, f0=None):
        p, f = self.encoder.forward_seg_feat(data, f0)
        return self.head(self.decoder(p, f).squeeze(-1))


# -------------------------------------------------------------------------------------------------------------- loss
class SmoothCrossEntropy(partseg.SmoothCrossEntropy):
    """openpoints/loss/build.py:12-63 with `ignore_index`: rows whose label equals it are dropped (a boolean selection:
    one host synchronisation, as in the reference), the rest remapped through `reducing_list` =
    cat(r[:ignore_index], [0], r[ignore_index:]) for r = 0..num_classes -- Python slicing as the reference writes it, so
    an ignore_index >= num_classes leaves labels unchanged and a NEGATIVE one shifts the list exactly as it does there.
    return_valid: -> (loss, selected logits (M,C), remapped labels (M,))."""

    def __init__(self, label_smoothing=0.2, ignore_index=None, num_classes=None, weight=None, return_valid=False):
        super().__init__(label_smoothing, weight)
        self.ignore_index, self.return_valid = ignore_index, return_valid
        reducing = None
        if ignore_index is not None:
            if num_classes is None:
                raise ValueError("SmoothCrossEntropy: ignore_index needs num_classes")
            r = torch.arange(0, num_classes + 1, dtype=torch.int64)             # torch.range(0, num_classes): inclusive
            reducing = torch.cat([r[:ignore_index], torch.zeros(1, dtype=torch.int64), r[ignore_index:]], 0)
        self.register_buffer('reducing_list', reducing, persistent=False)

    def forward(self, pred, gt):
        if pred.dim() > 2:
            pred = pred.transpose(1, 2).reshape(-1, pred.shape[1])
        gt = gt.contiguous().view(-1)
        if self.ignore_index is not None:
            valid_idx = gt != self.ignore_index
            pred = pred[valid_idx, :]
            gt = gt[valid_idx]
            gt = torch.gather(self.reducing_list, 0, gt)
        loss = super().forward(pred, gt)
        return (loss, pred, gt) if self.return_valid else loss


# ------------------------------------------------------------------------------------------------------------ metric
def _pack_read(scalars, vectors):
    """One host read of device scalars and vectors (float64 holds every float32 and every count below 2^53)."""
    flat = torch.cat([torch.stack([s.double() for s in scalars])] + [v.double().reshape(-1) for v in vectors]).cpu().numpy()
    out, at = [float(v) for v in flat[:len(scalars)]], len(scalars)
    for v in vectors:
        out.append(flat[at:at + v.numel()].astype(np.float32))
        at += v.numel()
    return out


def get_mious(tp, union, count):
    """metrics.py:169-176: the same float32 torch operations on the same int64 tensors, read with one transfer.
    -> (miou, macc, oa, ious, accs)."""
    iou_per_cls = (tp + 1e-10) / (union + 1e-10) * 100
    acc_per_cls = (tp + 1e-10) / (count + 1e-10) * 100
    over_all_acc = tp.sum() / count.sum() * 100
    miou = torch.mean(iou_per_cls)
    macc = torch.mean(acc_per_cls)
    return tuple(_pack_read([miou, macc, over_all_acc], [iou_per_cls, acc_per_cls]))


def count_composed(counts, pred, target, num_classes, ignore_index=None, keep=None):
    """The counters in plain torch: counts[t * C + p] += 1 for every kept point whose target t is not the ignored label;
    a target outside [0, C) adds to counts[C * C]."""
    C = num_classes
    pred, target = pred.reshape(-1).long(), target.reshape(-1).long()
    inside = (target >= 0) & (target < C)
    cell = torch.where(inside, target * C + pred, torch.full_like(target, C * C))
    drop = torch.zeros_like(inside) if keep is None else ~keep.reshape(-1)
    if ignore_index is not None:
        drop = drop | (target == ignore_index)
    cell = torch.where(drop, torch.full_like(cell, C * C + 1), cell)
    counts += torch.bincount(cell, minlength=C * C + 2)[:C * C + 1]


class SegMetrics:
    """The reference's `ConfusionMatrix` (metrics.py:51-166) on the device.  `update` takes the LOGITS (B,C,N) (the
    reference's callers pass `logits.argmax(dim=1)`) and is one launch of `apn_ss_confusion`, no host read.  The
    counters are C*C + 1 int64 cells: `value` is a (C,C) view of the first C*C; the last, `rejected`, counts points whose
    label lies outside [0,C) and is not `ignore_index` -- where the reference's bincount view raises, `all_metrics`
    raises.  Points labelled `ignore_index` are skipped: the reference maps them to a virtual class and slices it away."""

    def __init__(self, num_classes, ignore_index=None, device="cuda", counts=None, fused=True):
        self.num_classes = int(num_classes)
        self.ignore_index = None if ignore_index is None else int(ignore_index)
        self.fused = fused
        C = self.num_classes
        if C < 1:
            raise ValueError("SegMetrics: num_classes must be positive")
        if counts is None:
            counts = torch.zeros(C * C + 1, dtype=torch.int64, device=device)
        if counts.dtype != torch.int64 or counts.shape != (C * C + 1,):
            raise ValueError(f"SegMetrics: counts must be ({C * C + 1},) int64")
        self.counts = counts

    def _ignore_args(self):
        return (0, 0) if self.ignore_index is None else (self.ignore_index, 1)

    @torch.no_grad()
    def update(self, logits, target, valid=None, pred=None):
        """logits (B,C,N) float32; target (B,N) (or (B,N,1)) int32 or int64; valid: a one-element int32 tensor, only
        clouds below it count (None: all); pred: an optional contiguous (B,N) int32 tensor for every point's argmax."""
        C, dev = self.num_classes, self.counts.device
        if not (logits.dim() == 3 and logits.shape[1] == C and logits.device == dev):
            raise ValueError(f"SegMetrics.update: logits must be (B, {C}, N) on {dev}")
        B, _, N = logits.shape
        if target.dim() == 3 and target.shape[-1] == 1:
            target = target.squeeze(-1)
        if target.shape != (B, N) or target.device != dev or target.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"SegMetrics.update: target must be ({B}, {N}) int32 or int64 on {dev}")
        if valid is not None and not (valid.dtype == torch.int32 and valid.numel() == 1 and valid.device == dev):
            raise ValueError("SegMetrics.update: valid must be a one-element int32 tensor on the logits' device")
        if pred is not None and not (pred.dtype == torch.int32 and pred.shape == (B, N) and pred.is_contiguous()
                                     and pred.device == dev):
            raise ValueError(f"SegMetrics.update: pred must be a contiguous ({B}, {N}) int32 tensor")
        why = _why_composed(logits, C, self.fused)
        if why is None and B > 65535:
            why = "more than 65535 clouds"
        if why is not None:
            _composed(why)
            p = logits.argmax(dim=1)
            if pred is not None:
                pred.copy_(p)
            keep = None
            if valid is not None:
                keep = (torch.arange(B, device=dev) < valid.reshape(()).clamp(0, B)).unsqueeze(1).expand(B, N)
            count_composed(self.counts, p, target, C, self.ignore_index, keep)
            return pred
        ign = self._ignore_args()
        logits, target = logits.contiguous(), _labels32(target, max(C, abs(ign[0])))     # (held until the launch is queued)
        _call("apn_ss_confusion", dev, B, C, N, logits.data_ptr(), target.data_ptr(), *ign,
              None if valid is None else valid.data_ptr(), self.counts.data_ptr(), None if pred is None else pred.data_ptr())
        return pred

    def reset(self):
        self.counts.zero_()

    def add(self, other):
        """`all_cm.value += cm.value` (main.py:657), the rejected cell included."""
        self.counts += other.counts.to(self.counts.device)

    @property
    def value(self):
        C = self.num_classes
        return self.counts[:C * C].view(C, C)

    @property
    def rejected(self):
        """The number of counted points whose label was outside [0,C) and not ignored (a device scalar)."""
        return self.counts[-1]

    @property
    def tp(self):
        return self.value.diag()

    @property
    def actual(self):
        return self.value.sum(dim=1)

    @property
    def predicted(self):
        return self.value.sum(dim=0)

    @property
    def fn(self):
        return self.actual - self.tp

    @property
    def fp(self):
        return self.predicted - self.tp

    @property
    def count(self):
        return self.value.sum(dim=1)

    @property
    def union(self):
        return self.value.sum(dim=0) + self.value.sum(dim=1) - self.value.diag()

    @property
    def total(self):
        return self.value.sum()

    @property
    def overall_accuray(self):
        return self.tp.sum() / self.total

    def _checked(self, scalars, vectors):
        out = _pack_read([self.rejected] + scalars, vectors)
        if out[0]:
            raise ValueError(f"SegMetrics: {int(out[0])} counted point(s) had a label outside [0, {self.num_classes})"
                             + ("" if self.ignore_index is None else f" other than {self.ignore_index}"))
        return tuple(out[1:])

    def all_acc(self):
        """metrics.py:138-146 -> (macc, oa, accs); one host read."""
        tp, count = self.tp, self.count
        acc_per_cls = tp / count.clamp(min=1) * 100
        over_all_acc = tp.sum() / count.sum() * 100
        return self._checked([torch.mean(acc_per_cls), over_all_acc], [acc_per_cls])

    def all_metrics(self):
        """metrics.py:157-166 -> (miou, macc, oa, ious, accs); one host read."""
        tp, fp, fn = self.tp, self.fp, self.fn
        iou_per_cls = tp / (tp + fp + fn).clamp(min=1) * 100
        acc_per_cls = tp / self.count.clamp(min=1) * 100
        over_all_acc = tp.sum() / self.total * 100
        return self._checked([torch.mean(iou_per_cls), torch.mean(acc_per_cls), over_all_acc], [iou_per_cls, acc_per_cls])

    def mious(self):
        """`get_mious(cm.tp, cm.union, cm.count)` as validate and test close (main.py:425-428, :651-652, :664-667), with
        the rejected cell checked in the same host read."""
        tp, union, count = self.tp, self.union, self.count
        iou_per_cls = (tp + 1e-10) / (union + 1e-10) * 100
        acc_per_cls = (tp + 1e-10) / (count + 1e-10) * 100
        over_all_acc = tp.sum() / count.sum() * 100
        return self._checked([torch.mean(iou_per_cls), torch.mean(acc_per_cls), over_all_acc], [iou_per_cls, acc_per_cls])


# -------------------------------------------------------------------------------------------------- step and validate
class SegStep:
    """One iteration of `train_one_epoch` (main.py:334-385) for step_per_update = 1: forward, loss, backward, optional
    `grad_sync`, gradient-norm clipping, AdamW, zero_grad.  data = {'pos' (B,N,3), 'x' (B,C,N), 'y' (B,N)} on the device.
    metrics: a `SegMetrics` updated from the step's logits (`cm.update(logits.argmax(dim=1), target)`, :378) with no host
    read.  optimizer= / grad_sync= as `partseg.PartSegStep` takes them."""

    def __init__(self, model, criterion=None, lr=1e-3, weight_decay=1e-4, grad_norm_clip=10.0, optimizer=None,
                 grad_sync=None, metrics=None):
        self.model = model
        self.criterion = SmoothCrossEntropy(label_smoothing=0.2) if criterion is None else criterion
        self.grad_sync, self.clip, self.metrics = grad_sync, grad_norm_clip, metrics
        self.opt = optimizer or torch.optim.AdamW(model.parameters(), lr=lr, weight_decay=weight_decay)

    def __call__(self, data):
        """-> (logits, loss), both detached."""
        self.model.train()
        target = data['y'].squeeze(-1) if data['y'].dim() == 3 else data['y']
        logits = self.model({'pos': data['pos'], 'x': data['x']})
        loss = self.criterion(logits, target.long())
        loss.backward()
        if self.grad_sync is not None:
            self.grad_sync([q.grad for q in self.model.parameters() if q.grad is not None])
        if self.clip is not None and self.clip > 0:
            nn.utils.clip_grad_norm_(self.model.parameters(), self.clip, norm_type=2)
        self.opt.step()
        self.model.zero_grad()
        if self.metrics is not None:
            self.metrics.update(logits.detach(), target)
        return logits.detach(), loss.detach()


@torch.no_grad()
def validate(model, batches, metrics):
    """main.py:389-430: eval mode (the training flag restored afterwards), one `SegMetrics.update` per batch
    {'pos','x','y'}, then `get_mious(cm.tp, cm.union, cm.count)` -> (miou, macc, oa, ious, accs): the one host read."""
    was = model.training
    model.eval()
    try:
        for data in batches:
            metrics.update(model({'pos': data['pos'], 'x': data['x']}), data['y'])
    finally:
        model.train(was)
    return metrics.mious()


# -------------------------------------------------------------------------------------------------- the vote merge
class Votes:
    """The streamed `scatter(all_logits, idx_points, dim=0, reduce='mean')` of one scene of n points (see the module's
    docstring).  add(logits (C,n_part), rows (n_part)) after every forward; finish(...) once."""

    def __init__(self, n, num_classes, device, fused=True, dtype=torch.float32):
        self.n, self.num_classes, self.fused = int(n), int(num_classes), fused
        dev = torch.device(device)
        self.acc = torch.zeros(self.n, self.num_classes, dtype=dtype, device=dev)
        self.cnt = torch.zeros(self.n, dtype=torch.int32, device=dev)
        self.stamp = torch.zeros(self.n, dtype=torch.int32, device=dev)
        self.flags = torch.zeros(2, dtype=torch.int32, device=dev)            # {duplicates, rejected}
        self.calls = 0

    @torch.no_grad()
    def add(self, logits, rows):
        C, n = self.num_classes, self.n
        if not (logits.dim() == 2 and logits.shape[0] == C and rows.shape == (logits.shape[1],)
                and logits.device == self.acc.device and rows.device == self.acc.device
                and rows.dtype in (torch.int32, torch.int64)):
            raise ValueError(f"Votes.add: logits must be ({C}, n_part) and rows (n_part,) integers on {self.acc.device}")
        self.calls += 1
        why = _why_composed(logits, None, self.fused)
        if why is None and self.acc.dtype != torch.float32:
            why = f"dtype {self.acc.dtype}"
        if why is not None:
            _composed(why)
            rows = rows.long()
            ok = (rows >= 0) & (rows < n)
            at = torch.arange(rows.numel(), device=rows.device)
            first = torch.full((n,), rows.numel(), dtype=torch.int64, device=rows.device)
            first.scatter_reduce_(0, rows[ok], at[ok], 'amin')
            once = ok.clone()
            once[ok] = first[rows[ok]] == at[ok]                               # the first occurrence of every row
            self.flags += torch.stack([(ok & ~once).sum(), (~ok).sum()]).to(torch.int32)
            # distinct rows: index_add_ is one add per address, whatever its order
            self.acc.index_add_(0, rows[once], logits.t()[once].to(self.acc.dtype))
            self.cnt.index_add_(0, rows[once], torch.ones_like(rows[once], dtype=torch.int32))
            return
        logits, rows = logits.contiguous(), _labels32(rows, n)                 # (held until the launch is queued)
        _call("apn_ss_votes_add", logits.device, n, C, logits.shape[1], logits.data_ptr(), rows.data_ptr(), self.calls, self.acc.data_ptr(), self.cnt.data_ptr(), self.stamp.data_ptr(),
              self.flags.data_ptr())

    @torch.no_grad()
    def finish(self, labels=None, metrics=None, want_mean=False):
        """-> (pred (n,) int32, mean (n,C) or None).  labels (n,) with metrics (a `SegMetrics`): its counters are added
        to.  Raises ValueError when an `add` saw a repeated row or a row outside [0,n): the scene's one host read."""
        C, n, dev = self.num_classes, self.n, self.acc.device
        if (labels is None) != (metrics is None):
            raise ValueError("Votes.finish: labels and metrics come together")
        if labels is not None and (labels.shape != (n,) or labels.device != dev or metrics.num_classes != C):
            raise ValueError(f"Votes.finish: labels must be ({n},) on {dev}, metrics over {C} classes")
        why = _why_composed(self.acc, C if labels is not None else None, self.fused)
        if why is None and C > MAX_CLASSES:
            why = f"more than {MAX_CLASSES} classes"
        if why is not None:
            _composed(why)
            mean = self.acc / self.cnt.clamp(min=1).unsqueeze(1)
            pred = mean.argmax(dim=1).to(torch.int32)
            if labels is not None:
                count_composed(metrics.counts, pred, labels, C, metrics.ignore_index)
            if not want_mean:
                mean = None
        else:
            pred = torch.empty(n, dtype=torch.int32, device=dev)
            mean = torch.empty(n, C, dtype=torch.float32, device=dev) if want_mean else None
            ign = (0, 0) if metrics is None else metrics._ignore_args()
            labels = None if labels is None else _labels32(labels, max(C, abs(ign[0])))
            _call("apn_ss_votes_finish", dev, n, C, self.acc.data_ptr(), self.cnt.data_ptr(),
                  None if labels is None else labels.data_ptr(), *ign,
                  None if metrics is None else metrics.counts.data_ptr(), None if mean is None else mean.data_ptr(),
                  pred.data_ptr())
        duplicates, rejected = self.flags.tolist()
        if duplicates or rejected:
            raise ValueError(f"Votes: {duplicates} repeated row(s) inside one add, {rejected} row(s) outside [0, {n})")
        return pred, mean


@torch.no_grad()
def project(logits, slot, voxel_of, labels=None, metrics=None, fused=True):
    """The nearest-neighbour mode of `test` (main.py:599-600): `all_logits[reverse_idx_part][voxel_idx][reverse_idx]
    .argmax(1)`.  logits (C,m): one column per voxel; slot (m): the column that holds voxel v's pick; voxel_of (n).
    -> pred (n,) int32, and the counters of `metrics` against labels (n).  A slot or voxel outside [0,m) raises
    ValueError (one host read)."""
    C, m = logits.shape
    n, dev = voxel_of.shape[0], logits.device
    if slot.shape != (m,) or slot.device != dev or voxel_of.device != dev:
        raise ValueError(f"project: slot must be ({m},) and voxel_of (n,) on {dev}")
    if (labels is None) != (metrics is None):
        raise ValueError("project: labels and metrics come together")
    why = _why_composed(logits, C, fused)
    if why is not None:
        _composed(why)
        slot, voxel_of = slot.long(), voxel_of.long()
        bad = int((((slot < 0) | (slot >= m)).sum() + ((voxel_of < 0) | (voxel_of >= m)).sum()).item())
        if bad:
            raise ValueError(f"project: {bad} slot / voxel entries outside [0, {m})")
        pred = logits[:, slot].argmax(dim=0)[voxel_of].to(torch.int32)
        if labels is not None:
            count_composed(metrics.counts, pred, labels, C, metrics.ignore_index)
        return pred
    pred = torch.empty(n, dtype=torch.int32, device=dev)
    pred_voxel = torch.empty(m, dtype=torch.int32, device=dev)
    flags = torch.zeros(2, dtype=torch.int32, device=dev)
    ign = (0, 0) if metrics is None else metrics._ignore_args()
    # (the converted copies are held in locals until the launches are queued: a temporary's memory could be handed out again)
    logits, slot, voxel_of = logits.contiguous(), _labels32(slot, m), _labels32(voxel_of, m)
    labels = None if labels is None else _labels32(labels, max(C, abs(ign[0])))
    _call("apn_ss_project", dev, C, m, n, logits.data_ptr(), slot.data_ptr(), voxel_of.data_ptr(),
          None if labels is None else labels.data_ptr(), *ign, pred_voxel.data_ptr(), None if metrics is None else metrics.counts.data_ptr(), pred.data_ptr(),
          flags.data_ptr())
    bad = flags.tolist()[1]
    if bad:
        raise ValueError(f"project: {bad} slot / voxel entries outside [0, {m})")
    return pred


# ---------------------------------------------------------------------------------------------------------- the crop
def crop_distance(coord, centre):
    """np.sum(np.square(coord - centre), 1) in float32: (dx*dx + dy*dy) + dz*dz, every operation rounded."""
    sq = torch.square(coord - centre)
    return (sq[:, 0] + sq[:, 1]) + sq[:, 2]


@torch.no_grad()
def crop_nearest(coord, sizes, centre, k, fused=True):
    """The k rows nearest to a centre row in each cloud of the stacked layout: `np.argsort(np.sum(np.square(coord -
    coord[init]), 1))[:k]` of crop_pc as a SET (the reference shuffles it afterwards), in ascending row.
    coord (n,3) float32; sizes: the clouds' row counts (host integers, their sum n); centre: a row inside each cloud
    (host integers or a (b,) tensor); -> idx (b,k) int32, global rows.  Ties at the cutoff go to the lower rows, so the
    set is np.argsort(d, kind='stable')[:k].  A cloud with fewer than k rows is a ValueError before any launch (pad
    first, as the reference does); a non-finite coordinate is a ValueError after it (the one host read)."""
    sizes = [int(s) for s in sizes]
    b, n, k = len(sizes), int(coord.shape[0]), int(k)
    if coord.dim() != 2 or coord.shape[1] != 3 or sum(sizes) != n or b < 1:
        raise ValueError("crop_nearest: coord must be (n,3) and sizes the clouds' row counts, summing to n")
    if k < 1 or any(s < k for s in sizes):
        raise ValueError(f"crop_nearest: k = {k} needs 1 <= k <= every cloud's rows (sizes {sizes}): pad first")
    if n >= _MAX_ROWS:
        raise ValueError(f"crop_nearest: {n} rows, the kernel takes fewer than 2^27")
    dev = coord.device
    centre_t = torch.as_tensor(centre, device=dev).reshape(-1)
    if centre_t.shape != (b,) or centre_t.dtype.is_floating_point:
        raise ValueError(f"crop_nearest: centre must be {b} integers")
    ends = np.cumsum(sizes)
    why = _why_composed(coord, None, fused)
    if why is not None:
        _composed(why)
        centres = centre_t.tolist()
        if any(not 0 <= c < s for c, s in zip(centres, sizes)):
            raise ValueError("crop_nearest: a centre lies outside its cloud")
        if not bool(torch.isfinite(coord).all()):
            raise ValueError("crop_nearest: non-finite coordinates")
        out = []
        for end, s, c in zip(ends, sizes, centres):
            cloud = coord[end - s:end]
            order = torch.argsort(crop_distance(cloud, cloud[c]), stable=True)[:k]
            out.append(torch.sort(order).values + (end - s))
        return torch.stack(out).to(torch.int32)
    offset = torch.from_numpy(ends.astype(np.int32)).to(dev)
    idx = torch.empty(b, k, dtype=torch.int32, device=dev)
    stats = torch.zeros(2, dtype=torch.int32, device=dev)
    coord, centre_t = coord.contiguous(), _labels32(centre_t, n)               # (held until the launch is queued)
    _call("apn_ss_crop_nearest", dev, b, n, k, coord.data_ptr(), offset.data_ptr(), centre_t.data_ptr(), idx.data_ptr(),
          stats.data_ptr())
    bad, refused = stats.tolist()
    if bad or refused:
        raise ValueError(f"crop_nearest: {bad} row(s) with a non-finite coordinate, {refused} cloud(s) refused "
                         "(a centre outside its cloud)")
    return idx


# ------------------------------------------------------------------------------------------------- grids on any device
def composed_grid(coord, voxel_size):
    """`voxel_grid.voxel_grid` of one cloud in plain torch (any device): the same fields by the same definitions."""
    vs = torch.tensor(_sizes(voxel_size), dtype=torch.float64, device=coord.device)
    n = coord.shape[0]
    cells = torch.floor(coord.double() / vs).long()
    _, inv = torch.unique(cells, dim=0, return_inverse=True)
    m = int(inv.max().item()) + 1 if n else 0
    rows = torch.arange(n, device=coord.device)
    first = torch.full((m,), n, dtype=torch.int64, device=coord.device).scatter_reduce_(0, inv, rows, 'amin')
    number = torch.empty(m, dtype=torch.int64, device=coord.device)
    number[torch.argsort(first)] = torch.arange(m, device=coord.device)        # voxels numbered by their smallest row
    voxel_of = number[inv]
    count = torch.bincount(voxel_of, minlength=m)
    start = torch.cumsum(count, 0) - count
    idx_sort = torch.argsort(voxel_of, stable=True)
    i32 = lambda t: t.to(torch.int32)
    return VoxelGrid(n, m, int(count.max().item()) if m else 0, i32(voxel_of), i32(count), i32(start), i32(idx_sort),
                     torch.tensor([m], dtype=torch.int32, device=coord.device))


def _grid(coord, voxel_size, fused=True):
    why = _why_composed(coord, None, fused)
    if why is not None:
        _composed(why)
        return composed_grid(coord, voxel_size)
    from .voxel_grid import voxel_grid
    return voxel_grid(coord.contiguous(), voxel_size)


def _features(data, keys):
    """get_features_by_keys (data_util.py:177-182): the keyed (B,n,c) tensors concatenated, channels first."""
    return torch.cat([data[k] for k in keys.split(',')], -1).transpose(1, 2).contiguous()


def _permutation(m, draws, dev):
    if draws is None:
        perm = np.arange(m)
        np.random.shuffle(perm)                       # np.random.shuffle(idx_part): the draws depend on the length alone
        return torch.from_numpy(perm).to(dev)
    if isinstance(draws, str):
        if draws != 'device':
            raise ValueError(f"draws must be None, 'device' or tensors, got {draws!r}")
        return torch.randperm(m, device=dev)
    draws = torch.as_tensor(draws, device=dev).long()
    if draws.shape != (m,):
        raise ValueError(f"a supplied permutation must have {m} entries, got {tuple(draws.shape)}")
    return draws


# ------------------------------------------------------------------------------------------------------ the test loop
class SceneTester:
    """`test` (main.py:507-668) over `load_data` (:64-109) for scenes already on the device.

    tester(coord (n,3), feat (n,cf) or None, label (n,) or None, draws=None) -> the scene's `SegMetrics` (also added
    into `self.total`, as `all_cm.value += cm.value`); `self.pred` (n,) int32 and `self.parts` (the rows of every
    forward) are kept for inspection.  The body: coord -= coord.min(0); grid = voxel_grid(coord, voxel_size); for i in
    range(count_max): rows = grid.part(i) under a row permutation, pos = coord[rows] - its min, heights =
    pos[:, gravity_dim], logits = model({'pos', 'x'}), votes.add(logits[0], rows); then votes.finish.
    draws: None makes the reference's host call (np.random.shuffle per part) so a seeded script consumes the same host
    stream; 'device' draws on the device; a sequence of count_max permutation tensors is used as given.
    mode='nearest_neighbor': ONE forward on a random pick per voxel in a random order, then `project`; draws: None (the
    reference's np.random.randint and np.random.permutation), 'device', or (pick draws (m,), permutation (m,)).
    voxel_size=None: one part, arange(n).  features: the reference's `feature_keys` over 'pos', 'x', 'heights'.
    transform: an optional callable on the part's {'pos','x','heights'} dict ((1,n,c) tensors) before the features are
    assembled (the reference's `pipe_transform`)."""

    def __init__(self, model, num_classes, voxel_size=None, ignore_index=None, features='x,heights', gravity_dim=2,
                 mode='multi_voxel', transform=None, fused=True):
        if mode not in ('multi_voxel', 'nearest_neighbor'):
            raise ValueError(f"SceneTester: unknown mode '{mode}'")
        self.model, self.num_classes, self.voxel_size = model, int(num_classes), voxel_size
        self.ignore_index, self.features, self.gravity_dim = ignore_index, features, gravity_dim
        self.mode, self.transform, self.fused = mode, transform, fused
        self.total = None
        self.pred, self.parts = None, []

    def _forward(self, coord, feat, rows):
        pos = coord[rows.long()]
        pos = pos - pos.min(0).values
        data = {'pos': pos.unsqueeze(0), 'heights': pos[:, self.gravity_dim:self.gravity_dim + 1].unsqueeze(0)}
        if feat is not None:
            data['x'] = feat[rows.long()].unsqueeze(0)
        if self.transform is not None:
            data = self.transform(data)
        return self.model({'pos': data['pos'].contiguous(), 'x': _features(data, self.features)})[0]

    @torch.no_grad()
    def __call__(self, coord, feat=None, label=None, draws=None):
        if not (torch.is_tensor(coord) and coord.dim() == 2 and coord.shape[1] == 3 and coord.shape[0] > 0):
            raise ValueError("SceneTester: coord must be a non-empty (n,3) tensor")
        n, dev, C = coord.shape[0], coord.device, self.num_classes
        cm = SegMetrics(C, self.ignore_index, device=dev, fused=self.fused)
        was = self.model.training
        self.model.eval()
        self.parts = []
        try:
            coord = coord - coord.min(0).values
            lab = None if label is None else label.reshape(-1)
            met = None if label is None else cm
            if self.voxel_size is None:
                rows = torch.arange(n, device=dev)
                self.parts.append(rows)
                votes = Votes(n, C, dev, self.fused)
                votes.add(self._forward(coord, feat, rows), rows)
                self.pred, _ = votes.finish(lab, met)
            elif self.mode == 'nearest_neighbor':
                grid = _grid(coord, self.voxel_size, self.fused)
                if draws is None:
                    pick = torch.from_numpy(np.random.randint(0, max(grid.count_max, 1), grid.m)).to(dev)
                    perm = torch.from_numpy(np.random.permutation(grid.m)).to(dev)
                elif isinstance(draws, str):
                    pick = torch.randint(0, max(grid.count_max, 1), (grid.m,), device=dev)
                    perm = _permutation(grid.m, draws, dev)
                else:
                    pick, perm = draws[0], _permutation(grid.m, draws[1], dev)
                rows = grid.pick(pick)[perm]                       # column j holds voxel perm[j]'s pick
                slot = torch.empty_like(perm)
                slot[perm] = torch.arange(grid.m, device=dev)      # reverse_idx_part
                self.parts.append(rows)
                self.pred = project(self._forward(coord, feat, rows), slot, grid.voxel_of, lab, met, self.fused)
            else:
                grid = _grid(coord, self.voxel_size, self.fused)
                votes = Votes(n, C, dev, self.fused)
                if not (draws is None or isinstance(draws, str)) and len(draws) != grid.count_max:
                    raise ValueError(f"SceneTester: {grid.count_max} parts need as many permutations, got {len(draws)}")
                for i in range(grid.count_max):
                    rows = grid.part(i)
                    rows = rows[_permutation(grid.m, draws if draws is None or isinstance(draws, str) else draws[i], dev)]
                    self.parts.append(rows)
                    votes.add(self._forward(coord, feat, rows), rows)
                self.pred, _ = votes.finish(lab, met)
        finally:
            self.model.train(was)
        if label is not None:
            if self.total is None:
                self.total = SegMetrics(C, self.ignore_index, device=dev, fused=self.fused)
            self.total.add(cm)
        return cm


# -------------------------------------------------------------------------------------------------- the training crop
class SceneSampler:
    """`crop_pc` (data_util.py:146-174) for split='train', variable=False, shuffle=True, with S3DIS's heights
    (s3dis.py:140-141), for scenes already on the device.  Per scene: coord -= coord.min(0); one pick per voxel
    (`voxelize` mode 0); with N voxels, N >= voxel_max draws a centre and keeps the voxel_max nearest picks
    (`crop_nearest`), N < voxel_max pads with `choice` draws; a permutation; coord -= coord.min(0); heights =
    coord[:, gravity_dim].  The crops of a batch are ONE `crop_nearest` launch over the stacked picks.

    draws=None makes the reference's host calls in the reference's order -- np.random.randint(0, count_max, m),
    np.random.randint(N) or np.random.choice(N, voxel_max - N), np.random.permutation(voxel_max) per scene -- so a seeded
    script consumes the same host stream; 'device' draws with torch.randint / torch.randperm on the device; a list with
    one dict per scene {'pick' (m,), 'centre' int, 'pad' (voxel_max - N,), 'perm' (voxel_max,)} is used as given.

    The reference's voxel ORDER is unmatchable (voxel_grid.py), so which row number a pick has differs from the
    reference: the crop is crop_pc's analogue -- the same partition, draws, nearest set, shuffle and shifts -- not its
    twin.  `self.rows` keeps, per scene, the scene rows of the crop in output order."""

    def __init__(self, voxel_size=0.04, voxel_max=24000, gravity_dim=2, features='x,heights', fused=True):
        self.voxel_size, self.voxel_max, self.gravity_dim = voxel_size, int(voxel_max), gravity_dim
        self.features, self.fused = features, fused
        self.rows = []

    def _draws(self, grid, draws, dev):
        m, k = grid.m, self.voxel_max
        if draws is None:
            out = {'pick': torch.from_numpy(np.random.randint(0, max(grid.count_max, 1), m)).to(dev)}
            if m >= k:
                out['centre'] = int(np.random.randint(m))
            else:
                out['pad'] = torch.from_numpy(np.random.choice(m, k - m)).to(dev)
            out['perm'] = torch.from_numpy(np.random.permutation(np.arange(k))).to(dev)
            return out
        if isinstance(draws, str):
            if draws != 'device':
                raise ValueError(f"SceneSampler: draws must be None, 'device' or a list of dicts, got {draws!r}")
            out = {'pick': torch.randint(0, max(grid.count_max, 1), (m,), device=dev), 'perm': torch.randperm(k, device=dev)}
            if m >= k:
                out['centre'] = torch.randint(0, m, (1,), device=dev)
            else:
                out['pad'] = torch.randint(0, m, (k - m,), device=dev)
            return out
        return draws

    @torch.no_grad()
    def batch(self, scenes, draws=None):
        """scenes: a list of (coord (n,3) float32, feat (n,cf), label (n,)) on one device -> {'pos' (B,k,3),
        'x' (B,C,k), 'y' (B,k) int64} for k = voxel_max."""
        if not scenes:
            raise ValueError("SceneSampler.batch: no scenes")
        k, dev = self.voxel_max, scenes[0][0].device
        if not (draws is None or isinstance(draws, str)) and len(draws) != len(scenes):
            raise ValueError("SceneSampler.batch: one dict of draws per scene")
        subs, sizes, centres, kept = [], [], [], []
        for s, (coord, feat, label) in enumerate(scenes):
            coord = coord - coord.min(0).values
            grid = _grid(coord, self.voxel_size, self.fused)
            d = self._draws(grid, draws if draws is None or isinstance(draws, str) else draws[s], dev)
            rows = grid.pick(d['pick']).long()                     # uniq_idx: scene rows, one per voxel
            if grid.m < k:                                         # the non-variable padding: every pick, then repeats
                rows = torch.cat([rows, rows[torch.as_tensor(d['pad'], device=dev).long()]])
                centre = torch.zeros(1, dtype=torch.int64, device=dev)
            else:
                centre = torch.as_tensor(d['centre'], device=dev).reshape(1).long()
            subs.append(coord[rows])
            sizes.append(rows.numel())
            centres.append(centre)
            kept.append((coord, feat, label, rows, torch.as_tensor(d['perm'], device=dev).long()))
        stacked = torch.cat(subs).contiguous()
        idx = crop_nearest(stacked, sizes, torch.cat(centres), k, self.fused).long()
        out = {'pos': [], 'x': [], 'y': []}
        self.rows = []
        start = 0
        for (coord, feat, label, rows, perm), size, crop in zip(kept, sizes, idx):
            if perm.shape != (k,):
                raise ValueError(f"SceneSampler.batch: a permutation must have {k} entries")
            chosen = rows[(crop - start)[perm]]
            start += size
            pos = coord[chosen]
            pos = pos - pos.min(0).values
            data = {'pos': pos.unsqueeze(0), 'heights': pos[:, self.gravity_dim:self.gravity_dim + 1].unsqueeze(0)}
            if feat is not None:
                data['x'] = feat[chosen].unsqueeze(0)
            out['pos'].append(pos)
            out['x'].append(_features(data, self.features)[0])
            out['y'].append(label.reshape(-1)[chosen].long())
            self.rows.append(chosen)
        return {key: torch.stack(v).contiguous() for key, v in out.items()}


__all__ = ["BaseSeg", "SegHead", "SmoothCrossEntropy", "SegMetrics", "get_mious", "count_composed", "SegStep", "validate",
           "Votes", "project", "crop_nearest", "crop_distance", "composed_grid", "SceneTester", "SceneSampler",
           "COMPOSED_CALLS", "MAX_CLASSES", "POINTNEXT_S_ENCODER", "POINTNEXT_S_DECODER", "POINTNEXT_S_HEAD"]
