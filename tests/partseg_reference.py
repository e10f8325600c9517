"""Shared pieces of the part-segmentation tests (test_partseg_cpu.py, test_gpu_part_metrics.py, test_gpu_partseg.py) and
of tests/golden/make_golden_partseg.py: the narrow decoder fixture's inputs regenerated from seeds, and a numpy
statement of the part metric (`get_ins_mious` and `validate`'s totals of the reference's
examples/shapenetpart/train_adapt.py), which the golden generator checks against the reference itself and the GPU tests
use as their checker."""
import numpy as np
import torch

import golden_inputs as GI

# ---------------------------------------------------------------------------------------------- the narrow decoder
CLS_MAPS = ('pointnet2', 'curvenet', 'pointnext', 'pointnext1')
NARROW_B, NARROW_N = 4, 64
NARROW_CHANNELS = [16, 32, 64]                  # three encoder levels: 64, 16 and 4 points
NARROW_LEVELS = (64, 16, 4)
NARROW_IN = 7
SHAPE_CLASSES, PART_LABELS = 16, 50
# one decoder stage with an InvResMLP block behind its propagation block (decoder.0 = [FeaturePropagation, InvResMLP])
BLOCKS_CASE = dict(cls_map='pointnet2', decoder_blocks=[1, 1, 2, 1], radius=0.15, nsample=8)


def decoder_args(cls_map, **over):
    args = dict(encoder_channel_list=list(NARROW_CHANNELS), decoder_layers=2, cls_map=cls_map, num_classes=SHAPE_CLASSES,
                conv_args={'order': 'conv-norm-act'})
    args.update(over)
    return args


def part_embed():
    """cls2partembed: row k has ones at category k's part labels (ShapeNetPart's table)."""
    from adaptpoint_amd.part_metrics import SHAPENETPART_CLS2PARTS
    t = torch.zeros(SHAPE_CLASSES, PART_LABELS)
    for k, parts in enumerate(SHAPENETPART_CLS2PARTS):
        t[k, list(parts)] = 1.0
    return t


def pyramid(seed, fps):
    """The encoder's outputs for the narrow decoder: p (4 levels, the first two the same cloud as after a stride-1 stem),
    f (NARROW_IN, then NARROW_CHANNELS), cls (B,1), and the weights of the scalar the gradients are taken of.
    fps(xyz, m) -> indices: the oracle's sampler."""
    p0 = GI.unit_sphere_cloud(NARROW_B, NARROW_N, seed=9000 + seed)
    p = [p0, p0]
    for m in NARROW_LEVELS[1:]:
        p.append(GI.take_points(p[-1], fps(p[-1], m)))
    chans = [NARROW_IN] + NARROW_CHANNELS
    sizes = (NARROW_N,) + NARROW_LEVELS
    f = [torch.from_numpy(GI.seeded_normal((NARROW_B, c, n), seed=9100 + 10 * seed + i))
         for i, (c, n) in enumerate(zip(chans, sizes))]
    cls = torch.from_numpy(np.random.RandomState(9200 + seed).randint(0, SHAPE_CLASSES, (NARROW_B, 1))).long()
    # a weighted MEAN over the clouds' points, as a loss is: gradients of order 0.1, the scale at which an absolute bar
    # of 1e-5 (tests/test_propagation_cpu.py) sits above float32 summation noise and far below any real difference
    gout = torch.from_numpy(GI.seeded_normal((NARROW_B, NARROW_CHANNELS[0], NARROW_N), seed=9300 + seed)) / (NARROW_B * NARROW_N)
    return [torch.from_numpy(q) for q in p], f, cls, gout


def run_decoder(dec, p, f, cls, gout):
    """One training-mode forward / backward of a decoder (the reference's or the mirror's) -> dict of numpy results."""
    f = [t.detach().clone().requires_grad_(i > 0) for i, t in enumerate(f)]
    out = dec([q.clone() for q in p], list(f), cls.to(p[0].device))
    (out * gout.to(out.dtype)).sum().backward()
    res = {"out": out.detach().cpu().numpy()}
    for n, q in dec.named_parameters():
        res[f"grad/{n}"] = q.grad.detach().cpu().numpy().ravel()[GI.gradient_sample_index(n, q.numel())]
    for n, b in dec.named_buffers():
        res[f"buf/{n}"] = b.detach().cpu().numpy()
    for i in (1, 2, 3):
        res[f"gin/{i}"] = f[i].grad.detach().cpu().numpy()
    return res


def rel(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.linalg.norm(a - ref) / max(np.linalg.norm(ref), 1e-30))


def loss_inputs(seed, B=3, C=7, N=11):
    g = torch.Generator().manual_seed(9400 + seed)
    logits = 2.0 * torch.randn(B, C, N, generator=g)
    labels = torch.randint(0, C, (B, N), generator=g)
    counts = torch.randint(1, 1000, (C,), generator=g).numpy()
    return logits, labels, counts


# ------------------------------------------------------------------------------------------------------ the metric
def predict(logits):
    """`logits.max(dim=1)[1]`: the first channel of the maximum; a NaN beats every number and the first NaN wins
    (numpy's argmax has the same two rules)."""
    return np.argmax(np.asarray(logits), axis=1)


def shape_ious(pred, target, cls, cls2parts):
    """get_ins_mious (train_adapt.py:77-107): per shape, the mean over its category's parts, in list order, of
    float32(100 I) / float32(U) (100 where U == 0), summed left to right in float32."""
    pred, target = np.asarray(pred), np.asarray(target)
    out = np.empty(pred.shape[0], np.float32)
    for b in range(pred.shape[0]):
        parts = cls2parts[int(np.asarray(cls).reshape(-1)[b])]
        s = np.float32(0.0)
        for part in parts:
            pp, tp = pred[b] == part, target[b] == part
            i, u = int(np.logical_and(pp, tp).sum()), int(np.logical_or(pp, tp).sum())
            iou = np.float32(100.0) if u == 0 else np.float32(100 * i) / np.float32(u)
            s = np.float32(s + iou)
        out[b] = s / np.float32(len(parts))
    return out


def totals(ious, cls, num_classes, state=None):
    """validate :576-582 as the device accumulates it: every counted shape (iou >= 0) added in ascending order --
    cls_sum float32, ins_sum float64.  state: the totals so far (for a pass fed in batches)."""
    cls_sum, cls_num, ins_sum, ins_num = state or (np.zeros(num_classes, np.float32), np.zeros(num_classes, np.int32),
                                                   np.float64(0.0), 0)
    cls_sum, cls_num = cls_sum.copy(), cls_num.copy()
    for v, k in zip(np.asarray(ious, np.float32), np.asarray(cls).reshape(-1)):
        if v >= 0:
            cls_sum[k] = np.float32(cls_sum[k] + v)
            cls_num[k] += 1
            ins_sum = np.float64(ins_sum + np.float64(v))
            ins_num += 1
    return cls_sum, cls_num, ins_sum, ins_num


def _shapenet():
    from adaptpoint_amd.part_metrics import SHAPENETPART_CLS2PARTS
    return [list(p) for p in SHAPENETPART_CLS2PARTS]


def crafted_cases():
    """(name, pred (B,N), target (B,N), cls (B,), cls2parts, num_parts): the corner cases of the metric."""
    sn = _shapenet()
    N = 12
    cases = []
    # a part absent from prediction and target (IoU 100): category 0 has parts 0..3, only 0 and 1 occur
    t = np.array([[0] * 6 + [1] * 6])
    p = np.array([[0] * 5 + [1] * 7])
    cases.append(("absent_part", p, t, np.array([0]), sn, 50))
    # a predicted label outside the category: counts for no part, but leaves the target's part with a larger union
    t = np.array([[4] * 6 + [5] * 6])
    p = np.array([[4] * 3 + [30] * 3 + [5] * 4 + [49] * 2])
    cases.append(("outside_label", p, t, np.array([1]), sn, 50))
    # everything wrong
    t = np.array([[6] * N, [8] * 4 + [9] * 4 + [10] * 2 + [11] * 2])
    p = np.array([[7] * N, [9] * 4 + [10] * 4 + [11] * 2 + [8] * 2])
    cases.append(("all_wrong", p, t, np.array([2, 3]), sn, 50))
    # a category with a non-contiguous part list (in an order that is not ascending), and one that never occurs
    table = [[5, 0, 9], [2, 3], [7], [1, 4, 6, 8]]
    t = np.array([[5] * 4 + [0] * 4 + [9] * 4, [2] * 6 + [3] * 6, [1] * 3 + [4] * 3 + [6] * 3 + [8] * 3])
    p = np.array([[5] * 3 + [0] * 5 + [9] * 2 + [2] * 2, [2] * 7 + [3] * 5, [1] * 3 + [4] * 2 + [6] * 4 + [8] * 2 + [7]])
    cases.append(("noncontiguous_and_missing_category", p, t, np.array([0, 1, 3]), table, 10))
    return cases


def random_case(B, N, C, seed, ties=True):
    """Random logits (B,C,N) with exact ties (values on a coarse grid), targets and classes over a table of S = 5
    categories that partition a shuffled [0, C) into non-contiguous lists."""
    rng = np.random.RandomState(seed)
    perm = rng.permutation(C)
    cuts = np.sort(rng.choice(np.arange(1, C), 4, replace=False))
    table = [list(map(int, part)) for part in np.split(perm, cuts)]
    logits = rng.randn(B, C, N).astype(np.float32)
    if ties:
        logits = np.round(logits * 2) / 2
    cls = rng.randint(0, len(table), B)
    target = np.stack([rng.choice(table[k], N) for k in cls]).astype(np.int64)
    # make the prediction right about half of the time, so that intersections are not all small
    hit = rng.rand(B, N) < 0.5
    b, n = np.nonzero(hit)
    logits[b, target[b, n], n] += 4.0
    return logits.astype(np.float32), target, cls.astype(np.int64), table
