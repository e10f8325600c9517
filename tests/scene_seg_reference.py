"""Shared pieces of the scene-segmentation tests (test_sceneseg_cpu.py, test_gpu_scene_seg.py) and of
tests/golden/make_golden_sceneseg.py: numpy statements of the four contracts of csrc/scene_seg.hip -- the channel-major
confusion matrix, the streamed vote merge ("fp32 adds in call order, one division"), the nearest-neighbour projection and
the nearest-k crop (numpy's float32 distance plus a stable argsort) -- and the seeded inputs of the tests."""
import numpy as np
import torch

import golden_inputs as GI
import partseg_reference as PR

NUM_CLASSES = 13
NARROW_IN = PR.NARROW_IN
NARROW_CHANNELS = PR.NARROW_CHANNELS
HEAD_CASES = {"plain": dict(num_classes=NUM_CLASSES, dropout=0.0, norm_args={'norm': 'bn'}),
              "global": dict(num_classes=NUM_CLASSES, dropout=0.0, norm_args={'norm': 'bn'}, global_feat='max,avg')}


# ----------------------------------------------------------------------------------------------------- the confusion
def predict(logits, axis=1):
    """`logits.argmax(dim)`: the first channel of the maximum; a NaN beats every number and the first NaN wins (numpy's
    argmax has the same two rules)."""
    return np.argmax(np.asarray(logits), axis=axis)


def count(pred, target, num_classes, ignore_index=None):
    """counts (C*C + 1,) int64: cell t*C + p; a target equal to ignore_index is skipped, any other target outside [0,C)
    adds to the last cell.  A prediction below 0 (a rejected point of the projection) is skipped."""
    C = num_classes
    pred, target = np.asarray(pred).reshape(-1).astype(np.int64), np.asarray(target).reshape(-1).astype(np.int64)
    keep = pred >= 0
    if ignore_index is not None:
        keep &= target != ignore_index
    pred, target = pred[keep], target[keep]
    inside = (target >= 0) & (target < C)
    cell = np.where(inside, target * C + pred, C * C)
    return np.bincount(cell, minlength=C * C + 1).astype(np.int64)


def confusion(logits, target, ignore_index=None, valid=None):
    """-> (counts, pred (B,N)) of logits (B,C,N) and target (B,N); only clouds below `valid` count."""
    logits, target = np.asarray(logits), np.asarray(target)
    B, C, N = logits.shape
    pred = predict(logits, 1)
    nv = B if valid is None else min(max(int(valid), 0), B)
    return count(pred[:nv], target[:nv], C, ignore_index), pred


def confusion_case(B, C, N, seed, ignore_index=None):
    """Logits on a coarse grid (ties between channels) with NaN and +-inf sprinkled in, about half the points predicted
    right; int64 targets with a few out-of-range labels (-1, C, C + 5, a large one) and a few ignored ones."""
    rng = np.random.RandomState(seed)
    logits = (np.round(rng.randn(B, C, N) * 2) / 2).astype(np.float32)
    target = rng.randint(0, C, (B, N)).astype(np.int64)
    b, n = np.nonzero(rng.rand(B, N) < 0.5)
    logits[b, target[b, n], n] += 4.0
    special = [np.nan, np.inf, -np.inf]
    for v in special:
        k = max(1, (B * C * N) // 40)
        logits.reshape(-1)[rng.choice(B * C * N, k, replace=False)] = v
    if N >= 2:
        logits[0, :, 0] = -np.inf                                     # an all -inf column: channel 0
        logits[0, :, 1] = np.nan                                      # an all-NaN column: channel 0
    flat = target.reshape(-1)
    pick = rng.choice(B * N, max(1, (B * N) // 10), replace=False)
    odd = [-1, C, C + 5, 2 ** 20] + ([ignore_index] if ignore_index is not None else [])
    flat[pick] = rng.choice(odd, pick.size)
    return logits, target


# --------------------------------------------------------------------------------------------------- the vote merge
def votes(n, num_classes, parts):
    """parts: [(logits (C,n_part) float32, rows (n_part,))] in call order.  acc[row, :] += logits[:, j] as a sequence of
    float32 adds in call order; a row outside [0,n) is rejected; a row that occurs again inside ONE call is a duplicate
    and only one of its occurrences is added (which one is not defined: `unsure` marks those rows).
    -> dict(mean (n,C) float32 = acc / max(cnt, 1), pred, cnt, duplicates, rejected, unsure (n,) bool)."""
    acc = np.zeros((n, num_classes), np.float32)
    cnt = np.zeros(n, np.int64)
    unsure = np.zeros(n, bool)
    duplicates = rejected = 0
    for logits, rows in parts:
        logits, seen = np.asarray(logits, np.float32), set()
        for j, r in enumerate(np.asarray(rows).reshape(-1).tolist()):
            if r < 0 or r >= n:
                rejected += 1
            elif r in seen:
                duplicates += 1
                unsure[r] = True
            else:
                seen.add(r)
                acc[r] = acc[r] + logits[:, j]                          # float32 + float32, rounded once per add
                cnt[r] += 1
    mean = acc / np.maximum(cnt, 1).astype(np.float32)[:, None]
    return dict(mean=mean, pred=predict(mean, 1), cnt=cnt, duplicates=duplicates, rejected=rejected, unsure=unsure)


def votes_case(n, C, nparts, seed, exact):
    """1-5 parts of unequal length over n points, every point seen at least once (part 0 covers the points no later part
    draws).  exact: logits that are multiples of 1/8 below 2^10 -- every sum of at most five of them is exact in float32,
    so the result does not depend on the order; otherwise seeded normal logits."""
    rng = np.random.RandomState(seed)
    parts, seen = [], np.zeros(n, bool)
    for i in range(nparts):
        size = n if nparts == 1 else rng.randint(1, n + 1)
        rows = rng.permutation(n)[:size]
        if i == nparts - 1:
            rows = np.unique(np.concatenate([rows, np.nonzero(~seen)[0]]))
            rows = rows[rng.permutation(rows.size)]
        seen[rows] = True
        if exact:
            logits = rng.randint(-8 * 1000, 8 * 1000, (C, rows.size)).astype(np.float32) / 8.0
        else:
            logits = rng.randn(C, rows.size).astype(np.float32)
        parts.append((logits, rows.astype(np.int64)))
    order = rng.permutation(nparts)
    return [parts[i] for i in order]


# --------------------------------------------------------------------------------------------------- the projection
def project(logits, slot, voxel_of):
    """pred[i] = argmax(logits[:, slot[voxel_of[i]]]); -1 where the voxel or its slot lies outside [0,m).
    -> (pred (n,), rejected: such slots plus such voxel_of entries)."""
    logits, slot, voxel_of = np.asarray(logits), np.asarray(slot).astype(np.int64), np.asarray(voxel_of).astype(np.int64)
    m = logits.shape[1]
    slot_ok = (slot >= 0) & (slot < m)
    pred_voxel = np.where(slot_ok, predict(logits[:, np.where(slot_ok, slot, 0)], 0), -1)
    vox_ok = (voxel_of >= 0) & (voxel_of < m)
    pred = np.where(vox_ok, pred_voxel[np.where(vox_ok, voxel_of, 0)], -1)
    return pred, int((~slot_ok).sum() + (~vox_ok).sum())


# ---------------------------------------------------------------------------------------------------------- the crop
def crop_distance(coord, centre_row):
    """crop_pc's `np.sum(np.square(coord - coord[init_idx]), 1)` on float32 rows."""
    coord = np.asarray(coord, np.float32)
    return np.sum(np.square(coord - coord[centre_row]), 1)


def crop(coord, sizes, centres, k):
    """Per cloud of the stacked layout: np.sort(np.argsort(d, kind='stable')[:k]) as global rows -> (b,k) int64."""
    out, start = [], 0
    for size, c in zip(sizes, centres):
        d = crop_distance(coord[start:start + size], int(c))
        out.append(np.sort(np.argsort(d, kind='stable')[:k]) + start)
        start += size
    return np.stack(out)


def uniform_cloud(n, seed):
    return np.random.RandomState(seed).rand(n, 3).astype(np.float32) * np.float32(4.0)


def lattice_cloud(n, seed):
    """Points of a small integer lattice, many of them repeated: whole shells of rows tie at any cutoff."""
    return np.random.RandomState(seed).randint(0, 4, (n, 3)).astype(np.float32)


# ------------------------------------------------------------------------------------------------------- the scene
def scene(n, seed, num_classes=NUM_CLASSES):
    """A seeded room-like scene: coord (n,3) float32 in a 2 x 2 x 1 box, colours (n,3) in [0,1], labels (n,)."""
    rng = np.random.RandomState(seed)
    coord = (rng.rand(n, 3) * np.array([2.0, 2.0, 1.0])).astype(np.float32) + np.float32(3.0)
    feat = rng.rand(n, 3).astype(np.float32)
    label = rng.randint(0, num_classes, n).astype(np.int64)
    return coord, feat, label


# ------------------------------------------------------------------------------------------- the narrow decoder + head
def seg_pyramid(seed, fps):
    """partseg_reference.pyramid's levels without the class label, and the weights of the scalar whose gradients are
    taken: a weighted mean over the logits (B, NUM_CLASSES, N)."""
    p, f, _, _ = PR.pyramid(seed, fps)
    gout = torch.from_numpy(GI.seeded_normal((PR.NARROW_B, NUM_CLASSES, PR.NARROW_N), seed=9700 + seed)) / (PR.NARROW_B * PR.NARROW_N)
    return p, f, gout


def run_decoder_head(dec, head, p, f, gout):
    """One training-mode forward / backward of decoder + head (the reference's or the mirror's) -> dict of numpy results."""
    f = [t.detach().clone().requires_grad_(i > 0) for i, t in enumerate(f)]
    out = head(dec([q.clone() for q in p], list(f)).squeeze(-1))
    (out * gout.to(out.dtype)).sum().backward()
    res = {"out": out.detach().cpu().numpy()}
    for tag, mod in (("decoder", dec), ("head", head)):
        for n, q in mod.named_parameters():
            res[f"grad/{tag}.{n}"] = q.grad.detach().cpu().numpy().ravel()[GI.gradient_sample_index(n, q.numel())]
        for n, b in mod.named_buffers():
            res[f"buf/{tag}.{n}"] = b.detach().cpu().numpy()
    for i in (1, 2, 3):
        res[f"gin/{i}"] = f[i].grad.detach().cpu().numpy()
    return res


def loss_inputs(seed, ignore_index, B=3, C=7, N=11):
    logits, labels, counts = PR.loss_inputs(seed, B, C, N)
    g = torch.Generator().manual_seed(9800 + seed)
    labels = labels.clone()
    labels[torch.rand(B, N, generator=g) < 0.25] = ignore_index
    return logits, labels, counts


LOSS_IGNORES = (255, 7, -100)          # above the classes, the class count itself, below zero (C = 7)


def metric_inputs(seed, C, n, ignore_index=None):
    rng = np.random.RandomState(9900 + seed)
    true = rng.randint(0, C, n).astype(np.int64)
    pred = np.where(rng.rand(n) < 0.6, true, rng.randint(0, C, n)).astype(np.int64)
    true[rng.randint(0, C, n) == 0] = C - 1 if C > 2 else 0            # an uneven class distribution
    if C > 3:
        pred[pred == 2], true[true == 2] = 1, 1                        # a class that never occurs: 0 / clamp(0, 1)
    if ignore_index is not None:
        true[rng.rand(n) < 0.2] = ignore_index
    return pred, true


METRIC_CASES = (("c13", 13, 4000, None), ("c13_ignore255", 13, 4000, 255), ("c13_ignore13", 13, 4000, 13),
                ("c13_ignore_neg", 13, 4000, -100), ("c2", 2, 77, None), ("c20_ignore", 20, 999, 255))
