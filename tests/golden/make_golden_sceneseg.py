"""Regenerates tests/golden/sceneseg_golden.npz (run in the BUILD container only):

    python tests/golden/make_golden_sceneseg.py

The reference's own `BaseSeg` / `SegHead` (openpoints/models/segmentation/base_seg.py), `PointNextDecoder`
(openpoints/models/backbone/pointnext.py:459-496), `SmoothCrossEntropy` (openpoints/loss/build.py:12-63) and
`ConfusionMatrix` / `get_mious` (openpoints/utils/metrics.py:51-176), imported in memory through make_golden's stubs
(nothing copied), run on CPU with name-seeded weights; interpolation runs on the oracle.  Inputs are regenerated from
seeds by tests/scene_seg_reference.py and not stored.

  sd/names, sd/shapes   the state_dict of the reference's BaseSeg for PointNeXt-S on S3DIS (13 classes)
  dh/<head>/...         PointNextDecoder + SegHead on partseg_reference.pyramid's narrow levels in training mode, for
                        the plain head and the head with global_feat='max,avg': output, every parameter's gradient, the
                        gradients of the three feature levels, the BatchNorm buffers after the step
  loss/<ignore>/...     SmoothCrossEntropy(ignore_index=...) with and without label smoothing: value, logit gradient
  m/<case>/...          ConfusionMatrix.update on seeded predictions with and without ignore_index: value, all_metrics,
                        all_acc, get_mious(tp, union, count)

It also asserts that the numpy statements of tests/scene_seg_reference.py equal the reference where the reference is
defined: the confusion counters against `ConfusionMatrix.value`, and the crop against crop_pc's own expression
`np.argsort(np.sum(np.square(coord - coord[init_idx]), 1))[:voxel_max]` as a set where no two rows tie at the cutoff.
The vote merge's reference is torch_scatter, which is not installed: its statement (fp32 adds in call order, one
division) stands on its own, and on exactly representable logits equals the float64 mean.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402
import make_golden_partseg as MGP  # noqa: E402
import partseg_reference as PR  # noqa: E402
import scene_seg_reference as R  # noqa: E402
from oracle import oracle as O  # noqa: E402

OUT = os.path.join(HERE, "sceneseg_golden.npz")


def state_dict_case():
    MGP.import_reference()
    import openpoints.models.segmentation.base_seg as ref_seg
    from easydict import EasyDict
    from adaptpoint_amd.sceneseg import POINTNEXT_S_DECODER, POINTNEXT_S_ENCODER, POINTNEXT_S_HEAD
    enc = EasyDict(NAME='PointNextEncoder', **{k: (list(v) if isinstance(v, tuple) else v)
                                               for k, v in POINTNEXT_S_ENCODER.items()})
    model = ref_seg.BaseSeg(encoder_args=enc, decoder_args=EasyDict(NAME='PointNextDecoder', **POINTNEXT_S_DECODER),
                            cls_args=EasyDict(NAME='SegHead', **POINTNEXT_S_HEAD))
    sd = model.state_dict()
    return {"sd/names": np.array(list(sd.keys())),
            "sd/shapes": np.array([",".join(str(s) for s in t.shape) for t in sd.values()])}


def decoder_head_cases():
    from adaptpoint_amd.pointnext import fill_parameters_by_name
    ref_pn = MGP.import_reference()
    import openpoints.models.segmentation.base_seg as ref_seg
    seed = int(np.load(os.path.join(HERE, "partseg_golden.npz"))["dec/seed"])       # the index-robust seed found there
    out = {"dh/seed": np.int64(seed)}
    for tag, head_args in R.HEAD_CASES.items():
        p, f, gout = R.seg_pyramid(seed, O.furthest_point_sampling)
        dec = fill_parameters_by_name(ref_pn.PointNextDecoder(encoder_channel_list=list(R.NARROW_CHANNELS),
                                                              in_channels=R.NARROW_IN)).train()
        head = fill_parameters_by_name(ref_seg.SegHead(in_channels=dec.out_channels, **head_args)).train()
        res = R.run_decoder_head(dec, head, p, f, gout)
        out.update({f"dh/{tag}/{k}": v for k, v in res.items()})
    return out


def loss_cases():
    MGP.import_reference()
    import openpoints.loss.build as ref_loss
    out = {}
    keep = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self             # (the constructor moves its remap list to a GPU)
    try:
        for ignore in R.LOSS_IGNORES:
            logits, labels, _ = R.loss_inputs(0, ignore)
            C = logits.shape[1]
            for tag, smoothing in (("smooth", 0.2), ("ce", 0.0)):
                crit = ref_loss.SmoothCrossEntropy(label_smoothing=smoothing, ignore_index=ignore, num_classes=C)
                x = logits.clone().requires_grad_(True)
                v = crit(x, labels.clone())
                v.backward()
                out[f"loss/{ignore}/{tag}/value"] = v.detach().numpy()
                out[f"loss/{ignore}/{tag}/grad"] = x.grad.numpy()
            out[f"loss/{ignore}/reducing_list"] = crit.reducing_list.numpy()
    finally:
        torch.Tensor.cuda = keep
    return out


def metric_cases():
    MGP.import_reference()
    import openpoints.utils.metrics as ref_metrics
    out = {}
    for index, (name, C, n, ignore) in enumerate(R.METRIC_CASES):
        seeds = [10 * index, 10 * index + 1]
        cm = ref_metrics.ConfusionMatrix(num_classes=C, ignore_index=ignore)
        halves = []
        for seed in seeds:                                         # two accumulated updates
            pred, true = R.metric_inputs(seed, C, n, ignore)
            halves.append((pred, true))
            cm.update(torch.from_numpy(pred.copy()), torch.from_numpy(true.copy()))
        mine = sum(R.count(p, t, C, ignore) for p, t in halves)
        assert mine[-1] == 0 and np.array_equal(mine[:-1].reshape(C, C), cm.value.numpy()), name
        out[f"m/{name}/seeds"] = np.array(seeds)
        miou, macc, oa, ious, accs = cm.all_metrics()
        out[f"m/{name}/value"] = cm.value.numpy()
        out[f"m/{name}/all_metrics"] = np.array([miou, macc, oa], np.float64)
        out[f"m/{name}/ious"], out[f"m/{name}/accs"] = ious, accs
        macc2, oa2, accs2 = cm.all_acc()
        out[f"m/{name}/all_acc"] = np.array([macc2, oa2], np.float64)
        miou3, macc3, oa3, ious3, accs3 = ref_metrics.get_mious(cm.tp, cm.union, cm.count)
        out[f"m/{name}/get_mious"] = np.array([miou3, macc3, oa3], np.float64)
        out[f"m/{name}/get_mious_ious"], out[f"m/{name}/get_mious_accs"] = ious3, accs3
        out[f"m/{name}/overall_accuray"] = np.float64(cm.overall_accuray.item())
    return out


def check_crop_statement():
    for seed, (n, k) in enumerate(((1000, 24), (5000, 999), (64, 63))):
        coord = R.uniform_cloud(n, 50 + seed)
        init_idx = n // 3
        d = np.sum(np.square(coord - coord[init_idx]), 1)
        crop_idx = np.argsort(d)[:k]                               # crop_pc :159-160
        srt = np.sort(d)
        if k < n and srt[k - 1] == srt[k]:
            continue                                               # a tie at the cutoff: the reference's set is not defined
        assert np.array_equal(np.sort(crop_idx), R.crop(coord, [n], [init_idx], k)[0]), (n, k)
    print("crop statement equals crop_pc's expression as a set")


def check_votes_statement():
    for seed, (n, C, parts) in enumerate(((65, 13, 5), (1000, 2, 3))):
        case = R.votes_case(n, C, parts, 70 + seed, exact=True)
        res = R.votes(n, C, case)
        acc, cnt = np.zeros((n, C), np.float64), np.zeros(n)
        for logits, rows in case:
            np.add.at(acc, rows, logits.T.astype(np.float64))
            np.add.at(cnt, rows, 1)
        assert np.array_equal(res["mean"], (acc / cnt[:, None]).astype(np.float32)) and np.array_equal(res["cnt"], cnt)
    print("votes statement equals the float64 mean on exactly representable logits")


def main():
    check_crop_statement()
    check_votes_statement()
    out = {}
    out.update(metric_cases())
    out.update(loss_cases())
    out.update(decoder_head_cases())
    out.update(state_dict_case())
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes, {len(out)} arrays)")


if __name__ == "__main__":
    main()
