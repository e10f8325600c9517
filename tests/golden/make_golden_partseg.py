"""Regenerates tests/golden/partseg_golden.npz (run in the BUILD container only):

    python tests/golden/make_golden_partseg.py

The reference's own `PointNextPartDecoder` (openpoints/models/backbone/pointnext.py:500-663), `BasePartSeg` / `SegHead`
(openpoints/models/segmentation/base_seg.py), `Poly1FocalLoss` / `SmoothCrossEntropy` (openpoints/loss/build.py),
`get_class_weights` (openpoints/dataset/data_util.py) and `get_ins_mious` (examples/shapenetpart/train_adapt.py:77-107),
imported in memory through make_golden's stubs (nothing copied), run on CPU with name-seeded weights
(`fill_parameters_by_name`); interpolation and grouping run on the oracle.  Inputs are regenerated from seeds by
tests/partseg_reference.py and not stored.

  dec/<cls_map>/...   the narrow decoder (channels 16 / 32 / 64 on 64 / 16 / 4 points, B = 4) in training mode for each of
                      the four cls_maps: output, every parameter's gradient, the gradients of the three feature levels,
                      the BatchNorm buffers after the step; err64 = the reference's own distance to its float64 run
                      (output, worst parameter gradient)
  dec/blocks/...      the same with an InvResMLP block behind the last propagation block (partseg_reference.BLOCKS_CASE)
  dec/seed            the input seed: the first of 8 at which no rounding variant of the oracle changes a three_nn or
                      ball-query index and every point's third and fourth nearest coarse points differ by more than 1e-4
                      relative
  sd/names, sd/shapes the state_dict of the default BasePartSeg configuration (PointNeXt-S, cls_map 'curvenet')
  loss/...            Poly1FocalLoss and SmoothCrossEntropy (plain, and with get_class_weights' weights) on (B,C,N)
                      logits: values and logit gradients
  m/<case>/ious       get_ins_mious on partseg_reference's crafted cases and on random ones
  m/<set>/...         validate's totals (:576-592 restated statement for statement on the CPU: `validate` itself moves
                      its tensors to a GPU) over the crafted cases that share ShapeNetPart's table
  m/mean_diff         the largest difference between partseg_reference.shape_ious (left-to-right float32 sum / count) and
                      the reference's torch.mean(torch.stack(...)), over every case; m/mean_err64 the reference's own
                      largest distance to the float64 mean
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402
import partseg_reference as R  # noqa: E402
from oracle import oracle as O  # noqa: E402

OUT = os.path.join(HERE, "partseg_golden.npz")
SCRIPT = os.path.join(MG.REF, "examples", "shapenetpart", "train_adapt.py")


def import_reference():
    _, ref_pn, _ = MG.import_reference()
    import openpoints.models.layers.upsampling as ref_up
    ref_up.three_nn = MG._OracleOps.three_nn
    ref_up.three_interpolate = MG._OracleOps._Interp.apply
    ref_pn.three_interpolation = ref_up.three_interpolation
    return ref_pn


class _Stub(types.ModuleType):
    """A module whose every attribute exists: stands in for the example script's imports that get_ins_mious never uses."""

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return _Stub(name)

    def __call__(self, *a, **k):
        return self


def import_example_script():
    """examples/shapenetpart/train_adapt.py as an in-memory module, every import of it but torch / numpy / the standard
    library stubbed for the duration of the import."""
    names = ["yaml", "wandb", "tqdm", "torch_scatter", "sklearn", "sklearn.metrics", "h5py", "openpoints",
             "openpoints.models", "openpoints.models.layers", "openpoints.loss", "openpoints.scheduler", "openpoints.optim",
             "openpoints.dataset", "openpoints.transforms", "openpoints.utils", "openpoints.models_adaptpoint",
             "openpoints.function_adaptpoint", "openpoints.online_aug", "openpoints.online_aug.pointwolf",
             "openpoints.dataset.shapenetpart_c", "openpoints.dataset.shapenetpart_c.shapenetpart_c",
             "torch.utils.tensorboard"]
    saved = {n: sys.modules.get(n) for n in names}
    path, bench = list(sys.path), torch.backends.cudnn.benchmark
    try:
        for n in names:
            sys.modules[n] = _Stub(n)
        sys.modules["torch.utils.tensorboard"].SummaryWriter = object
        spec = importlib.util.spec_from_file_location("_ref_shapenetpart_train_adapt", SCRIPT)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for n, m in saved.items():
            if m is None:
                sys.modules.pop(n, None)
            else:
                sys.modules[n] = m
        sys.path[:] = path
        torch.backends.cudnn.benchmark = bench
    return mod


# ------------------------------------------------------------------------------------------------------ the decoder
def reference_decoder(ref_pn, cls_map, **over):
    from adaptpoint_amd.pointnext import fill_parameters_by_name
    from easydict import EasyDict
    args = R.decoder_args(cls_map, **over)
    dec = ref_pn.PointNextPartDecoder(group_args=EasyDict(NAME='ballquery'), act_args={'act': 'relu'},
                                      cls2partembed=R.part_embed() if 'pointnext' in cls_map else None, **args)
    return fill_parameters_by_name(dec).train()


def _interp64(unknown, known, feat):
    """three_interpolation in torch at the tensors' precision (the float64 run of the reference)."""
    d, idx = torch.cdist(unknown, known).topk(3, dim=2, largest=False)
    w = 1.0 / (d + 1e-8)
    w = w / w.sum(2, keepdim=True)
    B, C, _ = feat.shape
    n = unknown.shape[1]
    return sum(torch.gather(feat, 2, idx[:, :, j].unsqueeze(1).expand(B, C, n)) * w[:, :, j].unsqueeze(1) for j in range(3))


def index_is_robust(p):
    """No rounding variant changes a three_nn index of either level (or a ball of the blocks case), and the third and
    fourth nearest coarse points of every point differ by more than 1e-4 relative."""
    p = [q.numpy() for q in p]
    try:
        for fine, coarse in ((p[1], p[2]), (p[2], p[3])):
            MG.all_variants_equal(lambda v: O.three_nn(fine, coarse, v)[1])
            d = np.sort(np.linalg.norm(fine[:, :, None].astype(np.float64) - coarse[:, None].astype(np.float64), axis=-1), -1)
            if not ((d[..., 3] - d[..., 2]) > 1e-4 * d[..., 3]).all():
                return False
        radius = 0.15 * 2 ** 3                       # BLOCKS_CASE: the InvResMLP of decoder.0, _to_full_list's value
        MG.all_variants_equal(lambda v: O.ball_query(radius, R.BLOCKS_CASE['nsample'], p[1], p[1], v))
    except SystemExit:
        return False
    return True


def decoder_case(ref_pn, tag, seed, cls_map, **over):
    p, f, cls, gout = R.pyramid(seed, O.furthest_point_sampling)
    dec = reference_decoder(ref_pn, cls_map, **over)
    res = R.run_decoder(dec, p, f, cls, gout)
    out = {f"dec/{tag}/{k}": v for k, v in res.items()}
    if not over:                                      # (the grouped block's float64 run would need a float64 grouper)
        dec64 = reference_decoder(ref_pn, cls_map).double()
        if dec64.cls_map in ('pointnext', 'pointnext1'):
            dec64.cls2partembed = dec64.cls2partembed.double()
        keep = ref_pn.three_interpolation
        ref_pn.three_interpolation = _interp64
        torch.set_default_dtype(torch.float64)        # (the decoder's one-hot is made by a bare torch.zeros)
        try:
            r64 = R.run_decoder(dec64, [q.double() for q in p], [t.double() for t in f], cls, gout)
        finally:
            ref_pn.three_interpolation = keep
            torch.set_default_dtype(torch.float32)
        # a gradient that is zero in exact arithmetic (global_conv1's bias where every cloud's maximum is an active
        # ReLU: a per-channel shift, which the BatchNorm behind the first convolution removes in training mode) has no
        # relative error: left out here, compared by absolute error in the tests
        grads = [k for k in res if k.startswith("grad/")]
        null = [k for k in grads if np.abs(r64[k]).max() < 1e-9]
        errs = [R.rel(res["out"], r64["out"]), max(R.rel(res[k], r64[k]) for k in grads if k not in null)]
        if null:
            print(f"{tag}: zero in float64:", [(k, float(np.abs(res[k]).max())) for k in null])
        print(f"{tag}: reference fp32 against float64: out {errs[0]:.2e}, worst parameter gradient {errs[1]:.2e}")
        out[f"dec/{tag}/err64"] = np.array(errs)
    return out


def decoder_cases():
    ref_pn = import_reference()
    seed = next(s for s in range(8) if index_is_robust(R.pyramid(s, O.furthest_point_sampling)[0]))
    print("decoder goldens: seed", seed)
    out = {"dec/seed": np.int64(seed)}
    for cls_map in R.CLS_MAPS:
        out.update(decoder_case(ref_pn, cls_map, seed, cls_map))
    over = {k: v for k, v in R.BLOCKS_CASE.items() if k != 'cls_map'}
    out.update(decoder_case(ref_pn, "blocks", seed, R.BLOCKS_CASE['cls_map'], **over))
    return out


def state_dict_case():
    import_reference()
    import openpoints.models.segmentation.base_seg as ref_seg
    from easydict import EasyDict
    from adaptpoint_amd.partseg import POINTNEXT_S_DECODER, POINTNEXT_S_ENCODER, POINTNEXT_S_HEAD
    enc = EasyDict(NAME='PointNextEncoder', **{k: (list(v) if isinstance(v, tuple) else v)
                                               for k, v in POINTNEXT_S_ENCODER.items()})
    model = ref_seg.BasePartSeg(encoder_args=enc, decoder_args=EasyDict(NAME='PointNextPartDecoder', **POINTNEXT_S_DECODER),
                                cls_args=EasyDict(NAME='SegHead', **POINTNEXT_S_HEAD))
    sd = model.state_dict()
    return {"sd/names": np.array(list(sd.keys())),
            "sd/shapes": np.array([",".join(str(s) for s in t.shape) for t in sd.values()])}


# ------------------------------------------------------------------------------------------------------- the losses
def loss_cases():
    import_reference()
    import openpoints.loss.build as ref_loss
    # (by its path: the package's __init__ imports every dataset, torchvision's among them)
    spec = importlib.util.spec_from_file_location("_ref_data_util", os.path.join(MG.REF, "openpoints", "dataset", "data_util.py"))
    ref_data = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref_data)
    logits, labels, counts = R.loss_inputs(0)
    weight = ref_data.get_class_weights(counts, normalize=True)
    out = {"loss/class_weights": weight.numpy()}
    smooth_w = ref_loss.SmoothCrossEntropy(label_smoothing=0.2)
    smooth_w.weight = weight                       # (the constructor moves a weight to a GPU)
    for tag, crit in (("poly1", ref_loss.Poly1FocalLoss()), ("smooth", ref_loss.SmoothCrossEntropy(label_smoothing=0.2)),
                      ("smooth_weighted", smooth_w), ("ce", ref_loss.SmoothCrossEntropy(label_smoothing=0.0))):
        x = logits.clone().requires_grad_(True)
        v = crit(x, labels)
        v.backward()
        out[f"loss/{tag}/value"] = v.detach().numpy()
        out[f"loss/{tag}/grad"] = x.grad.numpy()
    return out


# ------------------------------------------------------------------------------------------------------- the metric
def metric_cases():
    script = import_example_script()
    out, diff, err64 = {}, 0.0, 0.0
    cases = [(n, p, t, c, tab) for n, p, t, c, tab, _ in R.crafted_cases()]
    for i, (B, N, C) in enumerate(((5, 63, 50), (7, 64, 64), (3, 2048, 50), (4, 1, 50))):
        logits, target, cls, table = R.random_case(B, N, C, 9500 + i)
        cases.append((f"random{i}", R.predict(logits), target, cls, table))
    for name, pred, target, cls, table in cases:
        ref = torch.stack(script.get_ins_mious(torch.from_numpy(pred), torch.from_numpy(target), torch.from_numpy(cls),
                                               table)).numpy()
        mine = R.shape_ious(pred, target, cls, table)
        exact = np.array([np.mean([100.0 if not ((pred[b] == q) | (target[b] == q)).any() else
                                   100.0 * ((pred[b] == q) & (target[b] == q)).sum() / ((pred[b] == q) | (target[b] == q)).sum()
                                   for q in table[int(cls[b])]]) for b in range(pred.shape[0])])
        diff = max(diff, float(np.abs(mine.astype(np.float64) - ref.astype(np.float64)).max()))
        err64 = max(err64, float(np.abs(ref.astype(np.float64) - exact).max()))
        out[f"m/{name}/ious"] = ref
    print(f"metric: largest |numpy statement - reference| {diff:.3e}; reference against float64 {err64:.3e}")
    out["m/mean_diff"], out["m/mean_err64"] = np.float64(diff), np.float64(err64)
    # validate :540-542, :576-592 over the crafted cases on ShapeNetPart's table, fed as three batches
    shape_classes = 16
    cls_mious = torch.zeros(shape_classes, dtype=torch.float32)
    cls_nums = torch.zeros(shape_classes, dtype=torch.int32)
    ins_miou_list = []
    for name, pred, target, cls, table in cases[:3]:
        batch = script.get_ins_mious(torch.from_numpy(pred), torch.from_numpy(target), torch.from_numpy(cls), table)
        ins_miou_list += batch
        for shape_idx in range(pred.shape[0]):
            cur_gt_label = int(cls[shape_idx])
            cls_mious[cur_gt_label] += batch[shape_idx]
            cls_nums[cur_gt_label] += 1
    ins_mious_sum, count = torch.sum(torch.stack(ins_miou_list)), torch.tensor(len(ins_miou_list))
    for cat_idx in range(shape_classes):
        if cls_nums[cat_idx] > 0:
            cls_mious[cat_idx] = cls_mious[cat_idx] / cls_nums[cat_idx]
    out["m/validate/ins_miou"] = (ins_mious_sum / count).numpy()
    out["m/validate/cls_miou"] = torch.mean(cls_mious).numpy()
    out["m/validate/cls_mious"] = cls_mious.numpy()
    return out


def main():
    out = {}
    out.update(metric_cases())
    out.update(loss_cases())
    out.update(decoder_cases())
    out.update(state_dict_case())
    out = {k: (v.astype(np.float32) if isinstance(v, np.ndarray) and v.dtype == np.float64 and "err64" not in k
               and not k.startswith("m/mean_") else v) for k, v in out.items()}
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes, {len(out)} arrays)")


if __name__ == "__main__":
    main()
