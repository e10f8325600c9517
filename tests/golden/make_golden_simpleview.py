"""Regenerates tests/golden/simpleview_golden.npz (run in the BUILD container only):

    python tests/golden/make_golden_simpleview.py

The reference's own `points2depth`, `PCViews` (openpoints/models/backbone/simpleview_util.py) and `MVModel`
(openpoints/models/backbone/simpleview.py) with its `SmoothCrossEntropy`, imported in memory through make_golden's stubs
(nothing copied) and run on CPU.  `PCViews.__init__` calls `.cuda()`: `torch.Tensor.cuda` is the identity HERE, while the
reference's objects are constructed, and nowhere else; `simpleview_util.RESOLUTION` is set to 32 for the narrow runs.
Inputs are regenerated from seeds by tests/simpleview_reference.py and not stored.

  (a) a/...   `points2depth` on the exact lattice (s = 1: a/lattice_img, a/lattice_sw1 = `distribute`'s weight sum, zeros
              already ones) and on simpleview_reference.RANDOM_SHAPES at B = 3 (a/img<k>, a/sw1_<k>); a/grad: the
              reference's x.grad of sum(g * img) for RANDOM_SHAPES[GRAD_SHAPE]; a/err64: each image's distance to the
              float64 statement
  (b) b/img   `PCViews.get_img` on clouds(4, 64, seed 0, 32, 32); b/err64
  (c) c/...   the narrow `MVModel` (channels 4, 32 x 32) + SmoothCrossEntropy(0.3) in training mode, dropout 0, name-seeded
              weights, on classifier_inputs(0): logits, loss, BatchNorm buffers after the step, every parameter's gradient
              (sampled beyond 8192 entries), dpos; c/err64 (information, read by no test): the distance of the
              reference's float32 results from this library's composed mirror run in float64 (logits, loss, dpos, worst
              weight gradient)
  (d) d/logits the same model in eval mode
  (e) e/...   the name -> shape list of the default `MVModel()`
"""
import contextlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402
import simpleview_reference as R  # noqa: E402

OUT = os.path.join(HERE, "simpleview_golden.npz")


def import_reference():
    MG.import_reference()
    import openpoints.models.backbone.simpleview as ref_sv
    import openpoints.models.backbone.simpleview_util as ref_util
    import openpoints.loss.build as ref_loss
    return ref_sv, ref_util, ref_loss


@contextlib.contextmanager
def cuda_is_identity():
    keep = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        yield
    finally:
        torch.Tensor.cuda = keep


def points2depth_with_weight(ref_util, q, H, W, sx, sy):
    """The reference's points2depth and, beside it, what its `distribute` returned as the weight sum."""
    seen = []
    keep = ref_util.distribute

    def spy(**kw):
        out = keep(**kw)
        seen.append(out[1].detach().clone())
        return out
    ref_util.distribute = spy
    try:
        img = ref_util.points2depth(q, H, W, size_x=sx, size_y=sy)
    finally:
        ref_util.distribute = keep
    return img, seen[0].view(img.shape)


def rasteriser_cases(ref_util):
    out, errs = {}, []
    q = R.lattice()
    img, sw1 = points2depth_with_weight(ref_util, torch.from_numpy(q), 8, 8, 1, 1)
    out["a/lattice_img"], out["a/lattice_sw1"] = img.numpy(), sw1.numpy()
    st_img, st_sw = R.points2depth(q, 8, 8, 1, 1)
    assert np.array_equal(st_img, img.numpy()) and np.array_equal(st_sw + (st_sw == 0), sw1.numpy()), "lattice"
    valid, pixel, _, _ = R._splats(q, 8, 8, 1, 1, np.float32)
    print("lattice: the float32 statement is bit-equal; most splats on a pixel:",
          max(int(np.bincount(pixel[b][valid[b]]).max()) for b in range(len(q))))
    for k, (H, W, sx, sy, N) in enumerate(R.RANDOM_SHAPES):
        q = R.camera_points(R.RANDOM_B, N, k)
        x = torch.from_numpy(q).requires_grad_(k == R.GRAD_SHAPE)
        img, sw1 = points2depth_with_weight(ref_util, x, H, W, sx, sy)
        out[f"a/img{k}"], out[f"a/sw1_{k}"] = img.detach().numpy(), sw1.numpy()
        st_img, st_sw = R.points2depth(q, H, W, sx, sy)
        assert np.array_equal(st_img, out[f"a/img{k}"]) and np.array_equal(st_sw + (st_sw == 0), out[f"a/sw1_{k}"]), k
        errs.append(R.rel(out[f"a/img{k}"], R.points2depth(q, H, W, sx, sy, np.float64)[0]))
        if k == R.GRAD_SHAPE:
            g = np.random.default_rng(77).normal(size=img.shape).astype(np.float32)
            (img * torch.from_numpy(g)).sum().backward()
            out["a/grad"] = x.grad.numpy()
            assert not x.grad[..., :2].any() and x.grad[..., 2].any()
            print("gradient: reference against the float64 statement",
                  "%.2e" % R.rel(out["a/grad"], R.points2depth_grad(q, g, H, W, sx, sy)))
        print(f"shape {k} {(H, W, sx, sy, N)}: bit-equal; float32 against float64 {errs[-1]:.2e}")
    out["a/err64"] = np.array(errs)
    return out


def views_case(ref_util):
    with cuda_is_identity():
        views = ref_util.PCViews()
    rot, trans = R.view_matrices()
    assert np.array_equal(views.rot_mat.numpy(), rot) and np.array_equal(views.translation.numpy().reshape(-1, 3), trans)
    p = R.clouds(R.NARROW_B, R.NARROW_N, 0, R.NARROW_RES, R.NARROW_RES)
    img = views.get_img(torch.from_numpy(p)).numpy()
    st = R.depth_views(p, rot, trans, R.NARROW_RES, R.NARROW_RES)[0]
    assert np.array_equal(st, img), "PCViews.get_img: the float32 statement differs"
    err = R.rel(img, R.depth_views(p, rot, trans, R.NARROW_RES, R.NARROW_RES, dtype=np.float64)[0])
    print(f"six views: bit-equal; float32 against float64 {err:.2e}")
    return {"b/img": img, "b/err64": np.float64(err)}


def reference_classifier(ref_sv, ref_loss):
    from adaptpoint_amd.pointnext import fill_parameters_by_name
    with cuda_is_identity():
        model = ref_sv.MVModel(**R.narrow())

    class _Cls(torch.nn.Module):          # BaseCls without the registry, named as SimpleViewClassifier
        def __init__(self):
            super().__init__()
            self.encoder = model
            self.criterion = ref_loss.SmoothCrossEntropy(label_smoothing=0.3)

        def forward(self, data):
            return self.encoder(data)

        def get_logits_loss(self, data, gt):
            logits = self.forward(data)
            return logits, self.criterion(logits, gt.long())
    return R.no_dropout(fill_parameters_by_name(_Cls()))


def mirror():
    from adaptpoint_amd.simpleview import SimpleViewClassifier
    from adaptpoint_amd.pointnext import fill_parameters_by_name
    return R.no_dropout(fill_parameters_by_name(SimpleViewClassifier(fused=False, **R.narrow())))


def model_cases(ref_sv, ref_loss):
    pos, gt = R.classifier_inputs(0)
    ref = reference_classifier(ref_sv, ref_loss).train()
    got = R.train_step(ref, pos, gt)
    out = {"c/logits": got['logits'].numpy(), "c/loss": got['loss'].numpy(), "c/dpos": got['dpos'].numpy()}
    for n, g in got['grads'].items():
        out[f"c/grad/{n}"] = g.numpy().ravel()[R.sample_index(n, g.numel())]
    for n, b in ref.named_buffers():
        out[f"c/buf/{n}"] = b.numpy()
    r64 = R.run64(mirror().train(), pos, gt)
    errs = [R.rel(got['logits'], r64['logits']), R.rel(got['loss'], r64['loss']), R.rel(got['dpos'], r64['dpos'])]
    errs.append(max(R.rel(g, r64['grads'][n]) for n, g in got['grads'].items() if g.dim() > 1))
    print("narrow model: reference fp32 against the mirror in float64: logits %.2e loss %.2e dpos %.2e worst weight gradient %.2e" % tuple(errs))
    out["c/err64"] = np.array(errs)
    ref = reference_classifier(ref_sv, ref_loss).eval()
    with torch.no_grad():
        out["d/logits"] = ref({'pos': pos}).numpy()
    return out


def shapes_case(ref_sv):
    with cuda_is_identity():
        sd = ref_sv.MVModel().state_dict()
    return {"e/names": np.array(list(sd.keys())),
            "e/shapes": np.array([",".join(str(s) for s in t.shape) for t in sd.values()])}


def main():
    ref_sv, ref_util, ref_loss = import_reference()
    out = rasteriser_cases(ref_util)
    ref_util.RESOLUTION = R.NARROW_RES
    try:
        out.update(views_case(ref_util))
        out.update(model_cases(ref_sv, ref_loss))
    finally:
        ref_util.RESOLUTION = 128
    out.update(shapes_case(ref_sv))
    out = {k: (v.astype(np.float32) if isinstance(v, np.ndarray) and v.dtype == np.float64 and not k.endswith("err64")
               else v) for k, v in out.items()}
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
