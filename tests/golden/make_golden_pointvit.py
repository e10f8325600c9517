"""Regenerates tests/golden/pointvit_golden.npz (run in the BUILD container only):

    python tests/golden/make_golden_pointvit.py

The reference's own `PointViT` (openpoints/models/backbone/pointvit.py) with its `PointPatchEmbed`
(openpoints/models/layers/group_embed.py), `ClsHead` and `SmoothCrossEntropy`, imported in memory through make_golden's
stubs (nothing copied), run on CPU with attribute-dict arguments and name-seeded weights (`fill_parameters_by_name`);
its sampler is the oracle's.  Inputs are regenerated from seeds by tests/pointvit_reference.py and not stored.

  (a) a/...   the narrow classifier (pointvit_reference.narrow('knn'): dim 128, depth 2, 2 heads, 16 groups of 8; T = 17)
              at B = 4, N = 64 in training mode, dropout and DropPath 0: logits, loss, the BatchNorm buffers after the step
              and every parameter's gradient (sampled beyond 8192 entries); a/seed: the input seed (of 8, the one whose
              float64 restatement keeps the largest decision margin; seeds where a rounding variant of the oracle changes
              a sampled index, or where a neighbourhood's k-th and (k+1)-th distances are closer than 1e-4 relative, are
              rejected); a/err64: the reference's own distance to float64
  (b) b/...   the same model in eval mode: logits
  (c) c/...   the ball-query grouper (radius pointvit_reference.RADIUS; no ball is empty: asserted) on the same input, training
              mode: logits, loss, the gradients of the patch embedding and the class token; c/err64
  (d) d/...   the name -> shape list of the default `PointViT()`
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402
import pointvit_reference as R  # noqa: E402
from oracle import oracle as O  # noqa: E402

OUT = os.path.join(HERE, "pointvit_golden.npz")


def import_reference():
    MG.import_reference()
    import openpoints.models.backbone.pointvit as ref_vit
    import openpoints.models.layers.group_embed as ref_embed
    import openpoints.models.classification.cls_base as ref_cls
    import openpoints.loss.build as ref_loss
    ref_embed.furthest_point_sample = MG._OracleOps.furthest_point_sample
    return ref_vit, ref_cls, ref_loss


def reference_classifier(group):
    from adaptpoint_amd.pointnext import fill_parameters_by_name
    ref_vit, ref_cls, ref_loss = import_reference()
    from easydict import EasyDict
    args = R.narrow(group)
    enc = ref_vit.PointViT(in_channels=4, embed_dim=args['embed_dim'], depth=args['depth'], num_heads=args['num_heads'],
                           embed_args=EasyDict(args['embed_args']), norm_args=EasyDict(norm='ln', eps=1.0e-6),
                           act_args=EasyDict(act='gelu'))
    head = ref_cls.ClsHead(num_classes=15, in_channels=enc.out_channels, mlps=[256, 256], norm_args={'norm': 'bn1d'})

    class _Cls(torch.nn.Module):          # BaseCls without the registry, named as PointVitClassifier
        def __init__(self):
            super().__init__()
            self.encoder, self.prediction = enc, head
            self.criterion = ref_loss.SmoothCrossEntropy(label_smoothing=0.3)

        def forward(self, data):
            return self.prediction(self.encoder.forward_cls_feat(data))

        def get_logits_loss(self, data, gt):
            logits = self.forward(data)
            return logits, self.criterion(logits, gt.long())
    return R.no_dropout(fill_parameters_by_name(_Cls()))


def mirror(group):
    from adaptpoint_amd.pointvit import PointVitClassifier
    from adaptpoint_amd.pointnext import fill_parameters_by_name
    return R.no_dropout(fill_parameters_by_name(PointVitClassifier(fused=False, **R.narrow(group))))


def index_is_robust(pos, group):
    """No rounding variant of the oracle changes a sampled index (or a ball's members), and every kNN neighbourhood's
    k-th and (k+1)-th distances differ by more than 1e-4 relative."""
    p = pos.numpy()
    S, K = R.NARROW_N // 4, 8
    try:
        idx = MG.all_variants_equal(lambda v: O.furthest_point_sampling(p, S, v))
        centre = np.take_along_axis(p, idx[..., None].astype(np.int64), 1)
        if group != 'knn':
            nbr = MG.all_variants_equal(lambda v: O.ball_query(R.RADIUS, K, p, centre, v))
            d = np.linalg.norm(p[:, None].astype(np.float64) - centre[:, :, None].astype(np.float64), axis=-1)
            assert (d < R.RADIUS).any(-1).all(), "an empty ball"
            assert nbr.shape == (p.shape[0], S, K)
            return True
    except SystemExit:
        return False
    d = np.sort(np.linalg.norm(p[:, None].astype(np.float64) - centre[:, :, None].astype(np.float64), axis=-1), -1)
    return bool(((d[..., K] - d[..., K - 1]) > 1e-4 * d[..., K]).all())


def training_case(seed, group, tag, only=None):
    from oracle import cpu_block as CB
    pos, x, gt = R.classifier_inputs(R.NARROW_B, R.NARROW_N, seed)
    if not index_is_robust(pos, group):
        print(f"seed {seed} ({group}): an index decision is too close: rejected")
        return None
    ref = reference_classifier(group).train()
    logits, loss = ref.get_logits_loss({'pos': pos, 'x': x.clone()}, gt)
    loss.backward()
    res = {f"{tag}/logits": logits.detach().numpy(), f"{tag}/loss": loss.detach().numpy()}
    for n, q in ref.named_parameters():
        if only is None or n.startswith(only):
            res[f"{tag}/grad/{n}"] = q.grad.numpy().ravel()[R.sample_index(n, q.numel())]
    if only is None:
        for n, b in ref.named_buffers():
            res[f"{tag}/buf/{n}"] = b.numpy()
    m = mirror(group).train()
    with CB.CpuOps():
        index = m.encoder.patch_embed.index(pos)
    r64 = R.run_classifier64(m, pos, x, index, gt)
    errs = [R.rel(logits, r64['logits']), R.rel(loss, r64['loss'])]
    errs += [R.rel(q.grad, r64['grads'][n]) for n, q in ref.named_parameters() if q.dim() > 1]
    print(f"seed {seed} ({group}): margin {r64['margin']:.1e}; reference fp32 against float64: logits {errs[0]:.2e} loss "
          f"{errs[1]:.2e} worst weight gradient {max(errs[2:]):.2e}")
    res[f"{tag}/err64"] = np.array(errs)
    res[f"{tag}/margin"] = np.float64(r64['margin'])
    return res


def eval_case(seed):
    pos, x, _ = R.classifier_inputs(R.NARROW_B, R.NARROW_N, seed)
    ref = reference_classifier('knn').eval()
    with torch.no_grad():
        return {"b/logits": ref({'pos': pos, 'x': x.clone()}).numpy()}


def shapes_case():
    ref_vit, _, _ = import_reference()
    from easydict import EasyDict
    embed = EasyDict(NAME='PointPatchEmbed', num_groups=256, group_size=32, subsample='fps', group='knn', feature_type='fj',
                     norm_args={'norm': 'in2d'})
    sd = ref_vit.PointViT(embed_args=embed, norm_args=EasyDict(norm='ln', eps=1.0e-6), act_args=EasyDict(act='gelu')).state_dict()
    return {"d/vit_names": np.array(list(sd.keys())),
            "d/vit_shapes": np.array([",".join(str(s) for s in t.shape) for t in sd.values()])}


def main():
    out = {}
    cases = {}
    for seed in range(8):
        if not index_is_robust(R.classifier_inputs(R.NARROW_B, R.NARROW_N, seed)[0], 'ballquery'):
            print(f"seed {seed}: the ball query is not robust: rejected")
            continue
        c = training_case(seed, 'knn', 'a')
        if c is not None:
            cases[seed] = c
    seed = max(cases, key=lambda s: cases[s]["a/margin"])
    out.update(cases[seed])
    out["a/seed"] = np.int64(seed)
    out.update(eval_case(seed))
    out.update(training_case(seed, 'ballquery', 'c', only=('encoder.patch_embed.', 'encoder.cls_token')))
    out.update(shapes_case())
    out = {k: (v.astype(np.float32) if isinstance(v, np.ndarray) and v.dtype == np.float64 and not k.endswith("err64")
               else v) for k, v in out.items()}
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
