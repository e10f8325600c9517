"""Regenerates tests/golden/dgcnn_golden.npz (run in the BUILD container only):

    python tests/golden/make_golden_dgcnn.py

The reference's own `DGCNN` (openpoints/models/backbone/dgcnn.py), `ClsHead` and `SmoothCrossEntropy`, imported in
memory through make_golden's stubs (nothing copied), run on CPU with name-seeded weights (`fill_parameters_by_name`);
its grouping operator is the oracle's.  Inputs are regenerated from seeds by tests/dgcnn_reference.py and not stored.

  (a) a/...   the narrow classifier (dgcnn_reference.NARROW: channels 16, embed_dim 64, k 8; in_channels 4) at B = 2,
              N = 128 in training mode, dropout off: logits, loss, the BatchNorm buffers after the step and every
              parameter's gradient (sampled beyond 8192 entries); a/seed: the input seed (of 8, the one whose float64
              restatement keeps the largest decision margin, see main); a/err64: the reference's own distance to float64
  (b) b/...   the same model in eval mode: logits
  (d) d/...   the name -> shape lists of the default encoder `DGCNN()` and of the default classifier (in_channels 4)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402
import dgcnn_reference as R  # noqa: E402

OUT = os.path.join(HERE, "dgcnn_golden.npz")
LEAKY = {'act': 'leakyrelu', 'negative_slope': 0.2}


def import_reference():
    MG.import_reference()
    import openpoints.models.layers.graph_conv as ref_gc
    import openpoints.models.backbone.dgcnn as ref_dgcnn
    import openpoints.models.classification.cls_base as ref_cls
    import openpoints.loss.build as ref_loss
    ref_gc.grouping_operation = MG._OracleOps._Group.apply
    return ref_dgcnn, ref_cls, ref_loss


def reference_classifier(in_channels=4, **encoder_args):
    from adaptpoint_amd.pointnext import fill_parameters_by_name
    ref_dgcnn, ref_cls, ref_loss = import_reference()
    enc = ref_dgcnn.DGCNN(in_channels=in_channels, **encoder_args)
    head = ref_cls.ClsHead(num_classes=15, in_channels=enc.out_channels, mlps=[512, 256], norm_args={'norm': 'bn1d'},
                           act_args=dict(LEAKY))

    class _Cls(torch.nn.Module):          # BaseCls (cls_base.py:13-39) without the registry/config machinery
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


def training_case(seed):
    from adaptpoint_amd.dgcnn import DgcnnClassifier
    from adaptpoint_amd.pointnext import fill_parameters_by_name
    pos, x, gt = R.classifier_inputs(R.NARROW_B, R.NARROW_N, seed)
    ref = reference_classifier(**R.NARROW).train()
    logits, loss = ref.get_logits_loss({'pos': pos, 'x': x.clone()}, gt)
    loss.backward()
    res = {"a/logits": logits.detach().numpy(), "a/loss": loss.detach().numpy()}
    for n, q in ref.named_parameters():
        res[f"a/grad/{n}"] = q.grad.numpy().ravel()[R.sample_index(n, q.numel())]
    for n, b in ref.named_buffers():
        res[f"a/buf/{n}"] = b.numpy()
    # the reference's own distance to the float64 restatement (the mirror shares the reference's names, so it carries
    # its weights; its graphs are the same cdist / topk call on the same float32 activations)
    mirror = R.no_dropout(fill_parameters_by_name(DgcnnClassifier(**R.NARROW))).train()
    with torch.no_grad():
        mirror(({'pos': pos, 'x': x.clone()}), keep_graphs=True)
    fresh = R.no_dropout(fill_parameters_by_name(DgcnnClassifier(**R.NARROW))).train()
    r64 = R.run_classifier64(fresh, pos, x, mirror.encoder.last_graphs, gt)
    errs = [R.rel(logits, r64['logits']), R.rel(loss, r64['loss'])]
    errs += [R.rel(q.grad, r64['grads'][n]) for n, q in ref.named_parameters() if q.dim() > 1]
    print(f"seed {seed}: margin {r64['margin']:.1e}; reference fp32 against float64: logits {errs[0]:.2e} loss "
          f"{errs[1]:.2e} worst weight gradient {max(errs[2:]):.2e}")
    res["a/err64"] = np.array(errs)
    res["a/margin"] = np.float64(r64['margin'])
    return res


def eval_case(seed):
    pos, x, _ = R.classifier_inputs(R.NARROW_B, R.NARROW_N, seed)
    ref = reference_classifier(**R.NARROW).eval()
    with torch.no_grad():
        return {"b/logits": ref({'pos': pos, 'x': x.clone()}).numpy()}


def shapes_case():
    ref_dgcnn, _, _ = import_reference()
    res = {}
    for tag, sd in (("enc", ref_dgcnn.DGCNN().state_dict()), ("cls", reference_classifier().state_dict())):
        res[f"d/{tag}_names"] = np.array(list(sd.keys()))
        res[f"d/{tag}_shapes"] = np.array([",".join(str(s) for s in t.shape) for t in sd.values()])
    return res


def main():
    out = {}
    # Of 8 seeded inputs the one whose float64 restatement keeps its LeakyReLU gates and pool winners farthest from
    # switching (a criterion of the restatement alone); the seed is stored.  a/err64 is for the record only: at B = 2
    # the head's BatchNorm1d normalises the difference of two samples, which amplifies float32 rounding far beyond
    # 1e-5 in EITHER float32 implementation -- the fixture pins the mirror to the reference, operation for operation.
    cases = [training_case(seed) for seed in range(8)]
    seed = int(np.argmax([c["a/margin"] for c in cases]))
    case = cases[seed]
    out.update(case)
    out["a/seed"] = np.int64(seed)
    out.update(eval_case(seed))
    out.update(shapes_case())
    out = {k: (v.astype(np.float32) if isinstance(v, np.ndarray) and v.dtype == np.float64 and not k.endswith("err64")
               else v) for k, v in out.items()}
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
