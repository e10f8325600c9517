"""Float64 restatement of one DGCNN EdgeConv block and of the DGCNN classifier (tests/test_dgcnn_cpu.py,
tests/test_gpu_edge_conv.py, tests/test_gpu_dgcnn.py): plain torch operations under autograd on float64 copies of a
module's parameters, the grouped (B,2C,N,K) tensor materialised -- the composed form, stated once more.  The neighbour
graphs are inputs: the restatement is about the arithmetic behind them.  As `invres_reference.run_invres64` it reports
the decision margin of its pool winners and LeakyReLU gates."""
import numpy as np
import torch

import golden_inputs as GI
from invres_reference import _State, _group, rel, sample_index  # noqa: F401

NARROW = dict(channels=16, embed_dim=64, k=8)          # the fixture's model, at B = 2, N = 128
NARROW_B, NARROW_N = 2, 128


class _DgcnnState(_State):
    def leaky(self, x, slope):
        self._note(x.detach().abs(), x)
        return torch.where(x > 0, x, x * slope)

    def pool(self, x):
        if x.shape[-1] == 1:                      # K = 1: no winner to decide
            return x[..., 0]
        return super().pool(x)

    def edge(self, x, idx, pre, training):
        """The EdgeConv whose Sequential(conv, bn, LeakyReLU) is named `pre`, on x (B,C,N), idx (B,N,K) -> (B,H,N)."""
        mods = list(self.mods[pre])
        xj = _group(x, idx)
        y = self.convblock(torch.cat([x.unsqueeze(-1).expand_as(xj), xj - x.unsqueeze(-1)], 1), pre, training, act=False)
        # (the activation after the pool: the same function -- it is increasing --, and only the pooled value's gate
        # is a decision)
        return self.leaky(self.pool(y), mods[-1].negative_slope)

    def dgcnn(self, enc, pre, pos, x, graphs, training):
        feats = [self.edge(x, graphs[0], pre + 'head.gconv.nn', training)]
        self.layer_inputs = [pos]
        for i in range(len(enc.backbone)):
            self.layer_inputs.append(feats[-1].detach().transpose(1, 2))
            feats.append(self.edge(feats[-1], graphs[i + 1], f"{pre}backbone.{i}.gconv.nn", training))
        y = self.convblock(torch.cat(feats, 1), pre + 'fusion_block', training, act=False)
        y = self.leaky(y, list(enc.fusion_block)[-1].negative_slope)
        return torch.cat([y.max(-1)[0], y.mean(-1)], 1)

    def cls_head(self, head, pre, x, training):
        for i, m in enumerate(head):
            if isinstance(m, torch.nn.Dropout):
                assert m.p == 0 or not training, "the restatement has no dropout"
                continue
            name = f"{pre}.{i}"
            x = x @ self.P[name + '.0.weight'].t()
            if name + '.0.bias' in self.P:
                x = x + self.P[name + '.0.bias']
            if len(m) > 1:
                x = self.leaky(self.bn(x, name + '.1', training), m[-1].negative_slope)
        return x


def edge_inputs(B, N, C, seed=0):
    """x (B,C,N) float32 from a seed: normal features."""
    return torch.from_numpy(GI.seeded_normal((B, C, N), 1300 + seed).astype(np.float32))


def flip_every_third_gamma(edge):
    with torch.no_grad():
        edge.nn[1].weight[::3] *= -1.0
    return edge


def run_edge64(edge, x, idx, w=None, training=True):
    """The `adaptpoint_amd.dgcnn.EdgeConv` module `edge` restated in float64 on x (B,C,N) and idx (B,N,K).
    -> dict: out (B,H,N); with w: dx, grads {name: dL/dparam} for the loss (out * w).sum(); buffers after the step in
    training mode; margin: how close the nearest pool winner / LeakyReLU gate is to switching, relative to its
    tensor's rms."""
    st = _DgcnnState(edge)
    x64 = x.detach().double().requires_grad_(True)
    out = st.edge(x64, idx, 'nn', training)
    res = {'out': out.detach(), 'buffers': st.after, 'margin': st.margin}
    if w is not None:
        (out * w.double()).sum().backward()
        res.update(dx=x64.grad, grads={n: t.grad for n, t in st.P.items() if t.grad is not None})
    return res


def run_classifier64(model, pos, x, graphs, gt=None, training=True):
    """`adaptpoint_amd.dgcnn.DgcnnClassifier` restated in float64 on pos (B,N,3), x (B,C,N) and its four graphs.
    -> dict: logits; with gt: loss and grads {name: dL/dparam}; buffers, margin, layer_inputs (what each graph is the
    kNN of: (B,N,C) float64)."""
    st = _DgcnnState(model)
    feat = st.dgcnn(model.encoder, 'encoder.', pos.detach().double(), x.detach().double(), graphs, training)
    logits = st.cls_head(model.prediction.head, 'prediction.head', feat, training)
    res = {'logits': logits.detach(), 'buffers': st.after, 'margin': st.margin, 'layer_inputs': st.layer_inputs}
    if gt is not None:
        n_class = logits.shape[1]
        s = model.criterion.label_smoothing
        one_hot = torch.zeros_like(logits).scatter(1, gt.view(-1, 1).long(), 1)
        one_hot = one_hot * (1 - s) + (1 - one_hot) * s / (n_class - 1)
        loss = -(one_hot * torch.log_softmax(logits, dim=1)).sum(dim=1).mean()
        loss.backward()
        res.update(loss=loss.detach(), grads={n: t.grad for n, t in st.P.items() if t.grad is not None})
    return res


def classifier_inputs(B, N, seed):
    """pos (B,N,3) on the unit sphere, x (B,4,N) = (x, y, z, height), labels (B,) -- from a seed."""
    pos = torch.from_numpy(GI.unit_sphere_cloud(B, N, seed=1400 + seed))
    height = pos[:, :, 1:2] - pos[:, :, 1:2].min(1, keepdim=True)[0]
    x = torch.cat([pos, height], -1).transpose(1, 2).contiguous()
    gt = torch.from_numpy(np.random.default_rng(1500 + seed).integers(0, 15, size=B))
    return pos, x, gt


def no_dropout(model):
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    return model
