"""Float64 restatement of PointMLP (tests/test_pointmlp_cpu.py, tests/test_gpu_pointmlp.py, tests/test_gpu_affine_group.py,
tests/golden/make_golden_pointmlp.py): plain torch operations under autograd on float64 copies of a module's parameters,
the grouped (B,S,K,2C) tensor materialised -- the composed form, stated once more from the formulas

    d[s,k,:] = x[idx[s,k],:] - x[fps_idx[s],:]
    sigma    = unbiased std of all S K C entries of d (per cloud),   r = 1 / (sigma + 1e-5)
    grouped  = [alpha d r + beta ; x[fps_idx[s],:]]
    y        = W grouped

The graphs (`affine_group.GroupIndex`: fps_idx, idx) are inputs: the restatement is about the arithmetic behind them.
Also here: the HOISTED form of one stage's first layer and its hand-written backward pass (`hoisted_forward`,
`hoisted_backward`), in whatever dtype they are given -- what csrc/affine_group.hip computes, kernel by kernel."""
import numpy as np
import torch

import golden_inputs as GI
from invres_reference import _State, rel, sample_index  # noqa: F401

NARROW = dict(embed_dim=16, k_neighbors=[8, 8, 8, 8])          # the fixture's model, at B = 4, N = 64
NARROW_B, NARROW_N = 4, 64
ELITE = dict(embed_dim=32, groups=1, res_expansion=0.25, activation="relu", bias=False, use_xyz=False,
             normalize="anchor", dim_expansion=[2, 2, 2, 1], pre_blocks=[1, 1, 2, 1], pos_blocks=[1, 1, 2, 1],
             k_neighbors=[24, 24, 24, 24], reducers=[2, 2, 2, 2])


def classifier_inputs(B, N, seed):
    """pos (B,N,3) on the unit sphere, x (B,4,N) = (x, y, z, height), labels (B,) -- from a seed."""
    pos = torch.from_numpy(GI.unit_sphere_cloud(B, N, seed=1700 + seed))
    height = pos[:, :, 1:2] - pos[:, :, 1:2].min(1, keepdim=True)[0]
    x = torch.cat([pos, height], -1).transpose(1, 2).contiguous()
    gt = torch.from_numpy(np.random.default_rng(1800 + seed).integers(0, 15, size=B))
    return pos, x, gt


def no_dropout(model):
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    return model


def gather_rows(pts, idx):
    """pts (B,N,C), idx (B,S[,K]) -> (B,S[,K],C)."""
    B = pts.shape[0]
    return pts[torch.arange(B, device=pts.device).view([B] + [1] * (idx.dim() - 1)), idx.long()]


def grouped_affine(pts, idx, fps_idx, alpha, beta, detach_sigma=False):
    """LocalGrouper(normalize="anchor", use_xyz=False): pts (B,N,C) -> (B,S,K,2C)."""
    B = pts.shape[0]
    K = idx.shape[2]
    anchor = gather_rows(pts, fps_idx)
    d = gather_rows(pts, idx) - anchor.unsqueeze(2)
    sigma = d.reshape(B, -1).std(-1)
    if detach_sigma:
        sigma = sigma.detach()
    g = alpha.reshape(1, 1, 1, -1) * (d / (sigma.view(B, 1, 1, 1) + 1e-5)) + beta.reshape(1, 1, 1, -1)
    return torch.cat([g, anchor.unsqueeze(2).expand(-1, -1, K, -1)], -1)


def composed_first_layer(pts, idx, fps_idx, alpha, beta, weight, detach_sigma=False):
    """y (B,O,S K) = W grouped, position s K + k."""
    g = grouped_affine(pts, idx, fps_idx, alpha, beta, detach_sigma)
    B, S, K, _ = g.shape
    return torch.einsum('oc,bskc->bosk', weight.reshape(weight.shape[0], -1), g).reshape(B, -1, S * K)


def hoisted_forward(pts, idx, fps_idx, alpha, beta, weight):
    """The same y from [P | Q] = x [W1 alpha | W2]^T at the points: -> (y (B,O,S K), saved)."""
    B, N, C = pts.shape
    S, K = idx.shape[1:]
    w = weight.reshape(weight.shape[0], 2 * C)
    wa, w2 = w[:, :C] * alpha.reshape(1, C), w[:, C:]
    c0 = w[:, :C] @ beta.reshape(C)
    P, Q = pts @ wa.t(), pts @ w2.t()
    d = gather_rows(pts, idx) - gather_rows(pts, fps_idx).unsqueeze(2)
    n = S * K * C
    mu = d.reshape(B, -1).mean(-1)
    sigma = ((d.reshape(B, -1) - mu.view(B, 1)) ** 2).sum(-1).div(n - 1).sqrt()
    r = 1.0 / (sigma + 1e-5)
    Pa, Qa = gather_rows(P, fps_idx), gather_rows(Q, fps_idx)
    y = r.view(B, 1, 1, 1) * (gather_rows(P, idx) - Pa.unsqueeze(2)) + Qa.unsqueeze(2) + c0
    saved = dict(P=P, Q=Q, r=r, sigma=sigma, mu=mu, d=d, wa=wa, w2=w2, n=n)
    return y.permute(0, 3, 1, 2).reshape(B, -1, S * K), saved


def scatter_rows(vals, idx, N):
    """sum of vals (B,M,O) into rows idx (B,M) of a (B,N,O) tensor."""
    out = torch.zeros(vals.shape[0], N, vals.shape[2], dtype=vals.dtype, device=vals.device)
    return out.index_put((torch.arange(vals.shape[0], device=vals.device).view(-1, 1).expand_as(idx), idx.long()), vals,
                         accumulate=True)


def hoisted_backward(gy, pts, idx, fps_idx, saved, sigma_path=True):
    """The backward pass by its formulas: gy (B,O,S K) -> dict(dP, dQ, dc0, dr, kappa, dx_sigma, dx, dwa, dw2)."""
    B, N, C = pts.shape
    S, K = idx.shape[1:]
    g = gy.reshape(B, -1, S, K).permute(0, 2, 3, 1)                       # (B,S,K,O)
    O = g.shape[-1]
    G = g.sum(2)                                                          # (B,S,O)
    r, sigma, mu, d, n = saved['r'], saved['sigma'], saved['mu'], saved['d'], saved['n']
    A = scatter_rows(g.reshape(B, S * K, O), idx.reshape(B, S * K), N)
    Ga = scatter_rows(G, fps_idx, N)
    dP, dQ = r.view(B, 1, 1) * (A - Ga), Ga
    dc0 = G.sum((0, 1))
    P = saved['P']
    dr = (g * (gather_rows(P, idx) - gather_rows(P, fps_idx).unsqueeze(2))).sum((1, 2, 3))
    kappa = -r * r * dr / ((n - 1) * sigma)
    dm = d - mu.view(B, 1, 1, 1)
    dxs = kappa.view(B, 1, 1) * (scatter_rows(dm.reshape(B, S * K, C), idx.reshape(B, S * K), N)
                                 - scatter_rows(dm.sum(2), fps_idx, N))
    dx = dP @ saved['wa'] + dQ @ saved['w2']
    if sigma_path:
        dx = dx + dxs
    dwa = torch.einsum('bno,bnc->oc', dP, pts)
    dw2 = torch.einsum('bno,bnc->oc', dQ, pts)
    return dict(dP=dP, dQ=dQ, dc0=dc0, dr=dr, kappa=kappa, dx_sigma=dxs, dx=dx, dwa=dwa, dw2=dw2)


class _MlpState(_State):
    def res_blocks(self, t, pre, n, training):
        for j in range(n):
            h = self.convblock(t, f"{pre}.operation.{j}.net1", training)
            z = self.convblock(h, f"{pre}.operation.{j}.net2", training, act=False)
            t = self.relu(z + t)
        return t

    def stage(self, enc, i, pre, x, graph, training):
        """x (B,C,N) -> (B,O,S)."""
        g = grouped_affine(x.transpose(1, 2), graph.idx, graph.fps_idx,
                           self.P[f"{pre}local_grouper_list.{i}.affine_alpha"],
                           self.P[f"{pre}local_grouper_list.{i}.affine_beta"])
        t = self.convblock(g.permute(0, 3, 1, 2), f"{pre}pre_blocks_list.{i}.transfer.net", training)   # (B,O,S,K)
        t = self.res_blocks(t, f"{pre}pre_blocks_list.{i}", len(enc.pre_blocks_list[i].operation), training)
        t = self.pool(t)
        return self.res_blocks(t, f"{pre}pos_blocks_list.{i}", len(enc.pos_blocks_list[i].operation), training)

    def pointmlp(self, enc, pre, x, graphs, training):
        x = self.convblock(x, pre + 'embedding.net', training)
        for i in range(enc.stages):
            x = self.stage(enc, i, pre, x, graphs[i], training)
        x = self.pool(x)
        head = enc.classifier
        for i, m in enumerate(head):
            name = f"{pre}classifier.{i}"
            if isinstance(m, torch.nn.Linear):
                x = x @ self.P[name + '.weight'].t() + self.P[name + '.bias']
            elif isinstance(m, torch.nn.BatchNorm1d):
                x = self.relu(self.bn(x, name, training))
            elif isinstance(m, torch.nn.Dropout):
                assert m.p == 0 or not training, "the restatement has no dropout"
        return x


def run_classifier64(model, pos, x, graphs, gt=None, training=True):
    """`adaptpoint_amd.pointmlp.PointMlpClassifier` restated in float64 on x (B,C,N) and its stages' graphs.
    -> dict: logits; with gt: loss and grads {name: dL/dparam}; buffers after the step, margin."""
    st = _MlpState(model)
    logits = st.pointmlp(model.encoder, 'encoder.', x.detach().double(), graphs, training)
    res = {'logits': logits.detach(), 'buffers': st.after, 'margin': st.margin}
    if gt is not None:
        n_class = logits.shape[1]
        s = model.criterion.label_smoothing
        one_hot = torch.zeros_like(logits).scatter(1, gt.view(-1, 1).long(), 1)
        one_hot = one_hot * (1 - s) + (1 - one_hot) * s / (n_class - 1)
        loss = -(one_hot * torch.log_softmax(logits, dim=1)).sum(dim=1).mean()
        loss.backward()
        res.update(loss=loss.detach(), grads={n: t.grad for n, t in st.P.items() if t.grad is not None})
    return res
