"""GPU suite: the kernels of csrc/affine_group.hip through their raw entries, on EXACT cases compared with numpy for
equality.  Inputs are small integers and r, kappa powers of two, so every fp32 sum and product is exact whatever its
order; what is compared to a tolerance is BatchNorm's folded mean and variance only (their M2 shares are rounded to fp32).

Shapes: the smallest at which each mechanism can break -- one position; S K = 480, no multiple of the 128-position
statistics tile; S = N; K at its bound of 64 with a ragged S; O = 1024 (sixteen channel chunks).  In the clouds: a point
nothing gathers, a point every position gathers (cloud 0 of the multi-cloud cases: a list of S K), a neighbour repeated
inside a row, duplicate anchors, and indices outside the cloud (clamped by the kernels and by the reference alike)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(1, 8, 1, 1, 16, 32), (3, 40, 20, 24, 16, 32), (2, 64, 64, 8, 32, 64), (2, 70, 33, 64, 64, 128),
          (1, 32, 16, 24, 16, 1024)]


def _ints(rng, shape, lo, hi):
    return rng.integers(lo, hi + 1, size=shape).astype(np.float32)


class Case:
    def __init__(self, shape, dev):
        from adaptpoint_amd import affine_group as AG
        B, N, S, K, C, O = self.shape = shape
        rng = np.random.default_rng(sum(shape))
        idx = rng.integers(0, N - 2, size=(B, S, K))              # point N - 2: gathered by nothing
        fps = rng.integers(0, N - 2, size=(B, S))
        if S == 1:
            fps[:, 0] = (idx[:, 0, 0] + 1) % (N - 2)              # (an anchor that is not its only neighbour: sigma > 0)
        if B > 1:
            idx[0] = 2                                            # every position of cloud 0 gathers point 2
        if K > 1:
            idx[-1, 0, 1] = idx[-1, 0, 0]                         # a neighbour repeated inside a row
        if S > 1:
            fps[-1, 1] = fps[-1, 0]                               # duplicate anchors
            idx[-1, S - 1, 0] = -5                                # outside the cloud: clamped to 0
            idx[-1, S - 1, K - 1] = N + 3                         # ... and to N - 1
            fps[-1, S - 1] = N + 7
        self.idx_raw, self.fps_raw = idx, fps
        self.idx, self.fps = np.clip(idx, 0, N - 1), np.clip(fps, 0, N - 1)
        self.x = _ints(rng, (B, N, C), -3, 3)
        self.pq = _ints(rng, (B, N, 2 * O), -8, 8)
        self.r = (2.0 ** rng.integers(-2, 3, size=B)).astype(np.float32)
        self.c0 = _ints(rng, (O,), -4, 4)
        self.gy = _ints(rng, (B, O, S * K), -3, 3)
        self.kappa = (2.0 ** rng.integers(-3, 2, size=B)).astype(np.float32) * np.where(rng.random(B) < 0.5, -1, 1).astype(np.float32)
        self.mu = (rng.integers(-4, 5, size=B) * 0.5).astype(np.float32)
        self.dev = dev
        t = lambda a, dt=None: torch.from_numpy(np.ascontiguousarray(a)).to(dev) if dt is None else \
            torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(dev)
        self.t = t
        self.graph = AG.group_index(t(fps, torch.int32), torch.zeros(B, S, 3, device=dev), t(idx, torch.int32), N)
        self.bi = np.arange(B)[:, None, None]

    def gather(self, a, rows):                                    # a (B,N,O), rows (B,S[,K]) -> (B,S[,K],O)
        return a[self.bi if rows.ndim == 3 else self.bi[:, :, 0], rows]

    def scatter(self, vals, rows):                                # the sum of vals (B,...,O) into (B,N,O)
        B, N = self.shape[:2]
        out = np.zeros((B, N, vals.shape[-1]))
        np.add.at(out, (self.bi if rows.ndim == 3 else self.bi[:, :, 0], rows), vals)
        return out

    def y_ref(self):
        B, N, S, K, C, O = self.shape
        P, Q = self.pq[..., :O].astype(np.float64), self.pq[..., O:].astype(np.float64)
        Pa, Qa = self.gather(P, self.fps), self.gather(Q, self.fps)
        y = self.r.astype(np.float64)[:, None, None, None] * (self.gather(P, self.idx) - Pa[:, :, None]) + Qa[:, :, None] + self.c0
        return y.transpose(0, 3, 1, 2).reshape(B, O, S * K)


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "x".join(map(str, s)))
def case(request, dev):
    return Case(request.param, dev)


def test_the_graph_of_the_case_has_its_edge_cases(case):
    B, N, S, K, C, O = case.shape
    cnt = case.graph.nbr_cnt_off[0].view(B, N).cpu().numpy()
    ref = np.zeros((B, N), dtype=np.int64)
    np.add.at(ref, (np.arange(B)[:, None, None], case.idx), 1)
    assert np.array_equal(cnt, ref) and int(case.graph.anc_cnt_off[0].sum()) == B * S
    assert (cnt == 0).any()                                        # a point nothing gathers
    if B > 1:
        assert cnt[0, 2] == S * K                                  # a point every position gathers
    if S > 1:
        assert int(case.graph.anc_cnt_off[0].max()) >= 2           # duplicate anchors


def test_moments(case):
    from adaptpoint_amd import affine_group as AG
    x = case.t(case.x)
    mom = AG.moments(x, case.graph).cpu().numpy()
    d = case.gather(case.x.astype(np.float64), case.idx) - case.gather(case.x.astype(np.float64), case.fps)[:, :, None]
    B = case.shape[0]
    assert np.array_equal(mom[:, 0], d.reshape(B, -1).sum(1)) and np.array_equal(mom[:, 1], (d * d).reshape(B, -1).sum(1))


def _combine(case, training, **eval_args):
    from adaptpoint_amd import _lib
    from adaptpoint_amd.fused import _call, _ptr
    B, N, S, K, C, O = case.shape
    dev = case.dev
    lib = _lib.load()
    t = case.t
    pq, r, c0 = t(case.pq), t(case.r), t(case.c0)
    idx, fps = t(case.idx_raw, torch.int32), t(case.fps_raw, torch.int32)     # the RAW indices: the kernel clamps
    y = torch.full((B, O, S * K), float('nan'), device=dev)
    tiles = lib.apn_pw_conv_tiles(B, S * K)
    part = torch.full((tiles, 2, O), float('nan'), device=dev)
    out = torch.full((B, O, S * K), float('nan'), device=dev)
    stat = torch.full((4, O), float('nan'), device=dev)
    e = {k: t(v) for k, v in eval_args.items()}
    _call("apn_ag_combine_fwd", dev, B, N, S, K, O, pq.data_ptr(), idx.data_ptr(), fps.data_ptr(), r.data_ptr(),
          c0.data_ptr(), y.data_ptr(), part.data_ptr() if training else None, int(training), _ptr(e.get('gamma')),
          _ptr(e.get('beta')), _ptr(e.get('rm')), _ptr(e.get('rv')), 0.0, 1, stat.data_ptr() if not training else None,
          out.data_ptr() if not training else None)
    return y, part, tiles, out, stat


def test_combine_forward_and_the_folded_statistics(case):
    from adaptpoint_amd.fused import _call
    B, N, S, K, C, O = case.shape
    y, part, tiles, _, _ = _combine(case, True)
    ref = case.y_ref()
    assert np.array_equal(y.cpu().numpy().astype(np.float64), ref)
    assert torch.isfinite(part).all()
    # the partial rows, folded by apn_pw_bn_act (float64): stat = {mean, invstd, scale, shift}
    eps = 1e-5
    stat = torch.empty(4, O, device=case.dev)
    out = torch.empty_like(y)
    _call("apn_pw_bn_act", case.dev, B, O, S * K, y.data_ptr(), part.data_ptr(), tiles, None, None, eps, 0.1, 1, 0, None,
          None, None, stat.data_ptr(), out.data_ptr())
    stat = stat.cpu().numpy().astype(np.float64)
    per = ref.transpose(1, 0, 2).reshape(O, -1)
    mean, var = per.mean(1), per.var(1)
    # 1e-6 relative, as the fold is float64: every tile sum is a quarter-integer and exact in fp32, so the mean carries
    # the rounding of one fp32 store; atol only for a channel whose sum is exactly zero.  The variance is recovered from
    # invstd = 1 / sqrt(var + eps) and compared where it is positive (a channel of one position has none).
    assert np.allclose(stat[0], mean, rtol=1e-6, atol=1e-12), np.abs(stat[0] - mean).max()
    got_var = 1.0 / (stat[1] * stat[1]) - eps
    pos = var > 0
    assert np.allclose(got_var[pos], var[pos], rtol=1e-6, atol=0), (np.abs(got_var[pos] / var[pos] - 1).max() if pos.any() else 0)
    assert np.allclose(stat[1][~pos], 1.0 / np.sqrt(eps), rtol=1e-6, atol=0)


def test_combine_forward_in_eval_mode(case):
    B, N, S, K, C, O = case.shape
    rng = np.random.default_rng(7)
    gamma, beta, rm = _ints(rng, (O,), -2, 2), _ints(rng, (O,), -3, 3), _ints(rng, (O,), -2, 2)
    rv = np.ones(O, dtype=np.float32)                               # eps = 0: invstd = 1, scale and shift are integers
    y, _, _, out, stat = _combine(case, False, gamma=gamma, beta=beta, rm=rm, rv=rv)
    ref = case.y_ref()
    assert np.array_equal(y.cpu().numpy().astype(np.float64), ref)
    sc, sh = gamma.astype(np.float64), beta.astype(np.float64) - rm.astype(np.float64) * gamma
    want = np.maximum(ref * sc[None, :, None] + sh[None, :, None], 0.0)
    assert np.array_equal(out.cpu().numpy().astype(np.float64), want)
    assert np.array_equal(stat.cpu().numpy().astype(np.float64), np.stack([rm, np.ones(O), sc, sh]))


def _lists(case):
    g = case.graph
    return (g.nbr_cnt_off.data_ptr(), g.nbr_list.data_ptr(), g.anc_cnt_off.data_ptr(), g.anc_list.data_ptr())


def test_combine_backward(case):
    from adaptpoint_amd import _lib
    from adaptpoint_amd.affine_group import _fold
    from adaptpoint_amd.fused import _call
    B, N, S, K, C, O = case.shape
    dev = case.dev
    rows = _lib.load().apn_ag_point_rows(N)
    t = case.t
    gyt = t(case.gy.transpose(0, 2, 1))
    r, pq = t(case.r), t(case.pq)
    dpq = torch.full((B, N, 2 * O), float('nan'), device=dev)
    part_dr = torch.full((rows, B), float('nan'), dtype=torch.float64, device=dev)
    part_c0 = torch.full((B * rows, O), float('nan'), dtype=torch.float64, device=dev)
    _call("apn_ag_combine_bwd", dev, B, N, S, K, O, gyt.data_ptr(), r.data_ptr(), pq.data_ptr(), *_lists(case),
          dpq.data_ptr(), part_dr.data_ptr(), part_c0.data_ptr())
    dr = _fold(part_dr, rows, B).cpu().numpy()
    dc0 = _fold(part_c0, B * rows, O).cpu().numpy()
    g = case.gy.astype(np.float64).reshape(B, O, S, K).transpose(0, 2, 3, 1)             # (B,S,K,O)
    G = g.sum(2)
    A, Ga = case.scatter(g, case.idx), case.scatter(G, case.fps)
    dP = case.r.astype(np.float64)[:, None, None] * (A - Ga)
    got = dpq.cpu().numpy().astype(np.float64)
    assert np.array_equal(got[..., :O], dP) and np.array_equal(got[..., O:], Ga)          # every element written: no NaN left
    assert np.array_equal(dc0, G.sum((0, 1)))
    P = case.pq[..., :O].astype(np.float64)
    dr_ref = (g * (case.gather(P, case.idx) - case.gather(P, case.fps)[:, :, None])).sum((1, 2, 3))
    assert np.array_equal(dr, dr_ref)


def test_sigma_backward(case):
    from adaptpoint_amd.fused import _call
    B, N, S, K, C, O = case.shape
    dev = case.dev
    t = case.t
    x, kappa, mu = t(case.x), t(case.kappa), t(case.mu)
    idx, fps = t(case.idx_raw, torch.int32), t(case.fps_raw, torch.int32)
    dx = torch.full((B, N, C), float('nan'), device=dev)
    _call("apn_ag_sigma_bwd", dev, B, N, S, K, C, x.data_ptr(), idx.data_ptr(), fps.data_ptr(), kappa.data_ptr(),
          mu.data_ptr(), *_lists(case), dx.data_ptr())
    x64 = case.x.astype(np.float64)
    dm = case.gather(x64, case.idx) - case.gather(x64, case.fps)[:, :, None] - case.mu.astype(np.float64)[:, None, None, None]
    ref = case.kappa.astype(np.float64)[:, None, None] * (case.scatter(dm, case.idx) - case.scatter(dm.sum(2), case.fps))
    assert np.array_equal(dx.cpu().numpy().astype(np.float64), ref)


def test_res_relu_max_forward_and_backward_with_ties(case):
    """Small integers tie all the time: the FIRST maximum's slot is kept and takes the gradient; where no sum is
    positive the output is 0, the slot 0 and the gradient zero."""
    from adaptpoint_amd import affine_group as AG
    from adaptpoint_amd.fused import _call
    B, N, S, K, C, O = case.shape
    rng = np.random.default_rng(11 + S)
    z, h = _ints(rng, (B, O, S, K), -2, 2), _ints(rng, (B, O, S, K), -2, 1)
    z[:, :, 0] = -1.0                                               # query 0 of every channel: all sums negative
    h[:, :, 0] = -1.0
    g = _ints(rng, (B, O, S), -3, 3)
    zt = case.t(z.reshape(B, O, S * K)).requires_grad_(True)
    ht = case.t(h.reshape(B, O, S * K)).requires_grad_(True)
    out = AG.res_relu_max(zt, ht, K)
    v = z.astype(np.float64) + h
    m, arg = v.max(-1), v.argmax(-1)                               # numpy's argmax: the first maximum
    assert np.array_equal(out.detach().cpu().numpy().astype(np.float64), np.maximum(m, 0.0))
    # the raw entry: the kept slot as uint8, 0 where nothing is positive
    raw_out = torch.full((B, O, S), float('nan'), device=case.dev)
    sel = torch.full((B, O, S), 255, dtype=torch.uint8, device=case.dev)
    _call("apn_ag_res_relu_max", case.dev, B, O, S, K, zt.data_ptr(), ht.data_ptr(), raw_out.data_ptr(), sel.data_ptr())
    assert torch.equal(raw_out, out.detach())
    assert np.array_equal(sel.cpu().numpy(), np.where(m > 0, arg, 0).astype(np.uint8))
    out.backward(case.t(g))
    want = np.zeros_like(v)
    np.put_along_axis(want, arg[..., None], np.where(m > 0, g, 0.0)[..., None].astype(np.float64), -1)
    for grad in (zt.grad, ht.grad):
        assert np.array_equal(grad.cpu().numpy().astype(np.float64).reshape(B, O, S, K), want)
    assert (want[:, :, 0] == 0).all() and (out[:, :, 0] == 0).all()


def test_operator_on_the_case_matches_the_entries(case):
    """`affine_group_linear` end to end on the exact case (alpha = 1, beta and W integers): its y against the composed
    form in float64 within fp32 rounding of r alone, and two runs bit-identical, gradients included."""
    from adaptpoint_amd import affine_group as AG
    import pointmlp_reference as R
    B, N, S, K, C, O = case.shape
    rng = np.random.default_rng(3)
    w = case.t(_ints(rng, (O, 2 * C, 1), -1, 1))
    alpha, beta = torch.ones(C, device=case.dev), case.t(_ints(rng, (C,), -1, 1))
    runs = []
    for _ in range(2):
        x = case.t(case.x).requires_grad_(True)
        wl, al, be = (q.clone().requires_grad_(True) for q in (w, alpha, beta))
        y, part = AG.affine_group_linear(x, case.graph, al, be, wl)
        y.backward(case.t(case.gy))
        runs.append((y.detach(), part, x.grad, wl.grad, al.grad, be.grad))
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    idx, fps = case.t(case.idx), case.t(case.fps)
    leaves = [q.detach().double().requires_grad_(True) for q in (case.t(case.x), alpha, beta, w)]
    ref = R.composed_first_layer(leaves[0], idx, fps, leaves[1], leaves[2], leaves[3])
    grads = torch.autograd.grad(ref, leaves, case.t(case.gy).double())
    # bars: fp32 rounding of r and of the products (a few 1e-7 per operation, summed over 2C terms and the lists)
    assert R.rel(runs[0][0], ref) < 1e-5
    for got, want, name in zip((runs[0][2], runs[0][4], runs[0][5], runs[0][3]), grads, ("dx", "dalpha", "dbeta", "dW")):
        assert R.rel(got, want) < 1e-4, (name, R.rel(got, want))
