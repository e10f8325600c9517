"""CPU suite: the case table and the reference of tests/local_aggr_cases.py keep their own promises -- coverage of what
csrc/local_aggr.hip and the index stage treat differently, the exactness argument on every case's own values, the graph
kinds' claims, the index stage's statement against oracle.tile_map / inverse_map, the reference against the literal
composed statement in float64 with autograd (to equality), the float32 restatement against the float64 reference on the
exact cases, and the float cases' seeds.  No kernel runs (the row-count entry of the library needs no GPU)."""
import collections

import numpy as np
import pytest
import torch

import local_aggr_cases as C

F64, F32 = torch.float64, torch.float32


def test_the_table_covers_what_the_kernels_treat_differently():
    assert len(set(C.CASE_IDS)) == len(C.CASES)
    by_h = collections.defaultdict(list)
    for c in C.CASES:
        by_h[c.H].append(c)
    assert set(by_h) == set(C.WIDTHS) == {64, 128, 256, 512}
    assert [C.rows_in_flight(H) for H in C.WIDTHS] == [4, 4, 4, 2]
    for H, cases in by_h.items():
        G = C.rows_in_flight(H)
        classes = {(r, small) for r in range(G) for small in (False, True) if not small or r > 0}
        fixed = [c for c in cases if c.kind == "ball" and c.c]
        assert all(c.c <= c.N for c in fixed)                                 # (the cap by N never bites: c is what runs)
        assert {C.tail_class(H, c.c) for c in fixed} == classes, H
        assert {c.c for c in fixed} == {1, 2, 3, 4, 5, 6, 7, 8, 31, 32} and any(c.kind == "ball" and not c.c for c in cases)
        assert {c.kind for c in cases} == set(C.KINDS), H
        for field, values in (("gamma", C.GAMMAS), ("ldw", C.LDWS), ("train", (True, False)), ("dp", (True, False)),
                              ("r", C.RADII)):
            assert {getattr(c, field) for c in cases} == set(values), (H, field)
        # a wave's 16 consecutive queries span clouds (N < 16), with ball rows and with rows kept whole
        small = [c for c in cases if c.N < 16 and c.B > 1]
        assert {c.kind for c in small} & {"ball"} and {c.kind for c in small} & {"whole", "mixed", "ties"}, H
        # the backward's modes meet the long lists
        assert {c.train for c in cases if c.kind == "ladder"} == {True, False}, H
    assert {(c.B, c.N) for c in C.CASES} == set(C.SHAPES)
    # one query; ragged last workgroup and wave; a workgroup across two clouds; whole workgroups
    assert (1 * 63) % 64 and (2 * 65) % 64 <= 16 and (3 * 77) % 64 and 128 % 64 == 0 and (2 * 200) % 64 == 16
    assert all(c.B * c.N <= 400 for c in C.CASES)
    gen = torch.Generator().manual_seed(0)
    for H in C.WIDTHS:
        assert C.gamma_of("null", H, gen) is None and bool((C.gamma_of("pos", H, gen) > 0).all())
        for kind in ("mixed", "zeros"):
            tiles = C.gamma_of(kind, H, gen).view(-1, 64)
            assert bool(((tiles > 0).any(1) & (tiles < 0).any(1)).all())
        zeros = C.gamma_of("zeros", H, gen).view(-1, 64)
        assert bool((((zeros == 0) & torch.signbit(zeros)).any(1) & ((zeros == 0) & ~torch.signbit(zeros)).any(1)).all())


def test_every_ladder_length_occurs_and_the_chunk_edges_at_every_width():
    """Rows per point 0, 1, 2, 3, 5, 63, 64, 65, 127, 128, 129 as the index stage's statement counts them."""
    overall = set()
    for H in C.WIDTHS:
        seen = set()
        for c in C.CASES:
            if c.H == H and c.kind == "ladder":
                inp = C.exact_inputs(c)
                cnt = C.gather_rows(inp["idx"])["cnt"]
                for b, taken in enumerate(inp["ladder"]):
                    for p, n_rows in taken.items():
                        assert int(cnt[b * c.N + p]) == n_rows
                        seen.add(n_rows)
        assert {0, 1, 2, 3, 5, 63, 64, 65, 127, 128, 129} <= seen, (H, sorted(seen))
        overall |= seen
    assert overall == set(C.LADDER)


def _composed(case, inp, want):
    """The literal statement in float64 with autograd: gather p[idx] - p[q], divide by r, concatenate with f[idx], multiply
    by W = [Wp | Wf], take the extremum over K by a gather at the reference's own sel;
    L = sum gsel ext + sum (D y^2 / 2 + E y).  A zero-valued probe per gathered point takes dL/dU."""
    B, N, H = case.B, case.N, case.H
    p = inp["p"].double().requires_grad_()
    Wp = inp["W"][:, :3].double().requires_grad_()
    Wf, f = inp["W"][:, 3:].double(), inp["f"].double()
    probe = torch.zeros(B, N, H, dtype=F64, requires_grad=True)
    j = inp["idx"].long()
    feat = torch.cat([(C._take(p, j) - p.unsqueeze(2)) / inp["r"], C._take(f, j)], -1)         # (B,N,32,7)
    y = feat @ torch.cat([Wp, Wf], 1).t() + C._take(probe, j)
    ext = torch.gather(y, 2, want["sel"].long().unsqueeze(2)).squeeze(2)
    loss = (inp["gsel"].double() * ext).sum()
    if case.train:
        D, E = inp["de"][:H].double(), inp["de"][H:].double()
        loss = loss + (0.5 * D * y * y + E * y).sum()
    loss.backward()
    return y.detach(), ext.detach(), probe.grad, Wp.grad, p.grad


@pytest.mark.parametrize("case", C.CASES, ids=C.CASE_IDS)
def test_case_claims_and_reference(case):
    from oracle import oracle as O
    B, N, H = case.B, case.N, case.H
    inp = C.exact_inputs(case)
    want = C.expected(case, inp)
    idx = inp["idx"]
    assert idx.shape == (B, N, C.K) and idx.dtype == torch.int32 and inp["wp"].shape == (H, case.ldw)
    assert torch.equal(inp["U"], inp["f"] @ inp["W"][:, 3:].t())
    C.exact_range(case, inp, want)

    # ---- the graph kind's claim
    folded, c = C.ball_structure(idx)
    rows = want["rows"]
    if case.kind == "ball":
        assert bool(folded.all())
        if case.c:
            assert bool((c == case.c).all())
        else:
            assert len(set(c.reshape(-1).tolist())) > min(3, N - 1) or N == 1
    if case.kind == "whole":
        form = (torch.arange(B * N) % 5).view(B, N)
        assert not bool(folded[form == 0].any()) and not bool(folded[form == 1].any())
        assert bool(folded[form == 2].all()) and bool((c[form == 2] == 4).all())
        assert bool((idx[..., 2] == idx[..., 0])[form == 0].all()) and bool((idx[..., 1] == idx[..., 0])[form == 1].all())
        assert bool((idx[..., 1] == idx[..., 2])[form == 2].all())            # the same point in two rows of a folded query
        if N >= C.K:
            assert all(len(set(r)) == C.K for r in idx[form == 3].tolist()) and bool((c[form == 3] == C.K).all())
        assert any(len(set(r)) < C.K for r in idx[form == 4].tolist())
    if case.kind == "mixed":
        assert bool(folded.any()) and not bool(folded.all())
    if case.kind == "ties":
        assert bool((inp["p"] == inp["p"][:, torch.arange(N) % C.palette(N)]).all())
        assert bool((inp["U"] == inp["U"][:, torch.arange(N) % C.palette(N)]).all())
        t = want["y"] * C.sign_of(inp["gamma"], H)
        at = t == t.max(2, keepdim=True)[0]                                   # (B,N,32,H): slots that attain the extremum
        who = idx.long().unsqueeze(-1).expand(-1, -1, -1, H)
        two = torch.where(at, who, N).min(2)[0] != torch.where(at, who, -1).max(2)[0]
        assert bool(two.all()), "an extremum attained by one neighbour only"
        form = (torch.arange(B * N) % 4).view(B, N)
        assert bool(folded[form == 1].all()) and bool((c[form == 1] % 2 == 0).all()) and not bool(folded[form == 3].any())
        assert bool((want["sel"][form == 3] == 0).all()) and bool((want["sel"][..., :16] == 0).all())
        assert bool((want["y"][..., :16] == 0).all()) and bool((want["sel"] != 0).any())
    assert bool(rows["occ"].eq(torch.bincount((idx.long() + torch.arange(B).view(B, 1, 1) * N).reshape(-1),
                                              minlength=B * N)).all()), "occ counts the positions"

    # ---- the index stage's statement against the oracle's serial one
    tm = O.tile_map(idx.numpy())
    inv = O.inverse_map(tm, inp["p"].numpy(), N, N)
    info = tm["rowinfo"].reshape(-1).astype(np.int64)
    q_of = np.repeat(tm["tq0"].astype(np.int64), 32) + (info & 0xff)
    at = 0
    for gn, n_rows in enumerate(rows["cnt"].tolist()):
        lst = inv["lists"].get(gn, [])
        assert len(lst) == n_rows and lst == sorted(lst)
        sl = slice(at, at + n_rows)
        at += n_rows
        assert rows["point"][sl].tolist() == [gn] * n_rows and q_of[lst].tolist() == rows["query"][sl].tolist()
        assert ((info[lst] >> 8) & 0xff).tolist() == rows["slot"][sl].tolist()
        assert ((info[lst] >> 16) & 0xff).tolist() == rows["mult"][sl].tolist()
        assert inv["occ"].get(gn, 0) == float(rows["occ"][gn])
        assert np.array_equal(np.asarray(inv["sp"].get(gn, np.zeros(3))), rows["sp"][gn].numpy())

    # ---- the reference against the literal composed statement, to equality
    y, ext, dU, dWp, dp = _composed(case, inp, want)
    assert torch.equal(y, want["y"]) and torch.equal(ext, want["ext"])
    sign = C.sign_of(inp["gamma"], H)
    assert torch.equal((y * sign).max(2)[0] * sign, want["ext"])
    first = torch.gather(y, 2, want["sel"].long().unsqueeze(2)) == want["ext"].unsqueeze(2)
    earlier = torch.arange(C.K).view(1, 1, C.K, 1) < want["sel"].long().unsqueeze(2)
    assert bool(first.all()) and not bool(((y == want["ext"].unsqueeze(2)) & earlier).any())
    assert torch.equal(dU, want["dU"]), "dL/dU"
    assert torch.equal(dWp, torch.einsum("bnh,bnc->hc", want["dT"], inp["p"].double()) / inp["r"]), "dL/dWp = dT^T p / r"
    assert torch.equal(dp, want["dp"]), "dL/dp"

    # ---- the float32 restatement equals the float64 reference here
    e32, s32, ys32 = C.pool_fwd_f32(inp["U"], inp["p"], inp["W"][:, :3], idx, inp["gamma"], inp["r"])
    assert torch.equal(e32.double(), want["ext"]) and torch.equal(s32, want["sel"]) and torch.equal(ys32.double(), want["ysum"])
    ev = C.pool_bwd(want["y"], inp["gsel"], want["sel"], want["ysum"], idx, None, inp["W"][:, :3], inp["r"])[0]
    assert torch.equal(C.du_eval_f32(inp["gsel"], want["sel"], rows).double(), ev)


def test_row_counts_of_the_library_equal_the_reference():
    from adaptpoint_amd import _lib
    lib = _lib.load()
    for B, N in sorted({(c.B, c.N) for c in C.CASES} | {(c.B, c.N) for c in C.FLOAT}):
        assert lib.apn_la_pool_rows(B, N) == C.part_rows(B, N)
    assert lib.apn_la_pool_rows(0, 5) == 0


def test_outside_values_clamp_as_stated():
    for B, N in ((3, 7), (2, 65)):
        idx = C.outside_graph(B, N, torch.Generator().manual_seed(N))
        for val in C.outside_values(N):
            assert bool((idx == val).any()), val
        share = float(((idx < 0) | (idx >= N)).double().mean())
        assert 0.1 <= share <= 0.13
        cl = C.clamped(idx)
        assert bool(((cl >= 0) & (cl < N)).all()) and bool((cl[(idx >= 0) & (idx < N)] == idx[(idx >= 0) & (idx < N)]).all())
        assert bool((cl[idx < 0] == 0).all()) and bool((cl[idx >= N] == N - 1).all())
        assert int(C.clamped(torch.tensor([[[C.INT32_MIN, C.INT32_MAX]]], dtype=torch.int32).expand(1, 5, 2))[0, 0, 0]) == 0


@pytest.mark.parametrize("case", C.FLOAT, ids=C.FLOAT_IDS)
def test_float_cases_on_the_cpu(case):
    """The seeds keep the share of (query, channel) pairs whose winner float32 may decide otherwise within the cap; the
    float32 restatement stays within the derived bars of float64 and picks float64's slot wherever the margin is positive;
    its fixed-order list sum is what it claims."""
    B, N, H = case.B, case.N, case.H
    inp = C.float_inputs(case)
    Wp, idx, r = inp["W"], inp["idx"], inp["r"]
    assert bool(torch.isnan(inp["wp"][:, 3:]).all()) and len({c.r for c in C.FLOAT}) >= 3
    ref = C.pool_fwd(inp["U"], inp["p"], Wp, idx, inp["gamma"], r)
    ybar = C.y_bar(inp["U"], inp["p"], Wp, idx, r)
    margin = C.sel_margin(ref["y"], ybar, idx, C.sign_of(inp["gamma"], H))
    dropped = float((margin <= 0).double().mean())
    print(f"{case.name}: share of (query, channel) pairs dropped from the sel comparison {dropped:.2e}")
    assert dropped <= C.SEL_DROP_CAP
    y32 = C.positions_f32(inp["U"], inp["p"], Wp, idx, r)
    assert float(((y32.double() - ref["y"]).abs() / ybar.clamp_min(1e-300)).max()) <= 1.0
    e32, s32, ys32 = C.pool_fwd_f32(inp["U"], inp["p"], Wp, idx, inp["gamma"], r)
    assert torch.equal(s32[margin > 0], ref["sel"][margin > 0])
    rows = C.gather_rows(idx, inp["p"])
    ev32 = C.du_eval_f32(inp["gsel"], s32, rows).reshape(B * N, H)
    g, s = inp["gsel"].reshape(B * N, H), s32.reshape(B * N, H)
    start = (torch.cumsum(rows["cnt"], 0) - rows["cnt"]).tolist()
    for pt in range(0, B * N, 13):
        acc = torch.zeros(H)
        for e in range(start[pt], start[pt] + int(rows["cnt"][pt])):
            q, slot = int(rows["query"][e]), int(rows["slot"][e])
            acc = acc + torch.where(s[q] == slot, g[q], torch.zeros(()))
        assert torch.equal(acc, ev32[pt])
    # D and E are BatchNorm's: the dense term removes the gradient's mean and its projection on yhat
    D, E = inp["de"][:H].double(), inp["de"][H:].double()
    dy = (D * ref["y"] + E).sum((0, 1, 2)) + inp["gsel"].double().sum((0, 1))
    assert float((dy.abs() / inp["gsel"].double().abs().sum((0, 1))).max()) < 1e-5
