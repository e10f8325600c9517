"""CPU suite: the case table and the reference of tests/edge_conv_cases.py keep their own promises -- coverage of what
csrc/edge_conv.hip treats differently, the exactness argument on every case's own values, the graph kinds' claims, and the
reference against the literal composed statement in float64 with autograd.  No kernel runs (the two row-count entries of
the library need no GPU)."""
import collections

import pytest
import torch

import edge_conv_cases as C

F64 = torch.float64


def test_the_table_covers_what_the_kernels_treat_differently():
    assert len(set(C.CASE_IDS)) == len(C.CASES)
    by_h = collections.defaultdict(list)
    for c in C.CASES:
        by_h[c.H].append(c)
    assert set(by_h) == set(C.WIDTHS) == {64, 128, 256, 512}
    assert [C.rows_in_flight(H) for H in C.WIDTHS] == [4, 4, 4, 2]
    assert {1, 2, 3, 4, 5, 7, 8, 20, 33, 63, 64} <= set(C.KS) and max(C.KS) == C.K_MAX
    for H, cases in by_h.items():
        assert {c.K for c in cases} == set(C.KS)
        G = C.rows_in_flight(H)
        classes = {(r, small) for r in range(G) for small in (False, True) if (r < G and (not small or r > 0))}
        # every (K mod G, K < G) that exists, with every graph kind; each case runs in training AND in eval mode
        assert {(C.tail_class(H, c.K), c.kind) for c in cases} == {(t, kind) for t in classes for kind in C.KINDS}
        for field, values in (("ld_pad", C.LD_PADS), ("gamma", C.GAMMAS), ("slope", C.SLOPES), ("res", C.RESIDUALS),
                              ("g", C.G_LAYOUTS)):
            assert {getattr(c, field) for c in cases} == set(values), (H, field)
        assert {(c.B, c.N) for c in cases} == set(C.SHAPES), H
        # the longest neighbour rows with every kind, in both modes
        assert {c.kind for c in cases if c.K == 64} == set(C.KINDS) == {c.kind for c in cases if c.K == 63}
    # a ragged last workgroup with idle waves, a workgroup across two clouds, one point past a 64-point tile, multiples
    assert (1 * 63) % 64 and (2 * 65) % 64 <= 16 and 65 % 64 == 1 and 128 % 64 == 0 and (3 * 77) % 64 and 77 % 64
    assert all(c.B * c.N <= 400 for c in C.CASES)
    assert [(n + 1023) // 1024 for _, n, _ in C.CSR_ONLY] == [2, 3, 1]
    # the gamma forms are what their names say: both signs in every 64-channel tile, and zeros of both signs
    gen = torch.Generator().manual_seed(0)
    for H in C.WIDTHS:
        assert C.gamma_of("null", H, gen) is None and bool((C.gamma_of("pos", H, gen) > 0).all())
        for kind in ("mixed", "zeros"):
            tiles = C.gamma_of(kind, H, gen).view(-1, 64)
            assert bool(((tiles > 0).any(1) & (tiles < 0).any(1)).all())
        zeros = C.gamma_of("zeros", H, gen).view(-1, 64)
        assert bool((((zeros == 0) & torch.signbit(zeros)).any(1) & ((zeros == 0) & ~torch.signbit(zeros)).any(1)).all())


def test_every_ladder_length_occurs_at_every_width():
    """The reverse-list lengths 0, 1, 2, 3, 5, 63, 64, 65, 127, 128, 129, as the reference's own counts have them."""
    for H in C.WIDTHS:
        seen = set()
        for c in C.CASES:
            if c.H == H and c.kind == "ladder":
                inp = C.exact_inputs(c)
                pcnt = C.csr(inp["idx"])[0]
                for b, taken in enumerate(inp["ladder"]):
                    for p, cnt in taken.items():
                        assert int(pcnt[b * c.N + p]) == cnt
                        seen.add(cnt)
        assert seen == set(C.LADDER), (H, sorted(set(C.LADDER) - seen))


def _composed(case, inp, train):
    """The literal statement in float64 with autograd: gather x_j - x_i, multiply by W = [Wa | Wb], affine, activation,
    max over K by torch.max, the residual; loss = <out, g> (+ the dense term's potential sum_c D/2 y^2 + E y in training
    mode, whose gradient is D y + E).  Two zero-valued probes added to y -- one per query, one per gathered point -- take
    dL/du and dL/dv.  -> out (B,H,N), torch.max's indices (B,N,H), du, dv (B,N,H)."""
    B, N, H, K = case.B, case.N, case.H, case.K
    x, W = inp["x"].double(), inp["W"].double()
    scale, shift = inp["pack"][:H].double(), inp["pack"][H:2 * H].double()
    j = C.clamped(inp["idx"].long())
    probe_u = torch.zeros(B, N, H, dtype=F64, requires_grad=True)
    probe_v = torch.zeros(B, N, H, dtype=F64, requires_grad=True)
    take = lambda t: torch.gather(t.unsqueeze(1).expand(-1, N, -1, -1), 2, j.unsqueeze(-1).expand(-1, -1, -1, t.shape[-1]))
    xi = x.unsqueeze(2).expand(-1, -1, K, -1)
    feat = torch.cat([xi, take(x) - xi], -1)                                  # (B,N,K,2C)
    y = feat @ W.t() + probe_u.unsqueeze(2) + take(probe_v)                    # (B,N,K,H)
    z = scale * y + shift
    o, ind = torch.where(z > 0, z, inp["slope"] * z).max(dim=2)
    o = o.transpose(1, 2)
    if inp["res"] is not None:
        o = o + inp["res"].double()
    loss = (o * inp["g"].double()).sum()
    if train:
        D, E = inp["de"][:H].double(), inp["de"][H:].double()
        loss = loss + (0.5 * D * y * y + E * y).sum()
    loss.backward()
    return o.detach(), ind, probe_u.grad, probe_v.grad


@pytest.mark.parametrize("case", C.CASES, ids=C.CASE_IDS)
def test_case_claims_and_reference(case):
    B, N, H, K = case.B, case.N, case.H, case.K
    inp = C.exact_inputs(case)
    want = C.expected(case, inp)
    idx = inp["idx"]
    assert idx.shape == (B, N, K) and idx.dtype == torch.int32 and inp["uv"].shape == (B, N, 2 * H + case.ld_pad)
    C.exact_range(case, inp, want)

    # ---- the graph kind's claim
    u, v = inp["uv"][..., :H].double(), inp["uv"][..., H:2 * H].double()
    j = C.clamped(idx.long())
    inside = bool(((idx >= 0) & (idx < N)).all())
    if case.kind == "outside":
        for val in C.outside_values(N):
            assert bool((idx == val).any()), val
    else:
        assert inside
    if case.kind == "knn" and K <= N:
        assert all(len(set(row)) == K for row in idx.reshape(-1, K).tolist())
    if case.kind == "ties" and K >= 2:
        sign = 1.0 if inp["gamma"] is None else torch.where(inp["gamma"] >= 0, 1.0, -1.0).double()
        t = (u.unsqueeze(2) + torch.stack([torch.gather(v, 1, j[:, :, k:k + 1].expand(-1, -1, H)) for k in range(K)], 2)) * sign
        at = t == t.max(2, keepdim=True)[0]                                    # (B,N,K,H): slots that attain the extremum
        who = j.unsqueeze(-1).expand(-1, -1, -1, H)
        lo = torch.where(at, who, N).min(2)[0]
        hi = torch.where(at, who, -1).max(2)[0]
        share = float((lo != hi).double().mean(-1).min())                      # ... by two DIFFERENT neighbours, per query row
        assert share >= 0.5, share
        assert bool((v[:, 0] == 0).all()) and bool((v[:, C.palette(N)] == v[:, 0]).all())
    if B * N * H >= 4096 and case.gamma != "zeros":
        scale, shift = inp["pack"][:H].double(), inp["pack"][H:2 * H].double()
        assert bool((scale * want["ext"] + shift == 0).any()), "no z == 0: the activation's edge is not met"

    # ---- the reference against the literal composed statement, to equality
    for train in (True, False):
        o, ind, du, dv = _composed(case, inp, train)
        assert torch.equal(o, want["out"]), train
        # torch.max's index is the kernel's slot wherever the statement's values are strictly monotone in y: not under a
        # scale of 0 (every slot ties), nor where ReLU has flattened the extremum to 0
        zext = inp["pack"][:H].double() * want["ext"] + inp["pack"][H:2 * H].double()
        live = (inp["pack"][:H] != 0).expand(B, N, H) & ((zext > 0) | (inp["slope"] > 0))
        assert torch.equal(ind[live], want["sel"].long()[live])
        duv = want["duv"] if train else want["duv_eval"]
        assert torch.equal(du, duv[..., :H]) and torch.equal(dv, duv[..., H:]), train
    if inp["gamma"] is not None:
        zero = (inp["gamma"] == 0).expand(B, N, H)                              # gamma = +-0.0: the first maximum of y itself
        y = u.unsqueeze(2) + torch.stack([torch.gather(v, 1, j[:, :, k:k + 1].expand(-1, -1, H)) for k in range(K)], 2)
        assert torch.equal(y.max(2)[1][zero], want["sel"].long()[zero])

    # ---- eval mode: du == gsel, dv == the scatter of the selected gsel
    assert torch.equal(want["duv_eval"][..., :H], want["gsel"])
    scatter = torch.zeros(B * N, H, dtype=F64)
    sel, gsel = want["sel"].reshape(B * N, H).long(), want["gsel"].reshape(B * N, H)
    tgt = C.targets(idx).reshape(B * N, K)
    for q in range(B * N):                                                     # (plain loop: one query at a time)
        scatter[tgt[q][sel[q]], torch.arange(H)] += gsel[q]
    assert torch.equal(want["duv_eval"][..., H:].reshape(B * N, H), scatter)

    # ---- the adjoint identity: sum_ik y dL/dy = <u, du> + <v, dv>, with sum_ik y dL/dy = <ext, gsel> + <D, sum y^2> + <E, sum y>
    D, E = inp["de"][:H].double(), inp["de"][H:].double()
    p = want["part"].sum(0)
    lhs = (want["ext"] * want["gsel"]).sum() + (D * p[H:]).sum() + (E * p[:H]).sum()
    rhs = (torch.cat([u, v], -1) * want["duv"]).sum()
    assert float(lhs) == float(rhs) and abs(float(lhs)) < 2.0 ** 50

    # ---- the reverse lists: a partition of the positions, each list ascending and gathering its point
    pcnt, poff, plist = (t.long() for t in (want["pcnt"], want["poff"], want["plist"]))
    assert sorted(plist.tolist()) == list(range(B * N * K)) and int(pcnt.sum()) == B * N * K
    owner = torch.repeat_interleave(torch.arange(B * N), pcnt)
    assert torch.equal(C.targets(idx)[plist], owner)
    same = owner[1:] == owner[:-1]
    assert bool((plist[1:][same] > plist[:-1][same]).all())


def test_csr_only_cases_have_the_scan_depths_and_the_reference_partitions_them():
    for B, N, K in C.CSR_ONLY:
        idx = C.outside_graph(B, N, K, torch.Generator().manual_seed(N))
        pcnt, poff, plist = C.csr(idx)
        assert int(pcnt.sum()) == B * N * K and torch.equal(poff.long(), torch.cumsum(pcnt.long(), 0) - pcnt)
        assert torch.equal(C.targets(idx)[plist.long()], torch.repeat_interleave(torch.arange(B * N), pcnt.long()))


def test_row_counts_of_the_library_equal_the_reference():
    """apn_ec_pool_rows / apn_ec_bwd_prep_rows (host code) against the reference's row counts, for every case."""
    from adaptpoint_amd import _lib
    lib = _lib.load()
    shapes = {(c.B, c.N) for c in C.CASES} | {(c.B, c.N) for c in C.FLOAT} | {(b, n) for b, n, _ in C.CSR_ONLY}
    for B, N in sorted(shapes):
        assert lib.apn_ec_pool_rows(B, N) == (B * N + C.QPB - 1) // C.QPB
        assert lib.apn_ec_bwd_prep_rows(B, N) == B * ((N + C.TILE - 1) // C.TILE)
    for c in C.CASES[::7]:
        want = C.expected(c, C.exact_inputs(c))
        assert want["part"].shape[0] == lib.apn_ec_pool_rows(c.B, c.N)
        assert want["partS"].shape[0] == lib.apn_ec_bwd_prep_rows(c.B, c.N)
    assert lib.apn_ec_pool_rows(0, 5) == 0 and lib.apn_ec_bwd_prep_rows(5, 0) == 0


@pytest.mark.parametrize("case", C.FLOAT[:3] + C.FLOAT[-1:], ids=C.FLOAT_IDS[:3] + C.FLOAT_IDS[-1:])
def test_float32_restatement_and_bars_on_the_cpu(case):
    """The float32 restatement stays within the derived bars of float64 (it has the kernels' roundings, in another
    grouping of partS's sums), and its fixed-order sum is what it claims: the eval-mode dv equals adding each list in
    ascending position, one float32 add per entry."""
    H, K = case.H, case.K
    inp = C.float_inputs(case)
    F32 = torch.float32
    ext, sel, ysum, p1, p2 = C.pool_fwd(inp["uv"], H, inp["idx"], inp["gamma"], dtype=F32)
    e64, s64, y64, q1, q2 = C.pool_fwd(inp["uv"], H, inp["idx"], inp["gamma"])
    assert ext.dtype == F32 and torch.equal(ext, e64.float())         # rounding is monotone: the extremum of the rounded sums
    gsel, partS = C.bwd_prep(inp["g"], ext, inp["pack"], inp["slope"], dtype=F32)
    de = C.float_dense(inp, partS)
    bars = C.float_bars(H, K, inp["idx"], inp["uv"], inp["pack"], inp["slope"], inp["res"], inp["g"], ext, gsel, sel, ysum, de)
    g64, pS64 = C.bwd_prep(inp["g"], ext, inp["pack"], inp["slope"])
    o32, o64 = (C.out(ext, inp["pack"], inp["slope"], inp["res"], dtype=d) for d in (F32, F64))
    duv64 = C.pool_bwd(gsel, sel, inp["idx"], inp["uv"], H, ysum, de)
    duv32 = C.pool_bwd(gsel, sel, inp["idx"], inp["uv"], H, ysum, de, dtype=F32)
    n32, n64 = (C.out(ext, inp["pack"], inp["slope"], None, dtype=d) for d in (F32, F64))
    for name, got, ref in (("out", o32, o64), ("out_nores", n32, n64), ("gsel", gsel, g64), ("partS", partS, pS64),
                           ("duv", duv32, duv64)):
        ratio = float(((got.double() - ref).abs() / bars[name].clamp_min(1e-300)).max())
        print(f"{case.name} {name}: float32 restatement / bar {ratio:.3f}")
        assert ratio <= 1.0, (name, ratio)
    # the eval-mode dv, list by list in ascending position
    ev = C.pool_bwd(gsel, sel, inp["idx"], inp["uv"], H, None, torch.zeros(2 * H), dtype=F32)
    assert torch.equal(ev[..., :H], gsel)
    B, N = case.B, case.N
    pcnt, poff, plist = (t.tolist() for t in C.csr(inp["idx"]))
    for pt in range(0, B * N, 17):
        acc = torch.zeros(H)
        for pos in plist[poff[pt]:poff[pt] + pcnt[pt]]:
            q, slot = divmod(pos, K)
            acc = acc + torch.where(sel.reshape(B * N, H)[q] == slot, gsel.reshape(B * N, H)[q], torch.zeros(()))
        assert torch.equal(acc, ev.reshape(B * N, 2 * H)[pt, H:])
