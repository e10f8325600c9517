"""The case table of tests/sa_wide_cases.py on the CPU: every (case, width) meets the exactness and the non-vacuity
conditions, the statement's own notion of a query's rows is the tile map's, the blob helper lays the map out as the kernels
read it, every mutated statement differs from the true one somewhere in the table, and the float case's gap rule leaves
out at most 1 % of the pooled values on the float64 statement alone."""
import functools

import numpy as np
import pytest
import torch

import sa_wide_cases as C


@functools.lru_cache(maxsize=6)           # (the small cases stay for the tests that share them; the large ones go)
def _checked(name, H):
    return C.inputs(name, H)


@pytest.mark.parametrize("name,H", C.PAIRS)
def test_every_case_is_exact_and_telling(name, H):
    inp, fwd, bwd, bwd0 = _checked(name, H)            # (raises where a condition fails)
    assert fwd["ksel"].dtype == torch.uint8 and bwd["GU"].shape == (int(C.layout(name)["rep"].sum()), H)
    # without evec the Qm and evec terms are absent: another statement wherever a row with an open gate has them
    assert not torch.equal(bwd["GU"], bwd0["GU"]) and torch.equal(bwd["HB"], bwd0["HB"]) and torch.equal(bwd["R"], bwd0["R"])
    # every value the kernels are handed, and every value they return, is a float32 (the sums: float64 sums of such)
    for k in ("U", "V", "pack1", "W2", "Qm", "evec", "goa"):
        assert np.array_equal(inp[k].astype(np.float32).astype(np.float64), inp[k]), k
    for t in (fwd["ysel"], bwd["GU"], bwd["HA"], bwd["HB"]):
        assert torch.equal(t.float().double(), t)


def test_the_table_ties_across_the_lane_halves_both_ways():
    """Ties whose candidates sit in different lane halves of the accumulator, the lower slot in the UPPER half and the
    reverse -- in the case whose tiles hold several queries, at every width."""
    for H in C.WIDTHS:
        fwd = _checked("mixed", H)[1]
        assert fwd["lower_in_upper"] > 0 and fwd["lower_in_lower"] > 0, H


def test_the_generator_raises_on_a_case_that_is_not_exact_or_tells_nothing():
    inp, fwd, bwd, _ = _checked("mixed", 32)
    for change in (dict(W2=inp["W2"] * 256), dict(ksel=np.full_like(inp["ksel"], 31))):
        with pytest.raises(ValueError):
            C.check_exact(dict(inp, **change), fwd, bwd)
    big = dict(inp, goa=inp["goa"] * 2.0 ** 12)
    with pytest.raises(ValueError):
        C.check_exact(big, fwd, C.backward(big, telling=True))
    with pytest.raises(ValueError):
        C.check_telling(dict(inp, sgn2=np.ones_like(inp["sgn2"])), fwd)
    flat = dict(inp, U=np.zeros_like(inp["U"]), V=np.zeros_like(inp["V"]))
    with pytest.raises(ValueError):
        C.check_telling(flat, C.forward(flat, telling=True))


@pytest.mark.parametrize("name", list(C.CASES))
def test_the_rows_of_the_statement_are_the_rows_of_the_tile_map(name):
    """`position_slots` (written from the definition of a ball-query row) against `oracle.tile_map`: every query's live
    rows are its slots in ascending order, consecutive within ONE tile, each gathering idx[q, slot] with the number of the
    slot's positions as multiplicity; the queries of a tile are consecutive and of one cloud; padding rows carry 0xff."""
    c, lay = C.CASES[name], C.layout(name)
    tm, idx = lay["tm"], lay["idx"].reshape(-1, 32)
    seen = {}
    for t in range(tm["nt"]):
        live = 0
        for r in range(32):
            info = int(tm["rowinfo"][t, r])
            if r == 0:
                nq, info = info >> 24, info & 0xffffff
            if (info >> 16) & 0xff == 0:
                assert info == 0xff
                continue
            q = int(tm["tq0"][t]) + (info & 0xff)
            assert q // c["M"] == int(tm["tq0"][t]) // c["M"] and (info & 0xff) < nq
            seen.setdefault(q, []).append((t, r, (info >> 8) & 0xff, (info >> 16) & 0xff, int(tm["rownn"][t, r])))
            live += 1
        assert live > 0
    assert sorted(seen) == list(range(c["B"] * c["M"]))
    for q, rows in seen.items():
        slots = np.flatnonzero(lay["rep"][q])
        assert [s for _, _, s, _, _ in rows] == list(slots)
        assert len({t for t, _, _, _, _ in rows}) == 1 and [r for _, r, _, _, _ in rows] == list(rows[0][1] + slots)
        assert (rows[0][0], rows[0][1]) == (lay["tile"][q], lay["row0"][q])
        assert [m for _, _, _, m, _ in rows] == list(lay["mult"][q][slots])
        assert [n for _, _, _, _, n in rows] == list(idx[q][slots])
        assert np.array_equal(idx[q], idx[q][lay["slot"][q]])            # every position gathers its row's point
    if name == "mixed":             # the kinds the case was built for
        per_q = lay["nslots"].reshape(c["B"], c["M"])
        for q in range(c["M"]):
            assert per_q[0, q] == (C.MIXED_KINDS[q % 6] or 32)
        nqs = tm["rowinfo"][:, 0] >> 24
        assert (nqs == 1).any() and (nqs > 1).any() and len(lay["pad"])
        assert (tm["nt"] + 3) // 4 < (c["B"] * c["M"] + 3) // 4 - 4          # (whole workgroups without a tile)
    if name == "rounds":
        assert tm["nt"] == 2200 and tm["nt"] - 2048 == 152
    if name == "rounds_folded":
        assert tm["nt"] == 550 and (lay["nslots"] == 8).all()
    if name == "whole":
        assert tm["nt"] == 66 and tm["nt"] % 4
    if name == "one":
        assert tm["nt"] == 1 and len(lay["pad"]) == 31 and lay["mult"][0, 0] == 32


@pytest.mark.parametrize("name", list(C.CASES))
def test_the_blob_is_the_tile_map_field_by_field(name):
    c, lay = C.CASES[name], C.layout(name)
    tm, blob, bm = lay["tm"], lay["blob"], c["B"] * c["M"]
    nt = tm["nt"]
    rows_off = 4 + ((bm + 3) & ~3)
    assert blob.dtype == np.int32 and blob.size == rows_off + 64 * bm and rows_off % 4 == 0
    assert blob[0] == nt and not blob[1:4].any()
    assert np.array_equal(blob[4:4 + nt], tm["tq0"]) and not blob[4 + nt:rows_off].any()
    rowinfo = blob[rows_off:rows_off + 32 * bm].view(np.uint32).reshape(bm, 32)
    rownn = blob[rows_off + 32 * bm:].reshape(bm, 32)
    assert np.array_equal(rowinfo[:nt], tm["rowinfo"]) and not rowinfo[nt:].any()
    assert np.array_equal(rownn[:nt], tm["rownn"]) and not rownn[nt:].any()
    # the accessors of the kernels: qlocal | slot << 8 | mult << 16 (| queries << 24 in row 0)
    t, r = nt - 1, 0
    info = int(rowinfo[t, r])
    assert (info >> 24) >= 1 and (info >> 16) & 0xff >= 1 and (info >> 8) & 0xff == 0 and info & 0xff == 0


SMALL = [("one", 32), ("mixed", 32), ("whole", 32), ("mixed", 128)]


@pytest.mark.parametrize("mutation", C.MUTATIONS)
def test_every_mutated_statement_differs_from_the_true_one(mutation):
    """highest-slot tie rule; lane-half-order tie rule (the candidate in the lower half wins); statistics without the
    multiplicity; padding rows counted; cloud 0's rows of U for every cloud; ksel as the row's place in its TILE instead of
    its slot; evec not multiplied by the multiplicity; the Gram matrix without it."""
    where = {}
    for name, H in SMALL:
        inp = _checked(name, H)[0]
        f0, b0 = _checked(name, H)[1], _checked(name, H)[2]
        f1, b1 = C.forward(inp, mutate=mutation), C.backward(inp, mutate=mutation)
        diff = [k for k in ("stats1", "stats2", "ysel", "ksel") if not torch.equal(f0[k], f1[k])]
        diff += [k for k in ("GU", "T", "HA", "HB", "R") if not torch.equal(b0[k], b1[k])]
        if diff:
            where[(name, H)] = diff
    assert where, mutation
    expect = dict(tie_highest="ksel", tie_lower_half="ksel", stats_no_mult="stats2", padding_counted="stats1", cloud0="ysel",
                  ksel_row_in_tile="ksel", evec_no_mult="GU", gram_no_mult="R")[mutation]
    assert any(expect in d for d in where.values()), (mutation, where)


@pytest.mark.parametrize("H", C.WIDTHS)
def test_the_float_case_leaves_out_at_most_one_percent_by_the_float64_statement_alone(H):
    inp = C.float_inputs(H, C.FLOAT_SEED)
    y2bar, statbar = C.float_bars(inp, "cpu")
    ysel, ksel, bar, sure = C.float_pool(inp, "cpu", y2bar)
    assert 1.0 - sure.double().mean().item() <= 0.01
    assert bool((bar > 0).all()) and bool((statbar > 0).all()) and bool(torch.isfinite(ysel).all())
    # N(0,1) operands: their lo parts are not zero (the split-operand path has something to lose)
    assert (inp["W2"] != torch.from_numpy(inp["W2"]).bfloat16().double().numpy()).mean() > 0.9
