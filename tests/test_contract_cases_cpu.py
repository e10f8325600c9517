"""The raw-contraction case table (tests/contract_cases.py) checked against its own purpose, without a GPU: every loader
class x layout form is reached, the split-K cases are split by the library the way they are meant to be, the reference
helper is a matrix product, and the exact-input generator is exact under the kernel's arithmetic."""
import pytest
import torch

import contract_cases as CC


def test_every_loader_class_and_layout_form_is_in_the_table():
    """Every (layout form x loader class) -- each run at precision 2 and 3 by test_gpu_contract.py --, both grids
    (renumbered / plain) per form, and the causes of the value-by-value loads one by one."""
    seen = {(CC.form_of(c), CC.loader_class(c, CC.synthetic_ptrs(c))) for c in CC.CASES}
    for form in CC.FORMS:
        for cls in CC.CLASSES:
            assert (CC._form_name(form), cls) in seen, (form, cls)
    for form in CC.FORMS:
        mine = [c for c in CC.CASES if (c.a_kcont, c.b_kcont) == form]
        direct = [c for c in mine if not c.reduce]
        scalar = [c for c in mine if CC.loader_class(c, CC.synthetic_ptrs(c)) == "scalar"]
        assert {1, 2, 3} <= {c.a_off % 4 for c in scalar} and {1, 2, 3} <= {c.b_off % 4 for c in scalar}
        assert any(c.a_pad % 2 and c.b_pad % 2 for c in scalar), "odd leading dimensions"
        assert any(c.nbatch > 1 and CC.geometry(c)[0][0] % 2 and CC.geometry(c)[1][0] % 2 for c in scalar), "odd batch strides"
        if not (form[0] and form[1]):
            assert any(c.K % 32 == 0 and (c.R % 4 if not form[0] else c.Q % 4) and not (c.a_off or c.b_off or c.a_pad or c.b_pad)
                       for c in mine), "a row-contiguous operand whose rows are not whole quads"
        # K a multiple of 32 with exactly one operand float4-readable
        assert any(c.K % 32 == 0 and CC.loader_class(c, CC.synthetic_ptrs(c)) == "general4" for c in mine)
        assert any(c.K % 4 == 0 and c.K % 32 and CC.loader_class(c, CC.synthetic_ptrs(c)) == "general4" for c in mine)
        for nb in (1, 3, 8, 16):
            assert any(c.nbatch == nb and CC.grid(c)[0] * CC.grid(c)[1] > 1 for c in direct), (form, nb)
        assert any(c.nbatch == 8 and CC.grid(c)[0] > 1 and CC.grid(c)[1] > 1 for c in direct)
        assert {CC.grid(c)[3] for c in direct} == {True, False}, "renumbered and plain grids"
        assert {c.R for c in mine} >= set(CC.R_VALUES) and {c.Q for c in mine} >= set(CC.Q_VALUES)
        assert {c.K for c in mine} >= set(CC.K_VALUES)
        assert any(c.a_batch == "shared" for c in mine) and any(c.b_batch == "shared" for c in mine)
        assert any(c.d_pad for c in direct) and any(c.d_gap and c.nbatch > 1 for c in direct)
    assert len(set(CC.CASE_IDS)) == len(CC.CASES)
    cov = CC.coverage()
    want = [(CC._form_name(f), cls, planes) for f in CC.FORMS for cls in CC.CLASSES for planes in (2, 3)]
    want += [(CC._form_name(f), tag) for f in CC.FORMS
             for tag in ("renumbered grid", "plain grid", "split-empty", "split-straddle", "split-renumbered")]
    want += [("fold", "col_sums_kernel"),("fold", "pw_fold2_kernel"), ("pair", "direct")]
    for key in want:
        assert cov[key], key


def test_exact_ranges_keep_two_planes_and_stay_below_2_24():
    for c in CC.CASES:
        W = CC.exact_range(c)
        assert W >= 256, (c.name, W)                               # more than bf16's 8 bits: the second plane is not zero
        assert W * CC.NARROW * CC.contracted(c) < 2 ** 24, c.name


def test_split_cases_are_split_as_they_are_meant_to_be():
    """From the library's own `apn_pw_contract_splits`: trailing empty shares, shares that straddle batch entries in the
    steady-state form, a share count that engages the tile renumbering -- so that a later change of the split rule cannot
    silently empty these cases of their purpose."""
    from adaptpoint_amd import _lib
    lib = _lib.load()
    plan = {}
    for c in CC.CASES:
        if c.reduce:
            s = lib.apn_pw_contract_splits(c.nbatch, c.R, c.Q, c.K)
            assert 1 <= s <= 256
            plan[c.name] = (s,) + CC.split_plan(c.nbatch, c.K, s) + (CC.loader_class(c, CC.synthetic_ptrs(c)), CC.grid(c, s)[3])
    for form in CC.FORMS:
        fn = CC._form_name(form)
        assert plan[f"{fn}-split-empty4"][:3] == (4, 3, 1)         # 9 chunks in 4 shares of 3: the fourth empty
        assert plan[f"{fn}-split-empty7"][:3] == (7, 3, 2)         # 15 chunks in 7 shares of 3: two empty
        s, cps, empty, straddling, cls, _ = plan[f"{fn}-split-straddle"]
        assert (s, cps, empty) == (10, 2, 0) and straddling >= 2 and cls == "steady"
        s, cps, empty, straddling, cls, _ = plan[f"{fn}-split-straddle-general"]
        assert straddling >= 1 and cls != "steady"
        assert plan[f"{fn}-split-renumbered"][0] == 8 and plan[f"{fn}-split-renumbered"][5]
        assert not plan[f"{fn}-split-empty4"][5]
    assert any(p[2] for p in plan.values()) and any(p[3] for p in plan.values())


@pytest.mark.parametrize("name", ["rr-sizes2", "kr-scalar-off31", "rk-split-empty7"])
def test_reference_is_the_naive_triple_loop(name):
    """`reference` on the strided views of the poisoned parents against three nested loops over the logical values."""
    c = CC.CASES[CC.CASE_IDS.index(name)]
    c = c._replace(R=min(c.R, 5), Q=min(c.Q, 4), K=min(c.K, 6))
    gen = torch.Generator().manual_seed(7)
    av, bv = CC.exact_inputs(c, True, gen)
    (a, sa, lda), (b, sb, ldb) = CC.operands(c, av, bv)
    assert (sa, lda) == CC.geometry(c)[0] and (sb, ldb) == CC.geometry(c)[1]
    want = torch.zeros(1 if c.reduce else c.nbatch, c.R, c.Q, dtype=torch.int64)
    for z in range(c.nbatch):
        for i in range(c.R):
            for j in range(c.Q):
                for k in range(c.K):
                    want[0 if c.reduce else z, i, j] += int(av[z % av.shape[0], i, k]) * int(bv[z % bv.shape[0], j, k])
    assert torch.equal(CC.reference(c, a, b, torch.int64), want)
    assert torch.equal(CC.reference(c, a, b), want.double())
    # the views address the parent as the kernel's operand description does
    parent = a._base if a._base is not None else a
    for (z, i, k) in [(0, 0, 0), (c.nbatch - 1, c.R - 1, c.K - 1)]:
        at = CC.LEAD + c.a_off + z * sa + (i * lda + k if c.a_kcont else k * lda + i)
        assert float(parent[at]) == float(av[z % av.shape[0], i, k])
    assert int(torch.isnan(parent).sum()) == parent.numel() - av.numel()


def test_output_buffer_masks_exactly_the_result():
    c = CC.CASES[CC.CASE_IDS.index("kk-sizes1")]._replace(nbatch=3, R=5, Q=4, d_pad=5, d_gap=7)
    view, parent, mask = CC.output(c, "cpu")
    (d_batch, ldd) = CC.geometry(c)[2]
    assert ldd > c.Q and d_batch > c.R * ldd
    assert int(mask.sum()) == 3 * 5 * 4 and not mask[:CC.LEAD].any() and not mask[-CC.LEAD:].any()
    view.fill_(1.0)
    assert bool((parent[~mask] == CC.SENTINEL).all()) and bool((parent[mask] != CC.SENTINEL).all())


@pytest.mark.parametrize("planes", [2, 3])
@pytest.mark.parametrize("wide_a", [True, False])
@pytest.mark.parametrize("K", [33, 1100, 1536, 4096])
def test_exact_inputs_are_exact_under_the_kernels_arithmetic(planes, wide_a, K):
    """The kernel's arithmetic emulated in torch (bf16 planes by repeated rounding and subtraction, the plane products
    the kernel keeps, float32 accumulation) on the exact-input generator's operands: the wide operand is two planes, the
    narrow one a single plane, and the float32 result EQUALS the int64 product."""
    c = CC._case("emulated", 1, 37, 29, K, (True, True))
    gen = torch.Generator().manual_seed(K + planes)
    a, b = CC.exact_inputs(c, wide_a, gen)
    a, b = a[0], b[0]
    wide, narrow = (a, b) if wide_a else (b, a)
    pw, rem_w = CC.bf16_planes(wide, 2)
    pn, rem_n = CC.bf16_planes(narrow, 1)
    assert not rem_w.any() and not rem_n.any() and pw[1].any()
    assert float((a.abs().double() @ b.abs().double().t()).max()) < 2 ** 24
    got = CC.emulate(a, b, planes)
    assert torch.equal(got.to(torch.int64), a.to(torch.int64) @ b.to(torch.int64).t())
    assert torch.equal(got, got.round())


def test_emulation_of_float_inputs_meets_the_derived_bound():
    """The element-wise bar of test_gpu_contract.py on the emulated arithmetic: |d - ref| <= (c_p + (K + 6) 2^-24) |a| @ |b|."""
    for planes, cp in ((2, 3 * 2.0 ** -16), (3, 2.0 ** -22)):
        for K in (31, 160, 1536):
            gen = torch.Generator().manual_seed(K)
            a = torch.randn(40, K, generator=gen) * torch.exp2(torch.randint(-12, 13, (40, K), generator=gen).float())
            b = torch.randn(24, K, generator=gen)
            ref = a.double() @ b.double().t()
            bound = (cp + (K + 6) * 2.0 ** -24) * (a.abs().double() @ b.abs().double().t())
            assert bool(((CC.emulate(a, b, planes).double() - ref).abs() <= bound).all())
