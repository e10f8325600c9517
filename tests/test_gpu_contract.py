"""The contraction kernel of csrc/pointwise.hip (`pw_gemm_body`) through its raw-operand entries -- `pointwise.contract`
(apn_pw_contract) and `propagation._contract2` (apn_pw_contract2) -- on the problems of tests/contract_cases.py: every
layout form x loader class x precision, tile edges, moved origins, padded leading dimensions, shared and oddly strided
batches, the XCD tile renumbering, split-K with empty and straddling shares, outputs that are blocks of wider buffers.

Four kinds of check:
  exact       integer inputs for which every partial sum is an integer below 2^24: the result must EQUAL the int64 product;
  float64     Gaussian and random-binade inputs against float64, an element-wise bar derived from the arithmetic and the
              project's relative-L2 bars;
  containment every operand lies in a NaN-filled parent and every output in a sentinel-filled one: no NaN may come out,
              no sentinel may change;
  invariants  results that must agree bit for bit (layout forms, loaders, batching, power-of-two scaling, the pair launch).
"""
import pytest
import torch

import contract_cases as CC

pytestmark = pytest.mark.gpu

# planes per operand -> relative L2 against float64: tests/test_gpu_pointwise.py's TOL out-bars.  Measured on an MI355X,
# worst over this file (Gaussian and random-binade inputs): 1.4e-5 with two planes (a 1 x 4 result: few elements to average over),
# 4.4e-7 with three.
TOL_L2 = {2: 3e-5, 3: 2e-6}
# element-wise: |d - ref| <= (C_P + (terms + 6) 2^-24) (|a| @ |b|).  Two planes keep 16 bits of each operand (truncation
# <= 2^-16 each) and drop lo * lo (<= 2^-16): 3 * 2^-16 = 4.6e-5; three planes hold all 24 bits and drop plane products of
# <= 2 * 2^-24 + 2^-32: 2^-22 = 2.4e-7.  The second summand is the worst-case float32 accumulation of the terms (+ the
# fold and the final rounding).  Measured worst |d - ref| / (|a| @ |b|) over this file: 2.6e-5 with two planes,
# 8.7e-7 with three (at K = 1536, where the bar is 9.2e-5).
C_P = {2: 3 * 2.0 ** -16, 3: 2.0 ** -22}
WORST = {2: [0.0, 0.0, "", ""], 3: [0.0, 0.0, "", ""]}         # planes -> [element-wise ratio, relative L2, case, case]


def _planes(monkeypatch, planes):
    from adaptpoint_amd import pointwise
    monkeypatch.setattr(pointwise, "PRECISION", planes)


def _run(case, av, bv):
    """The case on the logical operand values -> (result view, output parent, its mask, a view, b view)."""
    from adaptpoint_amd import pointwise
    (a, sa, lda), (b, sb, ldb) = CC.operands(case, av, bv)
    d, parent, mask = CC.output(case, av.device)
    (d_batch, ldd) = CC.geometry(case)[2]
    pointwise.contract(case.nbatch, case.R, case.Q, case.K, a, sa, lda, case.a_kcont, b, sb, ldb, case.b_kcont, d,
                       d_batch=d_batch, ldd=ldd, reduce=case.reduce)
    return d, parent, mask, a, b


def _contained(d, parent, mask):
    """No poison came in, nothing but the result was written."""
    assert not bool(torch.isnan(d).any()), "a NaN from outside the operands reached the result"
    assert bool((parent[~mask] == CC.SENTINEL).all()), "an element outside the result was written"


def _result(case, av, bv):
    d, parent, mask, _, _ = _run(case, av, bv)
    _contained(d, parent, mask)
    return d.clone()


def _float_bars(case, planes, d, a, b, label):
    ref = CC.reference(case, a, b)
    mag = CC.reference(case, a.abs(), b.abs())
    err = (d.double() - ref).abs()
    bar = C_P[planes] + (CC.contracted(case) + 6) * 2.0 ** -24
    ratio = float((err / mag.clamp_min(1e-300)).max())
    l2 = float(err.norm() / ref.norm().clamp_min(1e-300))
    w = WORST[planes]
    if ratio > w[0]:
        w[0], w[2] = ratio, label
    if l2 > w[1]:
        w[1], w[3] = l2, label
    print(f"{label} planes {planes}: element-wise {ratio:.3e} (bar {bar:.3e}), relative L2 {l2:.3e} (bar {TOL_L2[planes]:.0e})")
    assert bool((err <= bar * mag).all()), (label, planes, ratio, bar)
    assert l2 < TOL_L2[planes], (label, planes, l2)


@pytest.mark.parametrize("case", CC.CASES, ids=CC.CASE_IDS)
def test_integer_inputs_give_the_integer_product(dev, case, monkeypatch):
    """Exact: one operand in [-2047, 2047] (two bf16 planes), the other in [-7, 7] (one), either way round, both
    precisions.  The result equals the int64 reference -- no tolerance: one wrong, missing or doubled element anywhere
    shows.  Also: the loader class the table claims for the case is the one the real addresses give."""
    gen = torch.Generator(dev).manual_seed(len(case.name) + case.R + 7 * case.Q + 13 * case.K)
    for wide_a in (True, False):
        av, bv = CC.exact_inputs(case, wide_a, gen, dev)
        want = None
        for planes in (2, 3):
            _planes(monkeypatch, planes)
            d, parent, mask, a, b = _run(case, av, bv)
            assert CC.loader_class(case, (a.data_ptr(), b.data_ptr())) == CC.loader_class(case, CC.synthetic_ptrs(case))
            if want is None:
                want = CC.reference(case, a, b, torch.int64)
                assert int(CC.reference(case, a.abs(), b.abs(), torch.float64).max()) < 2 ** 24
            _contained(d, parent, mask)
            got = d.cpu()
            assert torch.equal(got.to(torch.int64), want) and torch.equal(got, got.round()), (case.name, wide_a, planes)


@pytest.mark.parametrize("case", CC.CASES, ids=CC.CASE_IDS)
def test_float_inputs_against_float64(dev, case, monkeypatch):
    """Gaussian inputs and inputs with per-element random binades against the float64 product of the same strided
    views: the derived element-wise bar and the project's relative-L2 bar, both precisions."""
    gen = torch.Generator(dev).manual_seed(case.R + 3 * case.Q + 5 * case.K + case.nbatch)
    for binades in (False, True):
        av, bv = CC.float_inputs(case, binades, gen, dev)
        for planes in (2, 3):
            _planes(monkeypatch, planes)
            d, parent, mask, a, b = _run(case, av, bv)
            _contained(d, parent, mask)
            _float_bars(case, planes, d, a, b, f"{case.name}{'-binades' if binades else ''}")


@pytest.mark.parametrize("case", [c for c in CC.CASES if c.reduce], ids=[c.name for c in CC.CASES if c.reduce])
@pytest.mark.parametrize("planes", [2, 3])
def test_split_k_is_bit_reproducible(dev, case, planes, monkeypatch):
    _planes(monkeypatch, planes)
    gen = torch.Generator(dev).manual_seed(11)
    av, bv = CC.float_inputs(case, True, gen, dev)
    assert torch.equal(_result(case, av, bv), _result(case, av, bv))


# ---- bit-level invariants -----------------------------------------------------------------------------------------------

def _logical(dev, nbatch, R, Q, K, seed, binades=True):
    gen = torch.Generator(dev).manual_seed(seed)
    c = CC._case("values", nbatch, R, Q, K, (True, True))
    return CC.float_inputs(c, binades, gen, dev)


@pytest.mark.parametrize("shape", [(2, 132, 68, 64), (1, 130, 67, 100), (3, 64, 260, 33), (1, 128, 128, 1536)],
                         ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("planes", [2, 3])
def test_layout_forms_and_loaders_agree_bit_for_bit(dev, shape, planes, monkeypatch):
    """The same matrices in the four layout forms (transposed copies), with aligned and moved origins, tight and padded
    leading dimensions: the bf16 planes and the chunking of K do not depend on where a value was loaded from, so the
    steady-state, general-float4 and value-by-value loaders (PwLoader::stage_fast / stage) and both fragment reads
    (pw_fragment: direct and transposed) give identical results."""
    _planes(monkeypatch, planes)
    nb, R, Q, K = shape
    av, bv = _logical(dev, nb, R, Q, K, seed=R + K)
    first, classes = None, set()
    for form in CC.FORMS:
        for kw in (dict(), dict(a_off=1, b_off=2), dict(a_pad=4, b_pad=8, a_off=4), dict(a_pad=1, b_pad=3), dict(a_batch=3, b_batch=5)):
            c = CC._case("form", nb, R, Q, K, form, **kw)
            classes.add(CC.loader_class(c, CC.synthetic_ptrs(c)))
            got = _result(c, av, bv)
            if first is None:
                first = got
            assert torch.equal(got, first), (form, kw, float((got - first).abs().max()))
    assert "scalar" in classes and len(classes) >= 2


@pytest.mark.parametrize("form", CC.FORMS, ids=CC._form_name)
@pytest.mark.parametrize("planes", [2, 3])
def test_batched_call_equals_one_call_per_entry_and_shared_equals_expanded(dev, form, planes, monkeypatch):
    """nbatch = 8 (tiles renumbered) and 3 (not): entry z of the batched result == the call on entry z alone; an operand
    shared through a batch stride of 0 == the same operand repeated."""
    _planes(monkeypatch, planes)
    for nb, R, Q, K in [(8, 132, 260, 64), (3, 130, 129, 33), (16, 4, 132, 32)]:
        av, bv = _logical(dev, nb, R, Q, K, seed=nb + K)
        whole = _result(CC._case("batched", nb, R, Q, K, form, d_pad=1, d_gap=3), av, bv)
        for z in range(nb):
            one = _result(CC._case("single", 1, R, Q, K, form), av[z:z + 1], bv[z:z + 1])
            assert torch.equal(whole[z], one[0]), (nb, z)
        for share_a in (True, False):
            sa, sb = (av[:1], bv) if share_a else (av, bv[:1])
            kw = dict(a_batch="shared") if share_a else dict(b_batch="shared")
            shared = _result(CC._case("shared", nb, R, Q, K, form, **kw), sa, sb)
            full = _result(CC._case("expanded", nb, R, Q, K, form), sa.expand(nb, -1, -1).contiguous(),
                           sb.expand(nb, -1, -1).contiguous())
            assert torch.equal(shared, full)


@pytest.mark.parametrize("form", CC.FORMS, ids=CC._form_name)
@pytest.mark.parametrize("planes", [2, 3])
def test_power_of_two_scaling_is_exact(dev, form, planes, monkeypatch):
    """A * 2^s gives 2^s * result: scaling by a power of two is exact in every bf16 plane and in every sum (no
    underflow or overflow at these magnitudes)."""
    _planes(monkeypatch, planes)
    for reduce, (nb, R, Q, K) in [(False, (2, 130, 67, 100)), (False, (1, 64, 132, 96)), (True, (4, 64, 64, 160))]:
        av, bv = _logical(dev, nb, R, Q, K, seed=K, binades=False)
        c = CC._case("scaled", nb, R, Q, K, form, reduce=reduce)
        base = _result(c, av, bv)
        for s in (-40, -7, 9, 40):
            assert torch.equal(_result(c, av * 2.0 ** s, bv), base * 2.0 ** s), s
            assert torch.equal(_result(c, av, bv * 2.0 ** s), base * 2.0 ** s), s


# ---- the pair launch (apn_pw_contract2) -------------------------------------------------------------------------------

def _problem(case, a, b, d_ptr, d_batch, ldd):
    (av, sa, lda), (bv, sb, ldb) = a, b
    return (case.nbatch, case.R, case.Q, case.K, av.data_ptr(), sa, lda, bv.data_ptr(), sb, ldb, d_ptr, d_batch, ldd)


PAIRS = CC.PAIRS


@pytest.mark.parametrize("name", list(PAIRS))
@pytest.mark.parametrize("planes", [2, 3])
def test_pair_launch_equals_two_single_launches(dev, name, planes, monkeypatch):
    """Direct form: contract2(p0, p1) == contract(p0), contract(p1) bit for bit (the workgroup index picks the problem,
    everything after that is the same body), the pair given both ways round so that the internal "longer loop first"
    swap happens in one of them; nothing outside the two results is written."""
    from adaptpoint_amd.propagation import _contract2
    _planes(monkeypatch, planes)
    pair = PAIRS[name]
    gen = torch.Generator(dev).manual_seed(5)
    values = [CC.float_inputs(c, True, gen, dev) for c in pair]
    singles = [_result(c, *v) for c, v in zip(pair, values)]
    chunks = [(c.K + 31) // 32 for c in pair]
    for order in ((0, 1), (1, 0)):
        probs, outs = [], []
        for p in order:
            c = pair[p]
            a, b = CC.operands(c, *values[p])
            d, parent, mask = CC.output(c, dev)
            (d_batch, ldd) = CC.geometry(c)[2]
            probs.append(_problem(c, a, b, d.data_ptr(), d_batch, ldd))
            outs.append((d, parent, mask, a, b))
        _contract2(dev, pair[0].a_kcont, pair[0].b_kcont, probs)
        for p, (d, parent, mask, _, _) in zip(order, outs):
            _contained(d, parent, mask)
            assert torch.equal(d, singles[p]), (order, p)
    # (where the problems' loops differ in length, one of the two orders was swapped inside)
    assert name in ("grad-input-35+29", "eight-entries-kk") or chunks[0] != chunks[1]


@pytest.mark.parametrize("planes", [2, 3])
@pytest.mark.parametrize("shape", CC.PAIR_BLOCKS, ids=lambda s: f"{s[2]}+{s[3]}")
def test_pair_results_as_column_blocks_of_one_matrix(dev, shape, planes, monkeypatch):
    """gW[:, :C1] | gW[:, C1:] of the hoisted block: two results written with ldd = C1 + C2 (+ padding) into one
    matrix leave each other's columns and the padding alone -- the direct form (one batch entry: equal to the single
    launches bit for bit) and the split form through pw_fold2_kernel (integer inputs: equal to the int64 product;
    float inputs: within the bars, identical from run to run; the scratch buffers' surroundings untouched)."""
    from adaptpoint_amd import _lib
    from adaptpoint_amd.propagation import _contract2
    _planes(monkeypatch, planes)
    lib = _lib.load()
    B, O, C1, C2, n, m = shape
    C, ldd = C1 + C2, C1 + C2 + 3

    def launch(cases, values, splits):
        ops = [CC.operands(c, *v) for c, v in zip(cases, values)]
        parent = torch.full((2 * CC.LEAD + O * ldd,), CC.SENTINEL, dtype=torch.int32, device=dev)
        D = parent.view(torch.float32).as_strided((O, ldd), (ldd, 1), CC.LEAD)
        probs = [_problem(cases[0], *ops[0], D.data_ptr(), 0, ldd), _problem(cases[1], *ops[1], D.data_ptr() + 4 * C1, 0, ldd)]
        scratch = None
        if splits:
            sizes = [s * O * q for s, q in zip(splits, (C1, C2))]
            scratch = [torch.full((2 * CC.LEAD + sz,), CC.SENTINEL, dtype=torch.int32, device=dev) for sz in sizes]
            _contract2(dev, True, True, probs, splits=splits, scratch=tuple(s.data_ptr() + 4 * CC.LEAD for s in scratch))
            for s in scratch:
                assert bool((s[:CC.LEAD] == CC.SENTINEL).all()) and bool((s[-CC.LEAD:] == CC.SENTINEL).all())
        else:
            _contract2(dev, True, True, probs)
        assert bool((parent[:CC.LEAD] == CC.SENTINEL).all()) and bool((parent[-CC.LEAD:] == CC.SENTINEL).all())
        assert bool((parent[CC.LEAD:CC.LEAD + O * ldd].view(O, ldd)[:, C:] == CC.SENTINEL).all()), "the padding columns were written"
        assert not bool(torch.isnan(D[:, :C]).any())
        return D[:, :C].clone(), ops

    gen = torch.Generator(dev).manual_seed(3)
    # direct: one batch entry each
    direct = [CC._case("gw0", 1, O, C1, n, CC.kk), CC._case("gw1", 1, O, C2, m, CC.kk)]
    values = [CC.float_inputs(c, True, gen, dev) for c in direct]
    got, _ = launch(direct, values, None)
    assert torch.equal(got[:, :C1], _result(direct[0], *values[0])[0]) and torch.equal(got[:, C1:], _result(direct[1], *values[1])[0])
    # split: sum over the B entries
    split = [CC._case("gw0", B, O, C1, n, CC.kk, reduce=True), CC._case("gw1", B, O, C2, m, CC.kk, reduce=True)]
    splits = tuple(lib.apn_pw_contract2_splits(p, B, O, C1, n, B, O, C2, m) for p in (0, 1))
    assert all(s >= 1 for s in splits) and max(splits) > 1
    for wide_a in (True, False):
        values = [CC.exact_inputs(c, wide_a, gen, dev) for c in split]
        got, ops = launch(split, values, splits)
        want = torch.cat([CC.reference(c, o[0][0], o[1][0], torch.int64)[0] for c, o in zip(split, ops)], dim=1)
        assert torch.equal(got.cpu().to(torch.int64), want)
    values = [CC.float_inputs(c, True, gen, dev) for c in split]
    got, ops = launch(split, values, splits)
    again, _ = launch(split, values, splits)
    assert torch.equal(got, again)
    for c, o, block in zip(split, ops, (got[:, :C1], got[:, C1:])):
        _float_bars(c, planes, block.unsqueeze(0), o[0][0], o[1][0], f"pair-split-{c.name}-{C1}+{C2}")


def test_zz_worst_figures_of_this_run(dev):
    """Prints the worst element-wise ratio and relative L2 per precision over whatever ran before it in this process (the
    figures quoted above the bars come from a whole-file run)."""
    for planes, (ratio, l2, at_ratio, at_l2) in WORST.items():
        print(f"planes {planes}: worst element-wise ratio {ratio:.3e} ({at_ratio}), worst relative L2 {l2:.3e} ({at_l2})")
