"""CPU suite: the case table of tests/token_attention_cases.py and the references of tests/token_attention_reference.py
keep their own promises -- checked with integers, the float32 composition (`token_attention.composed`) and float64
autograd; no kernel runs.  Also: the reasons a call falls back, and the argument validation of the two C entries."""
import pytest
import torch

import token_attention_cases as TC
import token_attention_reference as TR


def _clouds(case, *tensors, most=2):
    pick = sorted({0, case.B - 1})[:most]
    return [t[pick] for t in tensors]


def test_the_table_covers_every_shape_the_kernels_treat_differently():
    for cases in (TC.EXACT, TC.FLOAT):
        Ts = {c.T for c in cases}
        assert set(TC.RAGGED_T) <= Ts and 1025 in Ts                       # ragged tails, the chunk boundary (64, 65), far past it
        assert {c.B for c in cases} >= {1, 2, 5, 32} and {c.H for c in cases} >= {1, 2, 6}
        assert any((c.B, c.T, c.H) == (32, 65, 6) for c in cases)
        assert len({c.name for c in cases}) == len(cases)
    for t in TC.RAGGED_T:                                                  # every ragged T: plain AND biased
        assert {c.biased for c in TC.EXACT if c.T == t} == {False, True}
    assert {c.r for c in TC.EXACT} == {0, 1, 2} and {c.pi for c in TC.EXACT} == set(TC.PIS)
    for r in TC.REGIMES:                                                   # every regime: one tile, a ragged tail, a deep recurrence
        Ts = {c.T for c in TC.FLOAT if c.regime == r}
        assert min(Ts) <= 65 and max(Ts) >= 300 and any(t % 32 for t in Ts), (r, Ts)


@pytest.mark.parametrize("case", TC.EXACT, ids=[c.name for c in TC.EXACT])
def test_exact_case_claims(case):
    """The gap, the plane count of every operand, the representability of every sum -- and the model of the kernels'
    arithmetic, like the float32 composition, returns the combinatorial answer exactly (out, lse, dV; dQ, dK narrow)."""
    from adaptpoint_amd.token_attention import composed
    st = TC.exact_structure(case)
    T, g = case.T, 1 << case.r
    gap = TC.min_gap_nats(st)
    assert gap >= 128.0 and gap * TC.LOG2E_F32 >= 150.0                    # exp2(-150) == 0 in float32
    assert st["score"] == (-64.0 if case.biased else 4096.0)
    q, k = st["q"], st["k"]
    assert TR.planes(q) == 1 and TR.planes(k) == 1
    if case.biased:                                                        # every real score is negative; a zero pad's is 0
        s = TC.per_head(q[:1], case.H).double() @ TC.per_head(k[:1], case.H).double().transpose(-1, -2) / 8
        assert float(s.max()) == -64.0
    assert set(torch.unique(st["size"]).tolist()) <= {1, g} and (T < g or int(st["size"].max()) == g)
    if case.pi == "many":
        assert set(TC.anchors(T)) <= set(st["tkey"][0, 0].tolist())
    for variant in ("wide", "narrow"):
        v, dO = TC.exact_values(case, variant)
        out, dq, dk, dv, lse, claims = TC.exact_expect(case, st, v, dO)
        vmax, gmax, fan = float(v.abs().max()), float(dO.abs().max()), claims["fan"]
        assert TR.planes(v) <= 2 and TR.planes(dO) <= 2
        assert g * vmax < 2 ** 24 and fan * gmax < 2 ** 24                  # out: g integers; dV: `fan` multiples of 1/g
        if variant == "narrow":
            gran = 16.0 if case.r == 0 else 1.0
            assert TR.planes(dO) == 1 and 64 * vmax * gmax / gran < 2 ** 24  # dP: no lo*lo term; partial sums representable
            ds_max = 2 * 64 * vmax * gmax / g if g > 1 else 0.0
            assert ds_max * g * g < 2 ** 16                                 # dS fits the two-plane split
            assert fan * ds_max * g * g < 2 ** 24                           # dK: `fan` terms, powers of two times dS
            assert bool((dq == 0).all()) and (g > 1 or bool((dk == 0).all()))
            if g > 1 and T >= 8:
                assert bool((dk != 0).any())
        qq, kk, vv, gg, eo, eq, ek, ev, el = _clouds(case, q, k, v, dO, out, dq, dk, dv, lse)
        qkv = TC.pack(qq, kk, vv)
        mod = TR.model(qkv, case.H, gg)
        assert torch.equal(mod["out"].double(), eo), (case.name, variant, "model out")
        assert torch.equal(mod["lse"], el), (case.name, variant, "model lse")
        mq, mk, mv = TC.unpack(mod["dqkv"])
        assert torch.equal(mv.double(), ev), (case.name, variant, "model dv")
        leaf = qkv.clone().requires_grad_(True)
        got = composed(leaf, case.H)
        assert torch.equal(got.detach().double(), eo), (case.name, variant, "composition out")
        got.backward(gg)
        cq, ck, cv = TC.unpack(leaf.grad)
        assert torch.equal(cv.double(), ev), (case.name, variant, "composition dv")
        if variant == "narrow":
            assert bool((mq == 0).all()) and bool((cq == 0).all()), (case.name, "dq")
            assert torch.equal(mk.double(), ek) and torch.equal(ck.double(), ek), (case.name, "dk")


@pytest.mark.parametrize("case", [c for c in TC.EXACT if c.T in (1, 33, 65, 129)], ids=lambda c: c.name)
def test_only_the_biased_cases_see_an_unmasked_pad(case):
    """31 zero keys appended and NOT masked: the plain cases still come out exact (a zero score is 4096 nats below the
    targeted one), the biased ones do not (the pad's zero score is the row's largest)."""
    st = TC.exact_structure(case)
    v, dO = TC.exact_values(case, "wide")
    out = TC.exact_expect(case, st, v, dO)[0]
    qkv, eo = TC.pack(st["q"][:1], st["k"][:1], v[:1]), out[:1]
    got = TR.model(qkv, case.H, pad_keys=31)["out"].double()
    if case.biased:
        assert float((got - eo).abs().max()) > 100.0
    else:
        assert torch.equal(got, eo)


@pytest.mark.parametrize("case", TC.FLOAT, ids=[c.name for c in TC.FLOAT])
def test_float_case_claims_and_the_references(case):
    """The float64 reference equals float64 autograd through the composition; the float32 composition and the model of the
    kernels' arithmetic both sit inside the derived element-wise bars."""
    from adaptpoint_amd.token_attention import composed
    qkv, g = _clouds(case, *TC.float_inputs(case), most=1 if case.T >= 1025 else 2)
    H = case.H
    ref = TR.float64(qkv, H, g)
    leaf = qkv.double().requires_grad_(True)
    want = composed(leaf, H)
    want.backward(g.double())
    for name, w in (("out", want.detach()), ("dqkv", leaf.grad)):
        assert float((ref[name] - w).abs().max()) <= 1e-11 * max(1.0, float(w.abs().max())), name
    leaf = qkv.clone().requires_grad_(True)
    comp = composed(leaf, H)
    comp.backward(g)
    mod = TR.model(qkv, H, g)
    worst = {}
    for name, got in (("out", comp.detach()), ("dqkv", leaf.grad)):
        for who, t in (("composition", got), ("model", mod[name])):
            ratio = float(((t.double() - ref[name]).abs() / ref["bar_" + name].clamp_min(1e-300)).max())
            worst[who] = max(worst.get(who, 0.0), ratio)
    lse_ratio = float(((mod["lse"].double() - ref["lse"]).abs() / ref["bar_lse"]).max())
    print(f"{case.name}: worst ratio to the element-wise bar: composition {worst['composition']:.3f}, model {worst['model']:.3f}, "
          f"model lse {lse_ratio:.3f}")
    assert worst["composition"] <= 0.25 and worst["model"] <= 1.0 and lse_ratio <= 1.0
    if case.regime == "q0":
        mean = TC.merged(TC.per_head(qkv.chunk(3, -1)[2], H).double().mean(2, keepdim=True).expand(-1, -1, case.T, -1))
        assert float((ref["out"] - mean).abs().max()) <= 1e-9


def test_supported_and_the_reasons_a_call_falls_back():
    from adaptpoint_amd import token_attention as TA
    t = lambda *shape: torch.empty(*shape, device="meta")
    assert not TA.supported(torch.zeros(2, 5, 3 * 128), 2) and TA._why_composed(torch.zeros(2, 5, 3 * 128), 2) == "cpu tensor"
    before = dict(TA.COMPOSED_CALLS)
    qkv = torch.randn(2, 5, 3 * 128)
    got = TA.token_attention(qkv, 2)                                       # CPU tensor: the composition, counted
    assert torch.equal(got, TA.composed(qkv, 2))
    assert TA.COMPOSED_CALLS.get("cpu tensor", 0) == before.get("cpu tensor", 0) + 1
    TA.COMPOSED_CALLS.clear()
    TA.COMPOSED_CALLS.update(before)


def test_argument_validation_of_the_token_attention_entries_needs_no_gpu():
    """Null pointers, t = 0, b / heads of 0 or above 65535 (grid dimensions), t above the documented bound, a row count the
    delta kernel's grid cannot hold, and pointers their 16-byte accesses could not take: APN_EINVAL before any HIP call
    (P: a non-null, 16-byte aligned address that is never read)."""
    from adaptpoint_amd import _lib
    lib = _lib.load()
    EINVAL, P = -1, 4096
    assert lib.apn_token_attention_max_tokens() == 1 << 24

    def fwd(b=1, t=65, heads=1, qkv=P, out=P, lse=P):
        return lib.apn_token_attention_fwd(b, t, heads, qkv, out, lse, None)

    def bwd(b=1, t=65, heads=1, qkv=P, out=P, lse=P, g_out=P, delta=P, dqkv=P):
        return lib.apn_token_attention_bwd(b, t, heads, qkv, out, lse, g_out, delta, dqkv, None)

    pointers = {fwd: ["qkv", "out", "lse"], bwd: ["qkv", "out", "lse", "g_out", "delta", "dqkv"]}
    aligned = {fwd: ["qkv", "out"], bwd: ["qkv", "out", "g_out", "dqkv"]}
    for entry, names in pointers.items():
        for name in names:
            assert entry(**{name: None}) == EINVAL, (entry.__name__, name)
        assert entry(t=0) == EINVAL and entry(t=-65) == EINVAL and entry(t=(1 << 24) + 1) == EINVAL, entry.__name__
        for bad in (0, -1, 65536):
            assert entry(b=bad) == EINVAL and entry(heads=bad) == EINVAL, (entry.__name__, bad)
        assert entry(b=65535, t=1 << 24, heads=65535) == EINVAL               # b * t * heads / 16 past the grid
        for name in aligned[entry]:
            for off in (4, 8):
                assert entry(**{name: P + off}) == EINVAL, (entry.__name__, name, off)
