"""CPU suite: the case table of tests/attention_cases.py and the references of tests/attention_reference.py keep their own
promises -- checked with integers, the float32 composition (`attention._reference`) and the numpy oracle; no kernel runs."""
import math

import numpy as np
import pytest
import torch

import attention_cases as AC
import attention_reference as AR

EXACT = AC.EXACT_MFMA + AC.EXACT_SMALL


def _clouds(case, *tensors, most=2):
    """The first and the last cloud of a case (the composition materialises B*H*M*M scores)."""
    pick = sorted({0, case.B - 1})[:most]
    return [t[pick] for t in tensors]


def test_the_table_covers_every_shape_the_kernels_treat_differently():
    for cases, Ms, Hs, Bs in ((AC.EXACT_MFMA, AC.MFMA_M, AC.MFMA_H, AC.MFMA_B), (AC.EXACT_SMALL, range(1, 32), AC.SMALL_H, AC.SMALL_B),
                              (AC.FLOAT_MFMA, AC.MFMA_M, AC.MFMA_H, AC.MFMA_B), (AC.FLOAT_SMALL, range(1, 32), AC.SMALL_H, AC.SMALL_B)):
        assert {c.M for c in cases} == set(Ms) and {c.H for c in cases} == set(Hs) and {c.B for c in cases} == set(Bs)
    for cases in (AC.EXACT_MFMA, AC.FLOAT_MFMA):
        shapes = {(c.M, c.H, c.B) for c in cases}
        assert (2048, 4, 32) in shapes and (288, 3, 5) in shapes
    assert {c.r for c in AC.EXACT_MFMA} == {0, 1, 2} == {c.r for c in AC.EXACT_SMALL}
    assert {c.pi for c in AC.EXACT_MFMA} == set(AC.PIS) == {c.pi for c in AC.EXACT_SMALL}
    for r in AC.REGIMES:                      # every regime: a single chunk, a ragged last chunk and a deep recurrence
        Ms = {c.M for c in AC.FLOAT_MFMA if c.regime == r}
        assert min(Ms) <= 256 and max(Ms) >= 1024 and Ms & {288, 544}, (r, Ms)
        assert any(c.regime == r for c in AC.FLOAT_SMALL)
    assert len({c.name for c in EXACT}) == len(EXACT) and len({c.name for c in AC.FLOAT_MFMA}) == len(AC.FLOAT_MFMA)


@pytest.mark.parametrize("case", EXACT, ids=[c.name for c in EXACT])
def test_exact_case_claims(case):
    """gap >= 150 log2 units; targeted keys in the first tile, the last tile of a chunk, the first tile of the next
    chunk and the last tile of the cloud, reached both first (alpha = 0 after it) and later (alpha = 1); groups spread
    over tiles and chunks; every partial sum exactly representable; the float32 composition returns the combinatorial
    answer exactly."""
    st = AC.exact_structure(case)
    M, g = case.M, 1 << case.r
    assert AC.min_gap_log2(st) >= 150.0
    grp, tgt, size = st["grp"], st["tgt"], st["size"]
    assert set(torch.unique(size).tolist()) <= {1, g} and (M < g or int(size.max()) == g)
    # positions: member[b,h,i,j] = key j belongs to the group query i targets (first cloud and head are enough to look at)
    member = tgt[0, 0].unsqueeze(1) == grp[0, 0].unsqueeze(0)
    assert bool((member.sum(1) == torch.gather(size[0, 0], 0, st["tkey"][0, 0])).all())
    hit = member.any(0)                                                # keys that some query targets
    first = member.float().argmax(1)                                   # first key of every query's group
    if M >= AC.TILE:
        tiles = set((torch.nonzero(hit).flatten() // AC.TILE).tolist())
        want = {0, M // AC.TILE - 1} | ({AC.CHUNK // AC.TILE - 1, AC.CHUNK // AC.TILE} if M > AC.CHUNK else set())
        assert want <= tiles, (want, tiles)
        if M >= 2 * AC.TILE:
            assert bool((first >= AC.TILE).any()), "alpha = 0: the maximum arrives after the first tile"
            assert bool((first < AC.TILE).any()) or g > 1, "alpha = 1 from the second tile on"
        if g > 1 and M >= 2 * AC.TILE:
            last = M - 1 - member.flip(1).float().argmax(1)
            assert bool((last // AC.TILE > first // AC.TILE).any()), "a group spread over tiles"
            if M > AC.CHUNK:
                assert bool((last // AC.CHUNK > first // AC.CHUNK).any()), "a group spread over chunks"
    for variant in ("wide", "narrow"):
        v, dO = AC.exact_values(case, variant)
        out, dq, dk, dv, claims = AC.exact_expect(case, st, v, dO)
        vmax, gmax, fan = float(v.abs().max()), float(dO.abs().max()), claims["fan"]
        # forward: integers, at most g of them summed; dV: multiples of 1/g, at most `fan` of them
        assert g * vmax < 2 ** 24 and fan * gmax < 2 ** 24
        if variant == "narrow":
            # dP = dO . v: one factor in one bf16 plane, multiples of `gran`
            gran = 16.0 if case.r == 0 else 1.0
            assert bool((dO / gran == (dO / gran).round()).all()) and float((dO / gran).abs().max()) <= 127
            assert 16 * vmax * gmax / gran < 2 ** 24
            # dS = (dP - delta) / g: multiples of 1 / g^2 that fit the two-plane split (16 bits); 0 with single keys
            ds_max = 2 * 16 * vmax * gmax / g if g > 1 else 0.0
            assert ds_max * g * g < 2 ** 16
            # dK: sums of `fan` values of 64 dS
            assert fan * 64 * ds_max * g * g / 64 < 2 ** 24
            assert bool((dq == 0).all()) and (g > 1 or bool((dk == 0).all()))
            if g > 1 and M >= 8:
                assert bool((dk != 0).any())
        # the float32 composition gives the same, exactly (forward; backward through autograd)
        q, k, vv, gg, eo, ek, ev = _clouds(case, st["q"], st["k"], v, dO, out, dk, dv)
        from adaptpoint_amd.attention import _reference
        leaves = [t.clone().requires_grad_(True) for t in (q, k, vv)]
        got = _reference(*leaves, case.H)
        assert torch.equal(got.detach().double(), eo), (case.name, variant)
        got.backward(gg)
        assert torch.equal(leaves[2].grad.double(), ev), (case.name, variant, "dv")
        if variant == "narrow":
            assert bool((leaves[0].grad == 0).all()), (case.name, "dq")
            assert torch.equal(leaves[1].grad.double(), ek), (case.name, "dk")


@pytest.mark.parametrize("case", AC.FLOAT_MFMA + AC.FLOAT_SMALL, ids=[c.name for c in AC.FLOAT_MFMA + AC.FLOAT_SMALL])
def test_float_case_claims_and_the_references(case):
    """The float64 reference equals the numpy oracle; the float32 composition and the model of the kernels' arithmetic
    both sit inside the derived element-wise bars (the composition far inside); the regimes are what they say."""
    from adaptpoint_amd.attention import _reference
    from oracle import oracle as O
    q, k, v, g = _clouds(case, *AC.float_inputs(case), most=1 if case.M >= 2048 else 2)
    H = case.H
    ref = AR.float64(q, k, v, H, g)
    want = O.attention(q.numpy(), k.numpy(), v.numpy(), H)
    grads = O.attention_grad(q.numpy(), k.numpy(), v.numpy(), H, g.numpy())
    for name, w in zip(("out", "dq", "dk", "dv"), (want,) + tuple(grads)):
        assert np.abs(ref[name].numpy() - w).max() <= 1e-12 * max(1.0, np.abs(w).max()), name
    leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
    comp = _reference(*leaves, H)
    comp.backward(g)
    mod = AR.model(q, k, v, H, g)
    worst = {}
    for name, got in (("out", comp.detach()), ("dq", leaves[0].grad), ("dk", leaves[1].grad), ("dv", leaves[2].grad)):
        for who, t in (("composition", got), ("model", mod[name])):
            ratio = float(((t.double() - ref[name]).abs() / ref["bar_" + name].clamp_min(1e-300)).max())
            worst[who] = max(worst.get(who, 0.0), ratio)
    lse_ratio = float(((mod["lse"].double() - ref["lse"]).abs() / ref["bar_lse"]).max())
    print(f"{case.name}: worst ratio to the element-wise bar: composition {worst['composition']:.3f}, model {worst['model']:.3f}, "
          f"model lse {lse_ratio:.3f}")
    assert worst["composition"] <= 0.05 and worst["model"] <= 1.0 and lse_ratio <= 1.0
    if case.regime == "q0":
        mean = AC.merged(AC.per_head(v, H).double().mean(2, keepdim=True).expand(-1, -1, case.M, -1))
        assert float((ref["out"] - mean).abs().max()) <= 1e-9
        if case.M & (case.M - 1) == 0:
            assert torch.equal(comp.detach().double(), mean) and torch.equal(mod["out"].double(), mean)
    if case.regime == "late-max" and case.M > AC.CHUNK:
        s = AC.per_head(q, H).double() @ AC.per_head(k, H).double().transpose(-1, -2)
        best = s[..., :case.M // AC.CHUNK * AC.CHUNK].reshape(*s.shape[:3], -1, AC.CHUNK).amax(-1)
        assert bool((best[..., 1:] > best[..., :-1]).all()), "every chunk's best score exceeds the previous chunk's"


def test_image_permutation_is_a_permutation_and_inverts():
    perm = AR.tile_permutation()
    assert sorted(perm) == list(range(32))
    x = torch.randn(1, 2, 64, 16)
    img = torch.empty(1, 2, 2, 16, 2, 32)
    hi, lo = AR.split(x)
    for part, t in enumerate((hi, lo)):
        tiles = t.permute(0, 1, 3, 2).reshape(1, 2, 16, 2, 32)
        img[:, :, part] = tiles[..., perm]
    got_hi, got_lo = AR.trans_image(img.to(torch.bfloat16).flatten(), 1, 2, 64)
    assert torch.equal(got_hi, hi) and torch.equal(got_lo, lo)


def test_the_reason_a_call_is_composed_names_what_is_out_of_range():
    """Shapes only (meta tensors): the grid limits of 65535 clouds and heads, a foreign head dim, a ragged M."""
    from adaptpoint_amd.attention import _why_composed, supported
    t = lambda *shape: torch.empty(*shape, device="meta")
    assert "batch 65536" in _why_composed(t(65536, 32, 16), 1)
    assert "heads 65536" in _why_composed(t(1, 32, 65536 * 16), 65536)
    assert "head dim 8" in _why_composed(t(2, 32, 32), 4)
    assert "heads 0" in _why_composed(t(2, 32, 32), 0)
    assert "M=50" in _why_composed(t(2, 50, 64), 4)
    assert not supported(t(2, 32, 64), 4)                     # not a GPU tensor
