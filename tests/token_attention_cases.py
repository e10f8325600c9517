"""The problems tests/test_gpu_token_attention.py gives the head-dim-64 kernels of csrc/token_attention.hip, in plain torch
(no extension); tests/test_token_attention_cases_cpu.py checks the table itself on the CPU.  The head-dim-64 counterpart of
tests/attention_cases.py, on the packed qkv (B, T, [3][H][64]) and for ragged T.

EXACT cases.  Per (cloud, head) the T keys are partitioned into groups of 2^r keys (what does not fill a group stays
single), scattered over the cloud by a random permutation.  Every group has its own random 64-bit code; its keys are the
+-1 sign code and a query is 512 * the code of the group it targets.  A key of the targeted group scores
64 * 512 / 8 = 4096 nats, any other at most 4096 - 128 (one differing bit costs 2 * 512 / 8): 184 log2 units, so every
other probability is below 2^-149 -- exactly 0 in float32 -- and the maximum's own is exp2(0) = 1.  Hence, with integer
values and NO tolerance,

    out[i] == mean of v over the targeted group          dV[j] == (sum of dO over the queries targeting j's group) / 2^r
    lse[i] == fl(score * log2e_f32) + r  (log2 units; the product is a power-of-two multiple of the float32 constant and
              the sum stays inside its binade's grid: both exact)
    dQ == 0                                              dK[j] == (sum_i dS_ij) * q_i / 8   (q_i the same for all i of j's group)

BIASED variant: the codes have 63 bits, k[63] = +1 for every key and q[63] = -32768, so the targeted score is
(63 * 512 - 32768) / 8 = -64 nats and every real score is negative: a zero-padded key that is not masked holds the LARGEST
score (0) of its row and takes all the probability.  The plain cases cannot see that (a zero score is 4096 nats below the
targeted one); test_token_attention_cases_cpu.py shows both on the model.

Exactness of the arithmetic the kernels use (two bf16 planes per operand, lo * lo dropped, float32 accumulation; the scale
0.125 * log2e_f32 applied to the finished sum):
  q, k      512, 32768, 1: one plane; every product and partial sum of a score is an integer multiple of 64 below 2^19.
  P         1 relative to the maximum, 2^-r after the division / against the saved lse: one plane.
  "wide"    v, dO integers in [-2047, 2047] (two planes, hi + lo exact): P v and P dO are exact, sums of at most 2^r
            resp. `fan` of them: out, lse and dV are compared.
  "narrow"  r = 0: v in [-1023, 1023], dO = 16 * [-127, 127] (ONE plane, so dO . v loses no lo * lo term; partial sums are
            multiples of 16 below 2^28): dP == delta exactly, dS == 0, dQ == dK == 0.
            r > 0: v, dO in [-7, 7]: dS = 2^-r (dO . (v_j - mean)) is a multiple of 4^-r with at most 15 bits: fits the
            split.  dK sums at most `fan` products dS * q (powers of two times dS): exact below 2^24 * 4^-r * 32768.
k has no low plane, so the score of a (query, key) pair is the same sum of the same products in the forward and in both
backward kernels: s - lse is exactly 0 or -r there.

FLOAT cases: the regimes of attention_cases.REGIMES at 64 dims.
"""
import collections

import torch

from attention_cases import REGIMES, SENTINEL, LEAD, in_nan_parent, in_sentinel_parent, borders_intact  # noqa: F401

HEAD_DIM = 64
TILE = 32                        # keys per MFMA tile
FWD_CHUNK, BWD_CHUNK = 64, 32    # points per LDS pass of the forward / of the two backward kernels
WG_ROWS = 128                    # rows a workgroup owns (4 waves of 32)
WIDE, NARROW_V, ONE_PLANE, SMALL = 2047, 1023, 127, 7
QMAG, QBIAS = 512.0, -32768.0
LOG2E_F32 = float(torch.tensor(1.4426950408889634, dtype=torch.float32))

RAGGED_T = [1, 2, 31, 32, 33, 63, 64, 65, 96, 129, 257, 300]
Exact = collections.namedtuple("Exact", "name B T H r pi biased")
PIS = ["identity", "perm", "many"]
_B, _H = [1, 2, 5], [1, 2, 6]


def _exact_cases():
    out = []
    for n, t in enumerate(RAGGED_T):
        for biased in (False, True):
            b, h = _B[(n + biased) % 3], _H[(n + 2 * biased) % 3]
            r = (n + biased) % 3 if (1 << ((n + biased) % 3)) <= t else 0
            pi = PIS[(n + 2 * biased) % 3]
            out.append(Exact("B%d-T%d-H%d-g%d-%s-%s" % (b, t, h, 1 << r, pi, "biased" if biased else "plain"), b, t, h, r, pi, biased))
    # past the forward's LDS chunk many times over and one past a multiple of every tile size; the working batch
    out.append(Exact("B1-T1025-H2-g2-many-biased", 1, 1025, 2, 1, "many", True))
    out.append(Exact("B1-T1025-H2-g1-perm-plain", 1, 1025, 2, 0, "perm", False))
    out.append(Exact("B32-T65-H6-g4-many-biased", 32, 65, 6, 2, "many", True))
    return out


EXACT = _exact_cases()


def per_head(t, heads):
    """(B, T, heads*64) -> (B, heads, T, 64)"""
    B, T, _ = t.shape
    return t.reshape(B, T, heads, HEAD_DIM).permute(0, 2, 1, 3)


def merged(t):
    """(B, heads, T, 64) -> (B, T, heads*64)"""
    B, H, T, _ = t.shape
    return t.permute(0, 2, 1, 3).reshape(B, T, H * HEAD_DIM)


def pack(q, k, v):
    """three (B, T, H*64) -> the packed (B, T, [3][H][64]) that nn.Linear(dim, 3 dim) produces"""
    return torch.cat([q, k, v], dim=-1).contiguous()


def unpack(t):
    return t.chunk(3, dim=-1)


def anchors(T):
    """Key positions a 'many' map always targets: the ends of the first tile, of the forward's first chunk, of the first
    workgroup's rows, and of the cloud (as far as the cloud has them)."""
    want = [0, TILE - 1, TILE, FWD_CHUNK - 1, FWD_CHUNK, WG_ROWS - 1, WG_ROWS, (T - 1) // TILE * TILE, T - 1]
    return sorted({p for p in want if 0 <= p < T})


def exact_structure(case, seed=0):
    """-> dict of CPU tensors: grp, size, tgt, tkey (B,H,T), sign (B,H,G,64) the +-1 code of every group (column 63 is +1 in
    the biased variant), q, k (B,T,H*64) float32, score (nats) of a targeted key."""
    B, T, H, g = case.B, case.T, case.H, 1 << case.r
    gen = torch.Generator().manual_seed(1000 * seed + 7 * T + 3 * H + B + case.r + 100003 * case.biased)
    full = (T // g) * g
    slot_group = torch.where(torch.arange(T) < full, torch.arange(T) // g, torch.arange(T) - full + T // g)
    slot_size = torch.where(torch.arange(T) < full, g, 1)
    order = torch.argsort(torch.rand(B, H, T, generator=gen), dim=-1)
    grp, size = slot_group[order], slot_size[order]
    if case.pi == "identity":
        tkey = torch.arange(T).expand(B, H, T).clone()
    elif case.pi == "perm":
        tkey = torch.argsort(torch.rand(B, H, T, generator=gen), dim=-1)
    else:
        pool = torch.tensor(anchors(T) + torch.randint(0, T, (max(1, T // 8),), generator=gen).tolist())
        tkey = pool[torch.randint(0, len(pool), (B, H, T), generator=gen)]
        tkey[..., :len(pool)] = pool[:T]
    tgt = torch.gather(grp, 2, tkey)
    G = int(grp.max()) + 1
    sign = torch.randint(0, 2, (B, H, G, HEAD_DIM), generator=gen).double() * 2 - 1
    qvec = sign * QMAG
    if case.biased:
        sign[..., 63] = 1.0
        qvec = sign * QMAG
        qvec[..., 63] = QBIAS
    idx = lambda t: t.unsqueeze(-1).expand(-1, -1, -1, HEAD_DIM)
    k = merged(torch.gather(sign, 2, idx(grp))).float()
    q = merged(torch.gather(qvec, 2, idx(tgt))).float()
    score = (63 * QMAG + QBIAS) / 8 if case.biased else 64 * QMAG / 8
    return dict(grp=grp, size=size, tgt=tgt, tkey=tkey, sign=sign, qvec=qvec, q=q, k=k, score=score)


def exact_values(case, variant, seed=0):
    """-> v, dO (B, T, H*64) float32 integers: 'wide' or 'narrow' (module docstring)."""
    gen = torch.Generator().manual_seed(77 + 1000 * seed + case.T + 5 * case.H + 11 * case.B + (variant == "wide"))
    shape = (case.B, case.T, case.H * HEAD_DIM)
    ri = lambda w: torch.randint(-w, w + 1, shape, generator=gen).float()
    if variant == "wide":
        return ri(WIDE), ri(WIDE)
    if case.r == 0:
        return ri(NARROW_V), 16.0 * ri(ONE_PLANE)
    return ri(SMALL), ri(SMALL)


def exact_expect(case, st, v, dO):
    """The combinatorial statement in float64 (every value a small integer over a power of two: exact):
    -> out, dq, dk, dv (B, T, H*64), lse (B, H, T) float32 in log2 units, claims (dict)."""
    H = case.H
    grp, size, tgt = st["grp"], st["size"], st["tgt"]
    G = st["sign"].shape[2]
    vh, gh = per_head(v, H).double(), per_head(dO, H).double()
    B = vh.shape[0]
    idx = lambda t: t.unsqueeze(-1).expand(-1, -1, -1, HEAD_DIM)
    gsize = torch.zeros(B, H, G).scatter_add_(2, grp, torch.ones(grp.shape)).double()
    gsum = torch.zeros(B, H, G, HEAD_DIM, dtype=torch.float64).scatter_add_(2, idx(grp), vh)
    out = torch.gather(gsum / gsize.unsqueeze(-1), 2, idx(tgt))
    A = torch.zeros(B, H, G, HEAD_DIM, dtype=torch.float64).scatter_add_(2, idx(tgt), gh)
    delta = (gh * out).sum(-1)
    c = torch.zeros(B, H, G, dtype=torch.float64).scatter_add_(2, tgt, delta)
    Aj = torch.gather(A, 2, idx(grp))
    dv = Aj / size.unsqueeze(-1)
    colsum = ((Aj * vh).sum(-1) - torch.gather(c, 2, grp)) / size                 # sum_i dS_ij
    dk = colsum.unsqueeze(-1) * torch.gather(st["qvec"], 2, idx(grp)) / 8.0
    dq = torch.zeros_like(out)
    fan = torch.zeros(B, H, G).scatter_add_(2, tgt, torch.ones(tgt.shape))
    r = torch.log2(torch.gather(gsize, 2, tgt)).float()
    lse = torch.tensor(st["score"], dtype=torch.float32) * torch.tensor(LOG2E_F32, dtype=torch.float32) + r
    claims = dict(fan=int(fan.max()), g=1 << case.r, colsum=float(colsum.abs().max()), dk_abs=float(dk.abs().max()))
    return merged(out), merged(dq), merged(dk), merged(dv), lse, claims


def min_gap_nats(st):
    """The smallest score gap between a query's group and any other key: 128 nats per differing bit (asserts that no two
    groups of a (cloud, head) share a code)."""
    sign = st["sign"]
    agree = sign @ sign.transpose(-1, -2)                                          # 64 - 2 * differing bits
    agree.diagonal(dim1=-2, dim2=-1).fill_(-HEAD_DIM)
    ham = (HEAD_DIM - float(agree.max())) / 2 if sign.shape[2] > 1 else HEAD_DIM
    assert ham >= 1, "two groups share a code"
    return ham * 2 * QMAG / 8


# ---- float cases --------------------------------------------------------------------------------------------------------

Float = collections.namedtuple("Float", "name B T H regime")
_FLOAT_SHAPES = [(1, 1, 1), (2, 2, 2), (5, 31, 6), (1, 32, 2), (2, 33, 1), (5, 63, 2), (1, 64, 6), (2, 65, 6), (1, 96, 1),
                 (2, 129, 2), (5, 257, 1), (1, 300, 6), (1, 1025, 2), (32, 65, 6)]
_ALL_REGIMES = {(2, 65, 6), (2, 129, 2), (1, 300, 6)}


def _float_cases():
    out = []
    for s, (b, t, h) in enumerate(_FLOAT_SHAPES):
        regimes = REGIMES if (b, t, h) in _ALL_REGIMES else [REGIMES[(2 * s + i * 4) % 9] for i in range(2)]
        out += [Float("B%d-T%d-H%d-%s" % (b, t, h, r), b, t, h, r) for r in regimes]
    out += [Float("B1-T1025-H2-%s" % r, 1, 1025, 2, r) for r in ("late-max", "q0", "n8")]
    seen, uniq = set(), []
    for c in out:
        if c.name not in seen:
            seen.add(c.name)
            uniq.append(c)
    return uniq


FLOAT = _float_cases()


def float_inputs(case, device="cpu", seed=0):
    """-> qkv (B, T, 3*H*64), dO (B, T, H*64) float32 on `device` (generated on the CPU: the same values everywhere)."""
    gen = torch.Generator().manual_seed(31 * seed + case.T + 7 * case.H + 13 * case.B + 101 * REGIMES.index(case.regime))
    shape = (case.B, case.T, case.H * HEAD_DIM)
    q, k, v, g = (torch.randn(shape, generator=gen) for _ in range(4))
    r = case.regime
    if r.startswith("n"):
        q = q * float(r[1:])
    elif r == "offset":
        q, k, v = q + 1.5, k + 1.5, v + 5.0
    elif r == "binades":
        q, k, v, g = (t * torch.exp2(torch.randint(-6, 3, shape, generator=gen).float()) for t in (q, k, v, g))
    elif r == "late-max":
        # every query leans along one direction per head and the keys' component along it grows with the key index: the
        # best score of (nearly) every tile exceeds everything before it
        dirn = torch.nn.functional.normalize(torch.randn(1, 1, case.H, HEAD_DIM, generator=gen), dim=-1)
        ramp = torch.linspace(-2.0, 4.0, case.T).view(1, case.T, 1, 1)
        lean = (1.0 + torch.rand(case.B, case.T, case.H, 1, generator=gen)) * 12.0
        k = (0.1 * k.view(case.B, case.T, case.H, HEAD_DIM) + ramp * dirn).reshape(shape)
        q = (0.5 * q.view(case.B, case.T, case.H, HEAD_DIM) + lean * dirn).reshape(shape)
    elif r == "q0":
        q = torch.zeros(shape)
        v = torch.randint(-WIDE, WIDE + 1, shape, generator=gen).float()
    return pack(q, k, v).to(device), g.to(device)

