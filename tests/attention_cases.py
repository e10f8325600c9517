"""The problems tests/test_gpu_attention_cases.py gives the attention kernels of csrc/attention.hip, in plain torch (no
extension): tests/test_attention_cases_cpu.py checks the table itself on the CPU.

EXACT cases -- one wrong, missing or doubled element anywhere shows.  Per (cloud, head) the M keys are partitioned into
groups (of 2^r keys; what does not fill a group stays single), scattered over the cloud by a random permutation.  Group G
has its own random 16-bit code c_G; its keys are the +-1 sign code of c_G and query i is 256 * code of the group it
targets.  A key of the targeted group then scores 16 * 256 / 4 = 1024 nats, any other at most 1024 - 128 (>= one bit
differs): the gap of 128 nats = 184 in log2 units puts every other probability below 2^-149 -- exactly 0 in float32 --
while the maximum's own is exp2(0) = 1.  With integer values every operand fits two bf16 planes and every partial sum is
exact, so

    out[i] == mean of v over the targeted group        dV[j] == (sum of dO over the queries targeting j's group) / 2^r

with NO tolerance (float64 soft-max does not give this: it leaks ~1e-53; the reference is the combinatorial statement).
dQ and dK: dS_ij = P_ij (dO_i . v_j - delta_i), delta_i = dO_i . out_i.  With single keys (r = 0) out_i = v_j and dS = 0
provided the kernel's dO . v is the integer one.  Two bf16 planes drop lo * lo, so that needs ONE of the two factors in
one plane: the backward is run twice, with
    "wide"    v, dO integers in [-2047, 2047] (two planes each): out and dV are compared (P = 2^-r has one plane);
    "narrow"  r = 0: v as before, dO = 16 * [-127, 127] (one plane; partial sums multiples of 16 below 2^28);
              r > 0: v, dO in [-7, 7], where dS = 2^-r (dO . (v_j - mean)) has at most 13 bits (fits the split of dS);
              out, dQ == 0, dK == 64 code_j (sum_i dS_ij) and dV are compared.
k has no low plane (+-1), so the score of a (query, key) pair is the same sum of the same products in the forward and in
both backward kernels: s - lse is exactly 0 or -r there.

FLOAT cases: Gaussian q, k, v with q scaled by 0.25 .. 8, a common offset (the shape of x W + emb), per-element random
binades, a late maximum (every chunk's best score above the previous chunk's) and q = 0 (uniform soft-max).
"""
import collections
import math

import torch

HEAD_DIM = 16
TILE, CHUNK = 32, 256            # keys per MFMA tile / per LDS pass of csrc/attention.hip
SENTINEL = 0x4B1D5EED            # bit pattern around the outputs (a finite float, ~1.03e7, that no result here equals)
LEAD = 12                        # poisoned floats in front of every buffer (a multiple of 4: views stay 16-byte aligned)
WIDE, ONE_PLANE, SMALL = 2047, 127, 7

Exact = collections.namedtuple("Exact", "name B M H r pi")          # groups of 2^r keys; pi: identity | perm | many
MFMA_M = [32, 64, 224, 256, 288, 512, 544, 1024, 2048, 4096]
MFMA_H = [1, 2, 3, 4, 8, 16]
MFMA_B = [1, 2, 5, 32]
SMALL_H = [1, 2, 4, 16]
SMALL_B = [1, 3, 32]
PIS = ["identity", "perm", "many"]

_MFMA = [(1, 32, 1, 0, "identity"), (2, 32, 4, 1, "many"), (2, 64, 2, 1, "perm"), (1, 224, 3, 2, "many"),
         (2, 256, 8, 0, "perm"), (5, 288, 3, 1, "identity"), (1, 288, 1, 0, "many"), (1, 512, 16, 2, "perm"),
         (2, 544, 1, 0, "many"), (1, 544, 2, 2, "identity"), (2, 1024, 4, 1, "perm"), (32, 2048, 4, 0, "perm"),
         (1, 2048, 2, 2, "many"), (1, 4096, 2, 2, "identity"), (1, 4096, 1, 0, "many")]
EXACT_MFMA = [Exact("B%d-M%d-H%d-g%d-%s" % (b, m, h, 1 << r, pi), b, m, h, r, pi) for b, m, h, r, pi in _MFMA]


def _small_cases():
    out = []
    for m in range(1, 32):
        h, b = SMALL_H[m % 4], SMALL_B[m % 3]
        out.append(Exact("B%d-M%d-H%d-g1-%s" % (b, m, h, PIS[m % 3]), b, m, h, 0, PIS[m % 3]))
        r = 1 + m % 2
        if (1 << r) <= m:
            h, b = SMALL_H[(m + 2) % 4], SMALL_B[(m + 1) % 3]
            out.append(Exact("B%d-M%d-H%d-g%d-%s" % (b, m, h, 1 << r, PIS[(m + 1) % 3]), b, m, h, r, PIS[(m + 1) % 3]))
    return out


EXACT_SMALL = _small_cases()


def per_head(t, heads):
    """(B, M, heads*16) -> (B, heads, M, 16)"""
    B, M, _ = t.shape
    return t.reshape(B, M, heads, HEAD_DIM).permute(0, 2, 1, 3)


def merged(t):
    """(B, heads, M, 16) -> (B, M, heads*16)"""
    B, H, M, _ = t.shape
    return t.permute(0, 2, 1, 3).reshape(B, M, H * HEAD_DIM)


def _bits(code):
    """16-bit codes (...) -> +-1 sign codes (..., 16), float64"""
    d = torch.arange(HEAD_DIM)
    return (((code.unsqueeze(-1) >> d) & 1) * 2 - 1).double()


def anchors(M):
    """Key positions a 'many' map always targets: first tile, last tile of the first chunk, first tile of the next chunk,
    last tile of the cloud (as far as the cloud has them)."""
    want = [0, TILE - 1, CHUNK - TILE, CHUNK - 1, CHUNK, CHUNK + TILE - 1, M - TILE, M - 1]
    return sorted({p for p in want if 0 <= p < M})


def exact_structure(case, seed=0):
    """-> dict of CPU tensors: grp (B,H,M) the group of every key, size (B,H,M) its group's size, tgt (B,H,M) the group
    every query targets, code (B,H,M) the 16-bit code of every key's group, q, k (B,M,H*16) float32."""
    B, M, H, g = case.B, case.M, case.H, 1 << case.r
    gen = torch.Generator().manual_seed(1000 * seed + 7 * M + 3 * H + B + case.r)
    full = (M // g) * g
    slot_group = torch.where(torch.arange(M) < full, torch.arange(M) // g, torch.arange(M) - full + M // g)
    slot_size = torch.where(torch.arange(M) < full, g, 1)
    order = torch.argsort(torch.rand(B, H, M, generator=gen), dim=-1)       # key j holds slot order[..., j]
    grp, size = slot_group[order], slot_size[order]
    if case.pi == "identity":
        tkey = torch.arange(M).expand(B, H, M)
    elif case.pi == "perm":
        tkey = torch.argsort(torch.rand(B, H, M, generator=gen), dim=-1)
    else:                                                                   # many-to-one: a few targets, fan-in ~8
        pool = torch.tensor(anchors(M) + torch.randint(0, M, (max(1, M // 8),), generator=gen).tolist())
        tkey = pool[torch.randint(0, len(pool), (B, H, M), generator=gen)]
        tkey[..., :len(pool)] = pool[:M]                                    # every target of the pool occurs
    tgt = torch.gather(grp, 2, tkey)
    base = torch.randperm(1 << 16, generator=gen)                            # distinct codes within a (cloud, head)
    shift = (torch.arange(B).view(B, 1, 1) * H + torch.arange(H).view(1, H, 1)) * 977
    code = base[(grp + shift) % (1 << 16)]
    qcode = base[(tgt + shift) % (1 << 16)]
    k = merged(_bits(code)).float()
    q = merged(_bits(qcode) * 256.0).float()
    return dict(grp=grp, size=size, tgt=tgt, code=code, q=q, k=k, tkey=tkey)


def exact_values(case, variant, seed=0):
    """-> v, dO (B, M, H*16) float32 integers: 'wide' or 'narrow' (module docstring)."""
    gen = torch.Generator().manual_seed(77 + 1000 * seed + case.M + 5 * case.H + 11 * case.B + (variant == "wide"))
    shape = (case.B, case.M, case.H * HEAD_DIM)
    ri = lambda w: torch.randint(-w, w + 1, shape, generator=gen).float()
    if variant == "wide":
        return ri(WIDE), ri(WIDE)
    if case.r == 0:
        return ri(WIDE), 16.0 * ri(ONE_PLANE)
    return ri(SMALL), ri(SMALL)


def exact_expect(case, st, v, dO):
    """The combinatorial statement, in float64 (every value a small integer over a power of two: exact):
    -> out, dq, dk, dv (B, M, H*16) and the quantities the exactness argument bounds (dict)."""
    H = case.H
    grp, size, tgt = st["grp"], st["size"], st["tgt"]
    G = int(grp.max()) + 1
    vh, gh = per_head(v, H).double(), per_head(dO, H).double()
    B = vh.shape[0]
    idx = lambda t: t.unsqueeze(-1).expand(-1, -1, -1, HEAD_DIM)
    gsize = torch.zeros(B, H, G).scatter_add_(2, grp, torch.ones(grp.shape)).double()
    gsum = torch.zeros(B, H, G, HEAD_DIM, dtype=torch.float64).scatter_add_(2, idx(grp), vh)
    out = torch.gather(gsum / gsize.unsqueeze(-1), 2, idx(tgt))
    A = torch.zeros(B, H, G, HEAD_DIM, dtype=torch.float64).scatter_add_(2, idx(tgt), gh)      # sum of dO over the queries of G
    delta = (gh * out).sum(-1)
    c = torch.zeros(B, H, G, dtype=torch.float64).scatter_add_(2, tgt, delta)
    Aj = torch.gather(A, 2, idx(grp))
    dv = Aj / size.unsqueeze(-1)
    colsum = ((Aj * vh).sum(-1) - torch.gather(c, 2, grp)) / size                            # sum_i dS_ij
    dk = colsum.unsqueeze(-1) * 64.0 * _bits(st["code"])                                     # q_i / 4 = 64 code
    dq = torch.zeros_like(out)
    fan = torch.zeros(B, H, G).scatter_add_(2, tgt, torch.ones(tgt.shape))
    # what the exactness argument bounds (tests/test_attention_cases_cpu.py): the largest fan-in of a group, the largest
    # |dS| and the largest sum over a key's queries of |dS| * 64
    claims = dict(fan=int(fan.max()), g=1 << case.r, dk_abs=float(dk.abs().max()), colsum=float(colsum.abs().max()))
    return merged(out), merged(dq), merged(dk), merged(dv), claims


def min_gap_log2(st):
    """The smallest score gap between a query's group and any other key, in log2 units: 128 nats per differing bit."""
    code = st["code"]
    B, H, M = code.shape
    worst = HEAD_DIM
    for b in range(B):
        for h in range(H):
            c = torch.unique(code[b, h])
            assert len(c) == len(torch.unique(st["grp"][b, h])), "two groups share a code"
            if len(c) > 1 and M <= 1024:
                x = c.unsqueeze(0) ^ c.unsqueeze(1)
                pop = sum((x >> d) & 1 for d in range(HEAD_DIM))
                pop.fill_diagonal_(HEAD_DIM)
                worst = min(worst, int(pop.min()))
            else:
                worst = min(worst, 1)                      # distinct codes differ in at least one bit
    return worst * 128.0 * math.log2(math.e)


# ---- float cases --------------------------------------------------------------------------------------------------------

REGIMES = ["n0.25", "n1", "n2", "n4", "n8", "offset", "binades", "late-max", "q0"]
Float = collections.namedtuple("Float", "name B M H regime")
_FLOAT_SHAPES = [(1, 32, 1), (2, 32, 4), (2, 64, 2), (1, 224, 3), (2, 256, 8), (5, 288, 3), (1, 512, 16), (2, 544, 1),
                 (2, 1024, 4), (32, 2048, 4), (1, 2048, 2), (1, 4096, 2)]


def _float_cases():
    out = []
    for s, (b, m, h) in enumerate(_FLOAT_SHAPES):
        regimes = REGIMES if (b, m, h) in ((2, 64, 2), (2, 1024, 4), (5, 288, 3)) else [REGIMES[(2 * s + i * 4) % 9] for i in range(2)]
        out += [Float("B%d-M%d-H%d-%s" % (b, m, h, r), b, m, h, r) for r in regimes]
    # the hardest regimes on the flagship pair and the deepest recurrence as well
    have = {(c.M, c.regime) for c in out}
    for (b, m, h), regimes in (((32, 2048, 4), ["n8", "late-max"]), ((1, 4096, 2), ["q0", "offset"])):
        out += [Float("B%d-M%d-H%d-%s" % (b, m, h, r), b, m, h, r) for r in regimes if (m, r) not in have]
    return out


FLOAT_MFMA = _float_cases()
FLOAT_SMALL = [Float("B%d-M%d-H%d-%s" % (SMALL_B[m % 3], m, SMALL_H[m % 4], REGIMES[m % 9]), SMALL_B[m % 3], m, SMALL_H[m % 4],
                     REGIMES[m % 9]) for m in range(1, 32)]


def float_inputs(case, device="cpu", seed=0):
    """-> q, k, v, dO (B, M, H*16) float32 on `device` (generated on the CPU: the same values everywhere)."""
    gen = torch.Generator().manual_seed(31 * seed + case.M + 7 * case.H + 13 * case.B + 101 * REGIMES.index(case.regime))
    shape = (case.B, case.M, case.H * HEAD_DIM)
    q, k, v, g = (torch.randn(shape, generator=gen) for _ in range(4))
    r = case.regime
    if r.startswith("n"):
        q = q * float(r[1:])
    elif r == "offset":
        q, k, v = q + 3.0, k + 3.0, v + 5.0
    elif r == "binades":
        q, k, v, g = (t * torch.exp2(torch.randint(-6, 3, shape, generator=gen).float()) for t in (q, k, v, g))
    elif r == "late-max":
        # every query leans along one direction per head and the keys' component along it grows with the key index:
        # the best score of every chunk (of every tile, nearly) exceeds everything before it
        dirn = torch.nn.functional.normalize(torch.randn(1, 1, case.H, HEAD_DIM, generator=gen), dim=-1)
        ramp = torch.linspace(-2.0, 4.0, case.M).view(1, case.M, 1, 1)
        lean = (1.0 + torch.rand(case.B, case.M, case.H, 1, generator=gen)) * 6.0
        k = (0.1 * k.view(case.B, case.M, case.H, HEAD_DIM) + ramp * dirn).reshape(shape)
        q = (0.5 * q.view(case.B, case.M, case.H, HEAD_DIM) + lean * dirn).reshape(shape)
    elif r == "q0":
        q = torch.zeros(shape)
        v = torch.randint(-WIDE, WIDE + 1, shape, generator=gen).float()
    return tuple(t.to(device) for t in (q, k, v, g))


# ---- poisoned buffers ---------------------------------------------------------------------------------------------------

def in_nan_parent(t):
    """A contiguous copy of `t` as a 16-byte aligned view into a NaN-filled parent."""
    parent = torch.full((t.numel() + 2 * LEAD,), float("nan"), dtype=torch.float32, device=t.device)
    view = parent[LEAD:LEAD + t.numel()].view(t.shape)
    view.copy_(t)
    return view


def in_sentinel_parent(nbytes, device):
    """-> (int32 view of `nbytes` bytes, offset but 16-byte aligned, its int32 parent): the parent is SENTINEL everywhere.
    nbytes is a multiple of 4."""
    assert nbytes % 4 == 0
    parent = torch.full((nbytes // 4 + 2 * LEAD,), SENTINEL, dtype=torch.int32, device=device)
    return parent[LEAD:LEAD + nbytes // 4], parent


def borders_intact(parent):
    return bool((parent[:LEAD] == SENTINEL).all()) and bool((parent[-LEAD:] == SENTINEL).all())
