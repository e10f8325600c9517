"""Raw-contraction problems for csrc/pointwise.hip's `pw_gemm_body` as `pointwise.contract` / `apn_pw_contract2` reach it:
the case table, the operand construction (strided views into poisoned parent buffers), float64 / int64 references and a
Python statement of the host's loader choice.  Imports without a GPU; tests/test_contract_cases_cpu.py checks the table
itself, tests/test_gpu_contract.py runs it.

A problem is D[z] (R x Q) = A[z] (R x K) B[z] (K x Q).  Both operands are held here in the LOGICAL shape (nbatch, n, K)
-- element (i, k) of A, element (q, k) of B -- and laid out k-contiguous ((i, k) at i * ld + k) or row-contiguous
(k * ld + i), which is all the kernel's operand description says.
"""
import collections

import torch

PW_T, PW_KC = 128, 32            # csrc/pointwise.hip: workgroup tile, contraction indices per chunk
LEAD = 8                         # poisoned floats in front of every operand (a multiple of 4: `off` alone sets the alignment)
SENTINEL = 0x4B1D5EED            # bit pattern around the outputs (a finite float, ~1.03e7, that no result here equals)
WIDE, NARROW = 2047, 7           # exact inputs: integers of two bf16 planes against integers of one

FORMS = [(True, True), (True, False), (False, True), (False, False)]          # (a_kcont, b_kcont)
CLASSES = ["steady", "general4", "scalar"]
R_VALUES = Q_VALUES = [1, 3, 4, 31, 64, 127, 128, 129, 130, 257, 300]
K_VALUES = [1, 3, 4, 31, 32, 33, 64, 96, 100, 160, 1536]

# a_off / b_off: floats the origin is moved by; a_pad / b_pad: ld - (tight ld); a_batch / b_batch: "own" (rows * ld),
# "shared" (0) or an int g (rows * ld + g); d_pad: ldd - Q; d_gap: d_batch - R * ldd
Case = collections.namedtuple("Case", "name nbatch R Q K a_kcont b_kcont a_off b_off a_pad b_pad a_batch b_batch d_pad d_gap reduce")


def _case(name, nbatch, R, Q, K, form, a_off=0, b_off=0, a_pad=0, b_pad=0, a_batch="own", b_batch="own", d_pad=0, d_gap=0,
          reduce=False):
    return Case(name, nbatch, R, Q, K, form[0], form[1], a_off, b_off, a_pad, b_pad, a_batch, b_batch, d_pad, d_gap, reduce)


def _form_name(form):
    return ("k" if form[0] else "r") + ("k" if form[1] else "r")


def _table():
    cases = []
    for f, form in enumerate(FORMS):
        fn = _form_name(form)
        add = lambda name, *a, **kw: cases.append(_case(f"{fn}-{name}", *a, form, **kw))
        # every R, Q and K value with this form (three permutations of the eleven values: 3 and 5 are coprime to 11);
        # the other attributes cycle
        for i in range(11):
            R, Q, K = R_VALUES[i], Q_VALUES[(3 * i + f) % 11], K_VALUES[(5 * i + 2 * f) % 11]
            add(f"sizes{i}", [1, 2, 3][i % 3], R, Q, K, a_off=[0, 0, 1, 4][i % 4], b_off=[0, 4, 0, 3][(i + f) % 4],
                a_pad=[0, 4, 1][i % 3], b_pad=[0, 8, 3][(i + 1) % 3], a_batch=["own", "shared", 4][i % 3],
                b_batch=[8, "own", "shared"][i % 3], d_pad=[0, 5][i % 2], d_gap=[0, 7][(i // 2) % 2])
        # steady state: K % 32 == 0, both operands float4-readable (a row-contiguous operand in whole quads)
        add("steady-tight", 2, 132, 260, 96)
        add("steady-padded", 3, 64, 132, 160, a_off=4, b_off=8, a_pad=4, b_pad=12, a_batch=8, b_batch="shared", d_pad=3, d_gap=5)
        add("steady-long", 1, 128, 128, 1536, a_pad=8)
        add("steady-one-chunk", 2, 4, 4, 32, a_batch="shared")
        # the general form with float4: K % 4 == 0 but not % 32 ...
        add("g4-k100", 2, 132, 68, 100, a_pad=4, d_pad=1)
        add("g4-k4", 3, 260, 4, 4, b_batch="shared")
        # ... and K % 32 == 0 with only ONE operand float4-readable
        add("g4-a-moved", 2, 132, 68, 64, a_off=1)
        add("g4-b-moved", 2, 68, 132, 96, b_off=2, b_pad=4)
        add("g4-a-oddld", 1, 64, 64, 32, a_pad=1)
        # value by value: origins moved by 1, 2, 3 floats; odd ld; odd batch stride; rows % 4 != 0 (matters for a
        # row-contiguous operand only: a k-contiguous one does not care and the case is then steady state)
        add("scalar-off13", 2, 132, 68, 64, a_off=1, b_off=3)
        add("scalar-off22", 1, 130, 129, 100, a_off=2, b_off=2, d_pad=2)
        add("scalar-off31", 3, 31, 257, 33, a_off=3, b_off=1, a_batch="shared")
        add("scalar-oddld", 2, 132, 68, 96, a_pad=1, b_pad=3)
        add("scalar-oddbatch", 3, 64, 132, 64, a_batch=1, b_batch=3)
        add("rows-not-quads", 2, 127, 130, 64)
        # batch counts, more than one tile per entry: the XCD renumbering engages at 8 and 16, not at 3
        add("nb3-tiles", 3, 132, 260, 64)
        add("nb8-tiles", 8, 132, 260, 64, d_pad=4, d_gap=12)                       # gdx = 3, gdy = 2 at nbatch = 8
        add("nb8-general", 8, 130, 257, 33, a_off=1)
        add("nb16-tiles", 16, 129, 130, 36, a_batch="shared")
        add("nb16-steady", 16, 256, 132, 32, b_batch="shared")
        # split-K: trailing empty slices (a), slices that straddle batch entries in the steady-state form (b)
        add("split-empty4", 3, 128, 64, 96, reduce=True)
        add("split-empty7", 5, 100, 33, 70, reduce=True, a_off=1)
        add("split-straddle", 4, 128, 128, 160, reduce=True)
        add("split-straddle-general", 4, 130, 67, 150, reduce=True, b_pad=1)
        add("split-renumbered", 4, 64, 64, 128, reduce=True)                      # 16 chunks in 8 shares: gridDim.z = 8
    kk, kr, rk, rr = FORMS
    # the production call sites verbatim (B clouds, N points, M queries, H hidden, C + 3 input rows, O outputs)
    for C3, H, B, N in [(6, 32, 2, 256), (35, 64, 3, 200), (67, 64, 2, 130)]:
        M, C = N // 2, C3 - 3
        t = f"c{C3}h{H}"
        cases += [
            _case(f"wide255-{t}", B, N, H, C3, rk, b_batch="shared"),                                  # U = X^T W1^T
            _case(f"wide412-{t}", B, C, N, H, rk, a_off=3, a_pad=3, a_batch="shared"),                  # g_f, W1[:, 3:] in place
            _case(f"wide418-{t}", B, N, 3, H, kr, b_batch="shared"),                                   # g_p: a 3-column output
            _case(f"wide421-{t}", B, M, 3, H, kr, b_batch="shared"),                                   # g_q
            _case(f"wide426-{t}", B, H, C3, N, rk, reduce=True),                                       # g_w1
            _case(f"wide428-{t}", B, H, 3, M, rr, reduce=True),                                        # the queries' share
        ]
    for C1, C2, O, B, n, m in [(64, 128, 64, 2, 256, 64), (35, 29, 70, 3, 200, 50)]:
        t = f"c{C1}+{C2}"
        cases += [
            _case(f"prop138-{t}", B, O, m, C2, kr, a_batch="shared"),                                  # u = W f2 (no skip features)
            _case(f"prop201-{t}", B, C1, n, O, rr, a_pad=C2, a_batch="shared"),                         # g_f1 = W[:, :C1]^T gy
            _case(f"prop203-{t}", B, C2, m, O, rr, a_off=C1, a_pad=C1, a_batch="shared"),               # g_f2 = W[:, C1:]^T gu
            _case(f"prop216-{t}", B, O, C2, m, kk, reduce=True),                                       # gW = sum gu f2^T
        ]
    cases += [_case("linear-nobias-bwd-4096", 1, 96, 64, 4096, rr, reduce=True),                      # W.grad = g^T x
              _case("linear-nobias-bwd-odd", 1, 33, 70, 4100, rr, reduce=True)]
    return cases


CASES = _table()
CASE_IDS = [c.name for c in CASES]


# pairs for apn_pw_contract2's direct form (one operand form per pair) ...
kk, kr, rk, rr = FORMS
PAIRS = {
    # the hoisted feature-propagation block's pairs (propagation.py): the weight's column blocks addressed in place
    "forward-35+29": (_case("p0", 2, 70, 257, 35, kr, a_pad=29, a_batch="shared"),
                      _case("p1", 2, 70, 64, 29, kr, a_off=35, a_pad=35, a_batch="shared")),
    "forward-64+128": (_case("p0", 2, 64, 256, 64, kr, a_pad=128, a_batch="shared"),
                       _case("p1", 2, 64, 64, 128, kr, a_off=64, a_pad=64, a_batch="shared")),
    "grad-input-35+29": (_case("p0", 2, 35, 257, 70, rr, a_pad=29, a_batch="shared"),
                         _case("p1", 2, 29, 64, 70, rr, a_off=35, a_pad=35, a_batch="shared", d_pad=2, d_gap=1)),
    "eight-entries-kk": (_case("p0", 8, 130, 132, 64, kk), _case("p1", 8, 64, 260, 33, kk, d_pad=3)),
    "rk-uneven": (_case("p0", 3, 300, 31, 160, rk, b_batch="shared"), _case("p1", 1, 4, 129, 3, rk)),
}
# ... and (B, O, C1, C2, n, m) of the hoisted block's weight gradient, gW[:, :C1] | gW[:, C1:] as column blocks of one matrix:
# the direct form with one batch entry, the split form (pw_fold2_kernel) over the B entries
PAIR_BLOCKS = [(3, 70, 35, 29, 200, 50), (2, 64, 64, 128, 256, 64)]


def coverage():
    """What the GPU tests run, by purpose -> names: every (layout form, loader class, planes) -- each case runs with two
    and with three planes --, both folds, renumbered and plain grids of the direct and of the split form, split-K cases
    by name (their shares are checked against the library's answer in test_contract_cases_cpu.py)."""
    cov = collections.defaultdict(list)
    for c in CASES:
        for planes in (2, 3):
            cov[(form_of(c), loader_class(c, synthetic_ptrs(c)), planes)].append(c.name)
        if c.reduce:
            cov[("fold", "col_sums_kernel")].append(c.name)
            for tag in ("split-empty", "split-straddle", "split-renumbered"):
                if tag in c.name:
                    cov[(form_of(c), tag)].append(c.name)
        else:
            cov[(form_of(c), "renumbered grid" if grid(c)[3] else "plain grid")].append(c.name)
    cov[("fold", "pw_fold2_kernel")] = [f"{s[2]}+{s[3]}" for s in PAIR_BLOCKS]
    cov[("pair", "direct")] = list(PAIRS)
    return cov


def operand_geometry(n, K, kcont, pad, batch):
    """(rows, ld, batch stride) of an operand with n logical rows."""
    rows, cols = (n, K) if kcont else (K, n)
    ld = cols + pad
    stride = 0 if batch == "shared" else rows * ld + (0 if batch == "own" else int(batch))
    return rows, ld, stride


def geometry(case):
    """The numbers `apn_pw_contract` is called with: (a_batch, lda), (b_batch, ldb), (d_batch, ldd)."""
    _, lda, sa = operand_geometry(case.R, case.K, case.a_kcont, case.a_pad, case.a_batch)
    _, ldb, sb = operand_geometry(case.Q, case.K, case.b_kcont, case.b_pad, case.b_batch)
    ldd = case.Q + case.d_pad
    return (sa, lda), (sb, ldb), (case.R * ldd + case.d_gap, ldd)


def place(values, nbatch, kcont, off=0, pad=0, batch="own"):
    """The logical operand `values` (nbatch or 1 if shared, n, K) as a strided view into a parent buffer whose every
    other element -- the LEAD floats in front, the floats before a moved origin, the ld padding, the gaps between batch
    entries, the LEAD floats behind -- is NaN.  -> (view (nbatch, n, K), batch stride, ld, parent); view.data_ptr() is the
    operand's first element."""
    nb, n, K = values.shape
    assert nb == (1 if batch == "shared" else nbatch)
    rows, ld, stride = operand_geometry(n, K, kcont, pad, batch)
    parent = torch.full((LEAD + off + (nb - 1) * stride + rows * ld + LEAD,), float("nan"), dtype=torch.float32,
                        device=values.device)
    si, sk = (ld, 1) if kcont else (1, ld)
    parent.as_strided((nb, n, K), (stride, si, sk), LEAD + off).copy_(values)
    view = parent.as_strided((nbatch, n, K), (stride, si, sk), LEAD + off)
    return view, stride, ld, parent


def operands(case, a_values, b_values):
    """Both operands of a case placed: ((a view, a_batch, lda), (b view, b_batch, ldb)).  a_values (nbatch or 1, R, K),
    b_values (nbatch or 1, Q, K)."""
    a = place(a_values, case.nbatch, case.a_kcont, case.a_off, case.a_pad, case.a_batch)
    b = place(b_values, case.nbatch, case.b_kcont, case.b_off, case.b_pad, case.b_batch)
    return a[:3], b[:3]


def value_shapes(case):
    return ((1 if case.a_batch == "shared" else case.nbatch, case.R, case.K),
            (1 if case.b_batch == "shared" else case.nbatch, case.Q, case.K))


def output(case, device):
    """-> (view (nbatch or 1 if reduce, R, Q) float32, parent as int32, mask of the parent's elements the view covers);
    the parent is SENTINEL everywhere."""
    _, _, (d_batch, ldd) = geometry(case)
    nz = 1 if case.reduce else case.nbatch
    size = 2 * LEAD + (nz - 1) * d_batch + case.R * ldd
    parent = torch.full((size,), SENTINEL, dtype=torch.int32, device=device)
    shape, strides = (nz, case.R, case.Q), (d_batch, ldd, 1)
    mask = torch.zeros(size, dtype=torch.bool, device=device)
    mask.as_strided(shape, strides, LEAD).fill_(True)
    return parent.view(torch.float32).as_strided(shape, strides, LEAD), parent, mask


def reference(case, a, b, dtype=torch.float64):
    """The product from the same strided views `a` (nbatch, R, K), `b` (nbatch, Q, K): plain torch.einsum in float64, or
    in int64 (on the CPU: integer matrix products exist there only) -> (nbatch or 1 if reduce, R, Q)."""
    if not dtype.is_floating_point:
        a, b = a.cpu(), b.cpu()
    a, b = a.to(dtype), b.to(dtype)
    if case.reduce:
        return torch.einsum("zrk,zqk->rq", a, b).unsqueeze(0)
    return torch.einsum("zrk,zqk->zrq", a, b)


def contracted(case):
    """Terms per output element."""
    return case.K * (case.nbatch if case.reduce else 1)


def exact_range(case):
    """The wide operand's bound: 2047 (two bf16 planes), shrunk where the contraction is so long that sum |a| |b| could
    reach 2^24."""
    return min(WIDE, (2 ** 24 - 1) // (NARROW * contracted(case)))


def exact_inputs(case, wide_a, gen, device="cpu"):
    """Integer-valued float32 operands: one in [-W, W] (two bf16 planes), the other in [-7, 7] (one plane).  Every plane
    product the kernel drops (lo * lo with two planes; the three smallest of nine with three) is then zero and every
    partial sum an integer below 2^24: the float32 result equals the integer one whatever the order of the sums."""
    sa, sb = value_shapes(case)
    W = exact_range(case)
    la, lb = (W, NARROW) if wide_a else (NARROW, W)
    a = torch.randint(-la, la + 1, sa, generator=gen, device=device).float()
    b = torch.randint(-lb, lb + 1, sb, generator=gen, device=device).float()
    return a, b


def float_inputs(case, binades, gen, device="cpu"):
    """Gaussian operands, or (binades) Gaussians each scaled by its own random power of two in 2^-12 .. 2^12."""
    out = []
    for shape in value_shapes(case):
        v = torch.randn(shape, generator=gen, device=device)
        if binades:
            v = v * torch.exp2(torch.randint(-12, 13, shape, generator=gen, device=device).float())
        out.append(v)
    return out


def bf16_planes(x, planes):
    """The kernel's split of a float32 tensor (PwLoader::stage / pw_split_pair): plane p = bf16(remainder), round to
    nearest even, the remainder formed in float32.  -> (list of float32 planes, the remainder left over)."""
    out, rem = [], x.clone()
    for _ in range(planes):
        p = rem.to(torch.bfloat16).float()
        out.append(p)
        rem = rem - p
    return out, rem


def kept_terms(planes):
    """(plane of A, plane of B) of the MFMAs pw_gemm_body's `compute` issues, in its order (small terms first)."""
    return [(1, 1), (0, 2), (2, 0), (0, 1), (1, 0), (0, 0)] if planes == 3 else [(1, 0), (0, 1), (0, 0)]


def emulate(a, b, planes):
    """The kernel's arithmetic on logical operands a (R, K), b (Q, K) in torch: bf16 planes, the plane products it
    keeps, float32 accumulation."""
    pa, _ = bf16_planes(a, planes)
    pb, _ = bf16_planes(b, planes)
    acc = torch.zeros(a.shape[0], b.shape[0], dtype=torch.float32)
    for i, j in kept_terms(planes):
        acc = acc + pa[i] @ pb[j].t()
    return acc


def _float4_readable(ptr, batch, ld, n, K, kcont):
    # pw_vec (k-contiguous) and pw_vec_rows (row-contiguous) of csrc/pointwise.hip
    if kcont:
        return ptr % 16 == 0 and batch % 4 == 0 and ld % 4 == 0 and K % 4 == 0 and n * ld < (1 << 29)
    return ptr % 16 == 0 and batch % 4 == 0 and ld % 4 == 0 and n % 4 == 0 and (K + PW_KC) * ld < (1 << 29)


def synthetic_ptrs(case, base=1 << 20):
    """Operand addresses for a 16-byte aligned parent buffer."""
    return base + 4 * (LEAD + case.a_off), base + 4 * (LEAD + case.b_off)


def loader_class(case, ptrs):
    """Which loads pw_gemm_body takes for the case with operand addresses `ptrs` = (a, b), as the host decides it
    (apn_pw_contract: g.a_vec / g.b_vec from pw_vec / pw_vec_rows; pw_gemm_body: `fast = K % 32 == 0 && a_vec && b_vec`):
    "steady" (the float4 loads of whole chunks), "general4" (the general form with at least one operand flagged
    float4-readable: a k-contiguous one is then read as float4 with its k clamped, a row-contiguous one value by value
    as always in the general form) or "scalar" (neither flagged: every load a single value).
    Used ONLY to assert that the table reaches every class."""
    (sa, lda), (sb, ldb), _ = geometry(case)
    a_vec = _float4_readable(ptrs[0], sa, lda, case.R, case.K, case.a_kcont)
    b_vec = _float4_readable(ptrs[1], sb, ldb, case.Q, case.K, case.b_kcont)
    if case.K % PW_KC == 0 and a_vec and b_vec:
        return "steady"
    return "general4" if a_vec or b_vec else "scalar"


def grid(case, splits=0):
    """(gridDim.x, y, z) of the launch and whether pw_gemm_body renumbers its tiles (gridDim.z a multiple of 8)."""
    gdz = splits if case.reduce else case.nbatch
    return (case.Q + PW_T - 1) // PW_T, (case.R + PW_T - 1) // PW_T, gdz, gdz % 8 == 0


def split_plan(nbatch, K, splits):
    """What `splits` shares make of the (batch entry, chunk) range: (chunks per share, shares that get no chunk, shares
    whose chunks lie in more than one batch entry)."""
    cpb = (K + PW_KC - 1) // PW_KC
    total = nbatch * cpb
    cps = (total + splits - 1) // splits
    empty = straddling = 0
    for z in range(splits):
        c0, c1 = z * cps, min((z + 1) * cps, total)
        if c0 >= c1:
            empty += 1
        elif c0 // cpb != (c1 - 1) // cpb:
            straddling += 1
    return cps, empty, straddling


def form_of(case):
    return _form_name((case.a_kcont, case.b_kcont))
