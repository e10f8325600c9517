"""csrc/col_sums.hip -- the one fold of the workgroups' partial rows -- through the entries that launch it:

    apn_la_stats_fold   4 lanes, float64 -> float64, with the {count, 1} tail
    apn_ag_fold         4 lanes, float64 -> float64
    apn_pt_fold         16 lanes, float64 -> float64
    apn_pw_contract     4 lanes, float32 -> float32 (splits > 0: the shares stay in `scratch`, so the fold is checked on them)
    apn_rl_moments      8 lanes, float64 -> float64 (adaptpoint_amd.randla.encoding_moments, and raw for its shares)

at the row and column counts where the indexing can go wrong: around the lane count, around the 16 / 32 / 64 columns of
a workgroup, one column, more than one workgroup, no rows (where the entry writes), apn_pt_fold's limit of 2048 rows.

  exact     small integers: the result EQUALS part.sum(0) (and the tail {count, 1});
  order     float64 values over ~40 binades, mixed signs: the result EQUALS tests/col_sums_reference.py's restatement of
            the shared order, bit for bit (tests/test_col_sums_cpu.py checks the restatement);
  redzone   every output lies in a sentinel-filled parent whose margins must not change, every input in a NaN-filled
            one: a read outside it would show in the exact sums.
"""
import functools

import pytest
import torch

from attention_cases import LEAD, SENTINEL, borders_intact, in_sentinel_parent
from col_sums_reference import col_sums_ref, order_data

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
ROWS = [0, 1, 3, 4, 5, 15, 16, 17, 33]
NCOL = [1, 15, 16, 17, 63, 64, 65, 130]


def _call(name, dev, *args):
    from adaptpoint_amd.fused import _call as call
    call(name, dev, *args)


def _inside_nan(dev, t):
    """A contiguous copy of `t` inside a NaN-filled parent of its dtype (16-byte aligned)."""
    parent = torch.full((t.numel() + 2 * LEAD,), float("nan"), dtype=t.dtype, device=dev)
    view = parent[LEAD:LEAD + t.numel()].view(t.shape)
    view.copy_(t)
    return view


def _folded(dev, entry, part, count=5.0):
    """One fold launch of `part` (rows, ncol) float64 through `entry` -> the result on the CPU; the redzone is checked."""
    rows, ncol = part.shape
    n_out = ncol + 2 if entry == "la" else ncol
    view, parent = in_sentinel_parent(8 * n_out, dev)
    src = _inside_nan(dev, part)
    if entry == "la":
        assert ncol % 2 == 0
        _call("apn_la_stats_fold", dev, src.data_ptr(), rows, ncol // 2, float(count), view.data_ptr())
    elif entry == "ag":
        _call("apn_ag_fold", dev, rows, ncol, src.data_ptr(), view.data_ptr())
    else:
        _call("apn_pt_fold", dev, src.data_ptr(), rows, ncol, view.data_ptr())
    assert borders_intact(parent), f"{entry} {rows} x {ncol}: a sentinel outside the output changed"
    assert bool((view.view(torch.int64) != (SENTINEL << 32 | SENTINEL)).all()), f"{entry} {rows} x {ncol}: a part of the output was never written"
    return view.view(F64).cpu()


@functools.lru_cache(maxsize=None)
def _data(rows, ncol):
    """(small integers, order data, their exact sum) of one shape, made once."""
    gen = torch.Generator().manual_seed(1000 * rows + ncol)
    ints = torch.randint(-1000, 1001, (rows, ncol), generator=gen).double()
    return ints, order_data(rows, ncol, seed=7 * rows + ncol), ints.sum(0)


@functools.lru_cache(maxsize=None)
def _ref(rows, ncol, lanes):
    return col_sums_ref(_data(rows, ncol)[1], lanes)


ENTRIES = [("la", 4, [r for r in ROWS if r > 0]),             # rows == 0: returns before it writes
           ("ag", 4, ROWS),
           ("pt", 16, ROWS + [2048])]
CASES = [(e, lanes, rows) for e, lanes, rr in ENTRIES for rows in rr]


@pytest.mark.parametrize("entry,lanes,rows", CASES, ids=[f"{e}-{r}" for e, _, r in CASES])
def test_fold_entries_exact_and_in_the_shared_order(dev, entry, lanes, rows):
    for n in NCOL:
        ncol = 2 * n if entry == "la" else n                 # apn_la_stats_fold folds 2 c columns
        ints, order, total = _data(rows, ncol)
        got = _folded(dev, entry, ints)
        want = _ref(rows, ncol, lanes)
        if entry == "la":
            assert got[-2:].tolist() == [5.0, 1.0], (ncol, got[-2:])
            assert _folded(dev, entry, ints, count=0.0)[-2:].tolist() == [0.0, 1.0]
            got = got[:-2]
        assert torch.equal(got, total), (ncol, "integers")
        got = _folded(dev, entry, order)
        assert torch.equal(got[:ncol], want), (ncol, "order", float((got[:ncol] - want).abs().max()))


def test_la_stats_fold_without_rows_writes_nothing(dev):
    view, parent = in_sentinel_parent(8 * 34, dev)
    _call("apn_la_stats_fold", dev, None, 0, 16, 5.0, view.data_ptr())
    assert bool((parent == SENTINEL).all())


@pytest.mark.parametrize("splits", [1, 3, 4, 5, 17, 33])
def test_split_k_fold_of_float32_shares(dev, splits):
    """apn_pw_contract with `splits` shares (any count is legal: the trailing ones are empty and hold zeros): d == the
    restatement's four-lane float32 fold of the shares the launch left in scratch, and -- integer operands -- the exact
    product.  20 chunks of K over the shares; r x q = the column counts."""
    nb, K = 4, 160
    gen = torch.Generator().manual_seed(splits)
    for R, Q in [(1, 1), (3, 5), (4, 4), (1, 17), (7, 9), (8, 8), (5, 13), (10, 13)]:
        for exact in (True, False):
            if exact:
                a = torch.randint(-2047, 2048, (nb, R, K), generator=gen).float()
                b = torch.randint(-7, 8, (nb, Q, K), generator=gen).float()
            else:
                a, b = order_data(nb * R, K, seed=R + splits).float().view(nb, R, K), torch.randn(nb, Q, K, generator=gen)
            a, b = _inside_nan(dev, a), _inside_nan(dev, b)
            scratch = torch.full((splits, R * Q), float("nan"), device=dev)
            view, parent = in_sentinel_parent(4 * R * Q, dev)
            _call("apn_pw_contract", dev, nb, R, Q, K, a.data_ptr(), R * K, K, 1, b.data_ptr(), Q * K, K, 1, view.data_ptr(),
                  0, Q, splits, scratch.data_ptr(), 3)
            assert borders_intact(parent), (R, Q, "a sentinel outside the output changed")
            got = view.view(F32).cpu()
            assert torch.equal(got, col_sums_ref(scratch, 4, F32)), (R, Q, exact)
            if exact:
                want = torch.einsum("zrk,zqk->rq", a.cpu().double(), b.cpu().double())
                assert float(want.abs().max()) < 2 ** 24 and torch.equal(got.double(), want.reshape(-1)), (R, Q)


def test_randla_moments_at_eight_lanes(dev):
    """Nine partial rows (3 x 350 x 16 pairs, 2048 per row).  On a lattice the 65 moments are sums of integers: equal to
    the float64 statement, as tests/test_gpu_randla.py asks; on uniform coordinates mom is the eight-lane fold of the
    rows apn_rl_moments left in `part`, bit for bit."""
    import randla_reference as R
    from adaptpoint_amd import _lib
    from adaptpoint_amd.randla import encoding_moments
    B, N, K = 3, 350, 16
    rows = _lib.load().apn_rl_moment_rows(B, N, K)
    assert rows == 9
    t = R.tensors(R.layer_inputs(B, N, K, 8, seed=17, integer=True), dev, F32)
    mom = encoding_moments(t['coords'], t['idx'], t['dist'], False)
    flat = R.encoding(t['coords'].double(), t['idx'], t['dist'].double()).permute(1, 0, 2, 3).reshape(10, -1)
    second = flat @ flat.t()
    assert torch.equal(mom, torch.cat([flat.sum(1)] + [second[i, i:] for i in range(10)]))
    t = R.tensors(R.layer_inputs(B, N, K, 8, seed=18), dev, F32)
    part = torch.full((rows, 65), float("nan"), dtype=F64, device=dev)
    view, parent = in_sentinel_parent(8 * 65, dev)
    _call("apn_rl_moments", dev, B, N, K, t['coords'].data_ptr(), t['idx'].data_ptr(), t['dist'].data_ptr(), 0,
          part.data_ptr(), view.data_ptr())
    assert borders_intact(parent)
    assert torch.equal(view.view(F64).cpu(), col_sums_ref(part, 8))
