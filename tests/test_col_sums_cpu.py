"""tests/col_sums_reference.py -- the restatement of csrc/col_sums.hip's order that tests/test_gpu_col_sums.py compares the
kernel with bit for bit -- checked on the CPU: it is a sum, at four lanes it is the formula the four-lane folds have always
used, and it can tell one lane count from another."""
import pytest
import torch

from col_sums_reference import LANES, col_sums_ref, order_data

ROWS = [0, 1, 3, 4, 5, 15, 16, 17, 33, 2048]


@pytest.mark.parametrize("lanes", LANES)
def test_small_integers_give_the_plain_sum(lanes):
    gen = torch.Generator().manual_seed(lanes)
    for rows in ROWS:
        part = torch.randint(-1000, 1001, (rows, 37), generator=gen).double()
        assert torch.equal(col_sums_ref(part, lanes), part.sum(0)), rows
        assert torch.equal(col_sums_ref(part.float(), lanes, torch.float32), part.sum(0).float()), rows
        tail = col_sums_ref(part, lanes, tail_count=7.0)
        assert torch.equal(tail[:-2], part.sum(0)) and tail[-2:].tolist() == [7.0, 1.0]


@pytest.mark.parametrize("rows", ROWS[1:])
def test_four_lanes_are_the_interleaved_pairwise_formula(rows):
    """(r0 + r1) + (r2 + r3) with r_l = the rows l, l + 4, ... added in ascending order from +0, written out directly:
    what apn_la_stats_fold and the split-K folds computed before they shared a kernel."""
    part = order_data(rows, 65, seed=rows)
    for values, out_dtype in ((part, torch.float64), (part.float(), torch.float32)):
        r = []
        for lane in range(4):
            s = torch.zeros(65, dtype=torch.float64)
            for k in range(lane, rows, 4):
                s += values[k].double()
            r.append(s)
        assert torch.equal(col_sums_ref(values, 4, out_dtype), ((r[0] + r[1]) + (r[2] + r[3])).to(out_dtype))


def test_the_order_shows_in_the_bits():
    """One column whose float64 sum depends on the association: 2^53 swallows a lone 1 but not a 2.  The three lane
    counts give three different results, and seeded order data tell them apart as well."""
    big = 2.0 ** 53
    col = torch.tensor([big, 1.0, 1.0, -big] + [1.0] * 29, dtype=torch.float64).view(-1, 1)       # the exact sum: 31
    got = {lanes: float(col_sums_ref(col, lanes)) for lanes in LANES}
    assert got == {4: 23.0, 8: 27.0, 16: 29.0}, got             # lane 0 drops every 1 it meets behind 2^53: 8, 4, 2 of them
    part = order_data(33, 64, seed=5)
    res = [col_sums_ref(part, lanes) for lanes in LANES]
    assert not torch.equal(res[0], res[1]) and not torch.equal(res[1], res[2]) and not torch.equal(res[0], res[2])
    for x in res:
        assert torch.allclose(x, part.sum(0), rtol=0, atol=float(part.abs().sum(0).max()) * 33 * 2.0 ** -53)
