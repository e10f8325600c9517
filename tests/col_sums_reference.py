"""csrc/col_sums.hip's summation order (include/adaptpoint_amd.h, "Partial-row folds") restated in plain torch float64:
lane l of a column adds the rows l, l + lanes, l + 2 lanes, ... one after the other into one accumulator that starts at
+0; the lanes' sums are then combined by an adjacent-pair tree, (0+1), (2+3), ..., then pairs of those.  Every add is one
IEEE float64 add on a whole row of columns, so the result carries the kernel's bits.  Imports without a GPU."""
import torch

LANES = (4, 8, 16)


def order_data(rows, ncol, seed):
    """Seeded float64 values of mixed sign spanning about 40 binades: almost every reassociation of a column's sum
    changes its last bits."""
    gen = torch.Generator().manual_seed(seed)
    v = torch.randn(rows, ncol, generator=gen, dtype=torch.float64)
    return v * torch.exp2(torch.randint(-20, 21, (rows, ncol), generator=gen).double())


def col_sums_ref(part, lanes, out_dtype=torch.float64, tail_count=None):
    """part (rows, ncol), float32 or float64 -> (ncol,) of out_dtype, or (ncol + 2,) ending in {tail_count, 1}.  A float32
    result is the float64 total rounded once."""
    assert lanes in LANES and part.dim() == 2
    rows, ncol = part.shape
    part = part.detach().cpu().double()
    sums = []
    for lane in range(lanes):
        s = torch.zeros(ncol, dtype=torch.float64)
        for r in range(lane, rows, lanes):
            s = s + part[r]
        sums.append(s)
    while len(sums) > 1:
        sums = [sums[i] + sums[i + 1] for i in range(0, len(sums), 2)]
    out = sums[0]
    if tail_count is not None:
        out = torch.cat([out, torch.tensor([float(tail_count), 1.0], dtype=torch.float64)])
    return out.to(out_dtype)
