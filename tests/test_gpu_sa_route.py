"""Every row of tests/sa_route_table.py on the device: which entry point the block's forward reaches, whether the
residual branch went into the kernels, what the index stage (`sample` + `index_for`) built, and which fallback was
recorded -- against the table."""
import inspect

import pytest
import torch

from sa_route_table import ROWS


def _record(monkeypatch):
    """Wrap the entry point of every path; returns the list of (entry, residual branch fused) calls."""
    from adaptpoint_amd import fused, fused_wide, pointwise
    hits = []

    def wrap(mod, name, tag, skip_param=None):
        orig = getattr(mod, name)
        sig = inspect.signature(orig)

        def fn(*a, **k):
            skip = skip_param is not None and sig.bind(*a, **k).arguments.get(skip_param) is not None
            hits.append((tag, skip))
            return orig(*a, **k)
        monkeypatch.setattr(mod, name, fn)
    wrap(fused, "fused_set_abstraction", "resident", "skip_conv")
    wrap(fused_wide, "block", "wide", "skip_conv")
    wrap(fused, "grouped_mlp_max", "grouped")
    wrap(fused_wide, "grouped_mlp_max", "grouped-wide")
    wrap(pointwise, "run_block", "pointwise")
    return hits


def _path(blk, hits):
    tags = [t for t, _ in hits]
    for tag, path in (("resident", ("resident", False)), ("wide", ("wide", True)), ("grouped", ("grouped", False)),
                      ("grouped-wide", ("grouped", True))):
        if tag in tags:
            return path + (any(s for t, s in hits if t == tag),)
    if "pointwise" in tags and (blk.is_head or blk.all_aggr):
        return ("stem" if blk.is_head else "group_all", False, False)
    return ("composed", False, False)


def _built(smp):
    return tuple(n for n, v in (("geo", smp.geo), ("tmap", smp.tmap), ("rowmap", smp.rowmap), ("index", smp.index),
                                ("fq", None if smp.index is None else smp.index.fq)) if v is not None)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(ROWS))
def test_route_table_on_the_device(dev, name, monkeypatch):
    from adaptpoint_amd import fused, layers, synthetic as GI
    from adaptpoint_amd import set_abstraction as SA
    make, (c_in, B, N), prefer_wide, sampled, cuda, expected = ROWS[name]
    monkeypatch.setattr(SA, "PREFER_WIDE", prefer_wide)
    d = dev if cuda else torch.device("cpu")
    torch.manual_seed(0)
    blk = make().to(d).train()
    p = torch.from_numpy(GI.unit_sphere_cloud(B, N, seed=3)).to(d)
    f = torch.randn(B, c_in, N, device=d)
    smp, built = None, ()
    ball = not (blk.is_head or blk.all_aggr)
    if ball and cuda and sampled:
        # an index stage handed in for a cloud beyond the resident samplers: the unfused operators' own
        M, g = N // blk.stride, blk.grouper
        smp = fused.Sampling(B, M, g.nsample, d)
        smp.fidx.copy_(layers.furthest_point_sample(p, M))
        smp.new_p.copy_(torch.gather(p, 1, smp.fidx.long().unsqueeze(-1).expand(-1, -1, 3)))
        smp.idx.copy_(g.neighbours(smp.new_p, p))
        blk.index_for(smp, N, c_in)
        built = _built(smp)
    elif ball and cuda and N <= SA.MAX_SAMPLE_SEQ_POINTS:
        s = blk.sample(p)
        blk.index_for(s, N, c_in)
        built = _built(s)
    hits = _record(monkeypatch)
    before = dict(SA.FUSED_FALLBACKS)
    if cuda:
        blk([p, f], sampling=smp)
    else:
        from oracle import cpu_block as CB
        with CB.CpuOps():
            blk([p, f])
    torch.cuda.synchronize()
    new = {k: v - before.get(k, 0) for k, v in SA.FUSED_FALLBACKS.items() if v != before.get(k, 0)}
    path, wide, skip = _path(blk, hits)
    reason = next(iter(new)) if new else None
    assert len(new) <= 1 and all(v == 1 for v in new.values()), new
    assert (path, wide, skip, built, reason) == expected
