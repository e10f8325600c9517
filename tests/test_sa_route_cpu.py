"""`set_abstraction.route` on plain values, without a device: every row of tests/sa_route_table.py."""
import pytest

from sa_route_table import RESIDENT_INDEX, ROWS, block


def _index_stage(r):
    """What `sample` + `index_for` build for a route (see SetAbstraction.sample / index_for)."""
    from adaptpoint_amd import set_abstraction as SA
    if r.path == SA.RESIDENT:
        return RESIDENT_INDEX
    if r.path == SA.WIDE:
        return ("index", "fq") if r.fuse_skip else ("index",)
    return ()


@pytest.mark.parametrize("name", sorted(ROWS))
def test_route_table(name):
    from adaptpoint_amd import set_abstraction as SA
    make, (c_in, B, N), prefer_wide, sampling, cuda, expected = ROWS[name]
    plan = make().plan()
    momenta = (plan.mlp[1].momentum, plan.mlp[3].momentum) if plan.mlp is not None else ()
    r = SA.route(plan, c_in, B, N, cuda, momenta, prefer_wide, sampling)
    assert (r.path, r.wide, r.fuse_skip, _index_stage(r), r.reason) == expected


def test_route_reads_the_block_as_it_stands(monkeypatch):
    """SetAbstraction.route reads PREFER_WIDE and the momenta at the call (tests flip them at run time), and a block
    built with fused=False takes the composed path without recording a fallback."""
    from adaptpoint_amd import set_abstraction as SA
    blk = block(32, 64)
    assert blk.route(32, 32, 1024)[1].path == SA.RESIDENT
    monkeypatch.setattr(SA, "PREFER_WIDE", True)
    assert blk.route(32, 32, 1024)[1].path == SA.WIDE
    blk.convs[1][1].momentum = None
    assert blk.route(32, 32, 1024)[1].path == SA.COMPOSED
    blk.fused = False
    assert blk.route(32, 32, 1024)[1] == SA.Route(SA.COMPOSED)
    assert not blk.plan().fused and blk.plan().mlp is not None
