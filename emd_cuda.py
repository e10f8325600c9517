"""Drop-in for the reference's compiled `emd_cuda` module: its three functions on csrc/emd.hip, so that the reference's
`openpoints/cpp/emd/emd.py` (`import emd_cuda`) runs unmodified.  `adaptpoint_amd.emd` has the same functions, and an
`EarthMoverDistanceFunction` that never materialises the (B,m,n) `match` these three pass between them."""
from adaptpoint_amd.emd import approxmatch_forward, matchcost_backward, matchcost_forward

__all__ = ["approxmatch_forward", "matchcost_forward", "matchcost_backward"]
