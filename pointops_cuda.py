"""Drop-in for the reference's compiled `pointops_cuda` module: its eleven functions on csrc/pointops.hip, with the
reference's names, argument order and in-place outputs, so that the reference's
`openpoints/cpp/pointops/functions/pointops.py` (`import pointops_cuda`) runs unmodified.  `adaptpoint_amd.pointops`
has the same functions and the reference's Functions without their `.zero_()` calls."""
from adaptpoint_amd.pointops import (aggregation_backward_cuda, aggregation_forward_cuda, ballquery_cuda,
                                     furthestsampling_cuda, grouping_backward_cuda, grouping_forward_cuda,
                                     interpolation_backward_cuda, interpolation_forward_cuda, knnquery_cuda,
                                     subtraction_backward_cuda, subtraction_forward_cuda)

__all__ = ["knnquery_cuda", "ballquery_cuda", "furthestsampling_cuda", "grouping_forward_cuda", "grouping_backward_cuda",
           "interpolation_forward_cuda", "interpolation_backward_cuda", "subtraction_forward_cuda",
           "subtraction_backward_cuda", "aggregation_forward_cuda", "aggregation_backward_cuda"]
