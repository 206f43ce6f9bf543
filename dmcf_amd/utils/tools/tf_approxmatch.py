"""Mirror of the reference's ``utils/tools/tf_approxmatch.py``: ``approx_match`` (no gradient, as NoGradient('ApproxMatch'))
and ``match_cost`` (differentiable in both point sets, dmcf_match_cost_backward; the match is a constant)."""
from ... import ops

approx_match = ops.approx_match
match_cost = ops.match_cost

__all__ = ["approx_match", "match_cost"]
