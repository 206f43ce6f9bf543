"""Mirror of the reference's ``utils/tools/sampling.py``: ``farthest_point_sample`` (no gradient) and ``gather_point``
(differentiable in ``inp``, dmcf_gather_point_backward)."""
from ... import ops

farthest_point_sample = ops.farthest_point_sample
gather_point = ops.gather_point

__all__ = ["farthest_point_sample", "gather_point"]
