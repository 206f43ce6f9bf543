"""Mirror of the reference's ``utils/tools/nn_distance.py``: the custom op on dmcf_nn_distance, differentiable in both point
sets (dmcf_nn_distance_backward), and the Chamfer loss built on it (nn_distance.py:141-148).  ``nn_distance`` also takes
``row_splits1`` / ``row_splits2``: a batch of point sets of different sizes in one call (dmcf_nn_distance_ragged, no gradient)."""
import torch

from ... import ops

nn_distance = ops.nn_distance


def chamfer_loss(y_true, y_pred):
    """nn_distance.py:141-148: ``mean(dist(y_pred -> y_true)) + mean(dist(y_true -> y_pred))`` per batch item, [b]; [n, 3]
    inputs are treated as one batch item."""
    if y_true.dim() == 2:
        y_true = y_true.unsqueeze(0)
    if y_pred.dim() == 2:
        y_pred = y_pred.unsqueeze(0)
    cost_p1_p2, _, cost_p2_p1, _ = nn_distance(y_pred, y_true)
    return torch.mean(cost_p1_p2, dim=-1) + torch.mean(cost_p2_p1, dim=-1)


__all__ = ["nn_distance", "chamfer_loss"]
