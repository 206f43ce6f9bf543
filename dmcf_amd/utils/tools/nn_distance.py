"""Mirror of the reference's ``utils/tools/nn_distance.py``: the custom op on dmcf_nn_distance, differentiable in both point
sets (dmcf_nn_distance_backward), and the Chamfer loss built on it (nn_distance.py:141-148).  ``nn_distance`` also takes
``row_splits1`` / ``row_splits2``: a batch of point sets of different sizes in one call (dmcf_nn_distance_ragged, no gradient);
``chamfer_loss`` takes row splits too, and with ``record=True`` it trains through that one call."""
import torch

from ... import ops

nn_distance = ops.nn_distance


def _item_means(dist, splits):
    """[batch]: the mean of every item's rows of ``dist`` (0 for an item without rows).  Each mean is torch.mean over a copy of
    the item's rows, the reduction the un-batched chamfer_loss runs on its own [1, n] distances, so it has that call's bits (a
    segmented sum would add in another order)."""
    zero = dist.new_zeros(())
    return torch.stack([torch.mean(dist[a:b].clone().unsqueeze(0), dim=-1)[0] if b > a else zero for a, b in zip(splits, splits[1:])])


def chamfer_loss(y_true, y_pred, true_row_splits=None, pred_row_splits=None, record=False):
    """nn_distance.py:141-148: ``mean(dist(y_pred -> y_true)) + mean(dist(y_true -> y_pred))`` per batch item, [b]; [n, 3]
    inputs are treated as one batch item.

    ``true_row_splits`` / ``pred_row_splits`` (both or neither): a RAGGED batch, ``y_true`` [n_total, 3|2] and ``y_pred``
    [m_total, 3|2], in one nn_distance call (dmcf_nn_distance_ragged) -> [batch], entry b being what chamfer_loss returns for
    item b alone, bit for bit.  An item with both sets empty gives 0, one with exactly one empty set is nn_distance's
    ValueError.  ``record=True``: differentiable in both sets (ops.nn_distance_ragged records; one dmcf_nn_distance_backward
    call for the batch), every item's gradient rows with the bits of the loss on the item alone; without it inputs that require
    grad raise NotImplementedError, as ops.nn_distance with row splits does."""
    if true_row_splits is not None or pred_row_splits is not None:
        cost_p1_p2, _, cost_p2_p1, _ = ops.nn_distance_ragged(y_pred, y_true, pred_row_splits, true_row_splits, record=record)
        sp = ops._host_row_splits(pred_row_splits, "pred_row_splits")[0]
        st = ops._host_row_splits(true_row_splits, "true_row_splits")[0]
        return _item_means(cost_p1_p2, sp) + _item_means(cost_p2_p1, st)
    if y_true.dim() == 2:
        y_true = y_true.unsqueeze(0)
    if y_pred.dim() == 2:
        y_pred = y_pred.unsqueeze(0)
    cost_p1_p2, _, cost_p2_p1, _ = nn_distance(y_pred, y_true)
    return torch.mean(cost_p1_p2, dim=-1) + torch.mean(cost_p2_p1, dim=-1)


__all__ = ["nn_distance", "chamfer_loss"]
