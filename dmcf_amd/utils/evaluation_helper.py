"""Validation metrics of ``Simulator.run_valid`` -- mirror of the reference's ``utils/evaluation_helper.py`` (same names and
arguments):

  distance          :14-16  per-point Euclidean distance (host numpy)
  chamfer_distance  :25-28  for each point of ``gt`` the distance to its nearest point of ``pred``; on the GPU through
                            ops.nn_distance (dmcf_nn_distance) instead of a host cKDTree; with row splits, a
                            batch of scenes of different sizes in one call (dmcf_nn_distance_ragged)
  compare_dist      :43-75  KL divergence of two histograms (one bin per ``bin_size`` points, 1e-5 prior); host numpy,
                            vectorised, the same value as the reference's per-point loop.  compare_dist_pair: both
                            directions for a batch of scenes from one GPU call (dmcf_hist_pair_ragged), the same bits
  merge_dicts       :78-85

``optimal_assignment_distance`` and ``compute_stats`` are not used by run_valid and are not rebuilt.
"""
import numpy as np
import torch


def _host(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def distance(x, y):
    """:14-16: ``|x - y|`` along the last axis."""
    return np.linalg.norm(_host(x) - _host(y), axis=-1)


def chamfer_distance(pred, gt, pred_row_splits=None, gt_row_splits=None):
    """:25-28: for each point of ``gt`` [n, 3] the Euclidean distance to its nearest point of ``pred`` [m, 3], as a float32
    numpy array [n].  Numpy arrays or device tensors; the nearest neighbours come from ops.nn_distance on the GPU (float32
    squared distances, then the square root), where the reference queries a cKDTree in float64.

    ``pred_row_splits`` / ``gt_row_splits`` (both or neither, the rules of ops.nn_distance): a batch of scenes of different
    sizes, ``pred`` [m_total, 3] and ``gt`` [n_total, 3] holding them one after the other.  One kernel call
    (dmcf_nn_distance_ragged, the gt -> pred direction only) and one host copy for the whole batch; returns the concatenated
    distances [n_total], which the caller slices by ``gt_row_splits``: every slice has the bits of the per-scene call."""
    from .. import ops
    if pred_row_splits is not None or gt_row_splits is not None:  # (host checks before anything goes to the device)
        ops.nn_distance_row_splits(tuple(gt.shape), tuple(pred.shape), gt_row_splits, pred_row_splits)
    dev = next((t.device for t in (pred, gt) if isinstance(t, torch.Tensor) and t.is_cuda), torch.device("cuda"))

    def to_dev(x):
        if isinstance(x, torch.Tensor):
            return x.detach().to(dev, dtype=torch.float32)
        return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)

    if pred_row_splits is not None:
        d_gt = ops.nn_distance_ragged(to_dev(gt), to_dev(pred), gt_row_splits, pred_row_splits, want2=False)[0]
    else:
        d_gt, _, _, _ = ops.nn_distance(to_dev(gt), to_dev(pred))
    return torch.sqrt(d_gt).cpu().numpy()


def compare_dist(x, y, bin_size=25):
    """:43-75: histogram both point sets (e.g. velocities) [cnt, dim] on the same grid -- bin_cnt = cnt // bin_size bins in all,
    int(bin_cnt ** (1 / dim)) per axis between the 5th and 95th percentiles of both, clipped at the edges, every bin starting at
    1e-5 -- and return the KL divergence KL(x || y) of the two normalised histograms (scipy.stats.entropy(bins_x, bins_y))."""
    x, y = _host(x), _host(y)
    assert x.shape == y.shape
    cnt = x.shape[0]
    dim = x.shape[-1]
    bin_cnt = cnt // bin_size
    bin_cnt_per_dim = int(bin_cnt ** (1 / dim))
    both = np.concatenate((x, y), axis=0)
    min_v = np.percentile(both, 5, axis=0)
    max_v = np.percentile(both, 95, axis=0)
    bin_w = (max_v - min_v + 1e-6) / bin_cnt_per_dim
    shape = (bin_cnt_per_dim + 1,) * dim

    def hist(v):
        idx = np.clip(((v - min_v) / bin_w).astype("int32"), 0, bin_cnt_per_dim)
        flat = np.ravel_multi_index(tuple(idx.T), shape) if len(idx) else np.zeros(0, dtype=np.int64)
        return np.bincount(flat, minlength=int(np.prod(shape)))

    return _kl_from_counts(hist(x), hist(y))


def _kl_from_counts(cx, cy):
    """The end of :func:`compare_dist`: the bin counts of both sets (any integer or float arrays of one shape) -> KL(x || y) of
    the two histograms, every bin starting at 1e-5, both normalised (float64)."""
    px, py = np.asarray(cx).astype(np.float64) + 1e-5, np.asarray(cy).astype(np.float64) + 1e-5
    px, py = px / px.sum(), py / py.sum()
    return float(np.sum(px * np.log(px / py)))


def compare_dist_pair(x, y, bin_size=25, row_splits=None):
    """Both directions of :func:`compare_dist` for a batch of scenes: ``(kl_xy [batch], kl_yx [batch])``, float64 numpy arrays
    with ``kl_xy[b] == compare_dist(x_b, y_b, bin_size)`` and ``kl_yx[b] == compare_dist(y_b, x_b, bin_size)`` bit for bit.

    ``x`` and ``y`` [n_total, 3] (float32; numpy arrays or device tensors) share ``row_splits`` (None: one item).  The
    percentiles and the histograms come from ONE ops.hist_pair_ragged call on the GPU -- both directions use the same
    percentiles and the same two histograms -- and reach the host in one copy of the integer counts; the KL sums are
    :func:`_kl_from_counts`, the host function's own last lines, so equal counts give equal bits.  Finite inputs only."""
    from .. import ops
    dev = next((t.device for t in (x, y) if isinstance(t, torch.Tensor) and t.is_cuda), torch.device("cuda"))

    def to_dev(v):
        return v.detach().to(dev) if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(v)).to(dev)

    _, counts, offsets = ops.hist_pair_ragged(to_dev(x), to_dev(y), row_splits, bin_size)
    return _kl_pairs(counts.cpu().numpy(), offsets)


def _kl_pairs(counts, offsets):
    """Host counts in the layout of ops.hist_pair_ragged -> (KL(x || y) [batch], KL(y || x) [batch])."""
    kl_xy, kl_yx = np.empty(len(offsets) - 1), np.empty(len(offsets) - 1)
    for b in range(len(offsets) - 1):
        mid = (offsets[b] + offsets[b + 1]) // 2
        cx, cy = counts[offsets[b]:mid], counts[mid:offsets[b + 1]]
        kl_xy[b], kl_yx[b] = _kl_from_counts(cx, cy), _kl_from_counts(cy, cx)
    return kl_xy, kl_yx


def merge_dicts(dicts, op, start_val=0):
    """:78-85: fold the values of equal keys with ``op``, starting from ``start_val``."""
    output = {}
    for d in dicts:
        for k, v in d.items():
            if k not in output:
                output[k] = start_val
            output[k] = op(output[k], v)
    return output
