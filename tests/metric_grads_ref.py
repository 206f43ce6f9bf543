"""Float64 restatement of the gradients of the point-cloud ops (dmcf_amd/csrc/metrics_bwd.hip), written from the formulas of
the ops' contract, for the metric-gradient tests.  Each function returns the gradient and A, the same sum taken over the
absolute values of its terms: the scale of the element-wise error bar (16 2^-24 A).

  nn_distance_grad(xyz1, xyz2, g1, g2)       of sum g1 . dist1 + g2 . dist2 with the nearest-neighbour indices held fixed
  match_cost_grad(xyz1, xyz2, match, g)      of sum_b g_b match_cost_b with the match held fixed
  gather_point_grad(grad_out, idx, n_inp)    of sum grad_out . gather_point(inp, idx)

plus nn_distance / chamfer / match_cost values for finite differences.  The match comes from tests/metrics_ref.py."""
import numpy as np

import metrics_ref as R


def _f64(x):
    return R._pad3(np.asarray(x, np.float64))


def nn_distance_grad(xyz1, xyz2, g1=None, g2=None, idx1=None, idx2=None):
    """-> (grad1 [b, n, 3], grad2 [b, m, 3], A1, A2).  idx1 / idx2: the indices to hold (default: the float64 nearest)."""
    x1, x2 = _f64(xyz1), _f64(xyz2)
    if idx1 is None or idx2 is None:
        _, i1, _, i2 = R.nn_distance(x1, x2)
        idx1 = i1 if idx1 is None else idx1
        idx2 = i2 if idx2 is None else idx2
    b, n, m = x1.shape[0], x1.shape[1], x2.shape[1]
    gr1, gr2 = np.zeros((b, n, 3)), np.zeros((b, m, 3))
    a1, a2 = np.zeros((b, n, 3)), np.zeros((b, m, 3))
    for i in range(b):
        if g1 is not None:
            t = 2.0 * np.asarray(g1[i], np.float64)[:, None] * (x1[i] - x2[i][idx1[i]])
            gr1[i] += t
            a1[i] += np.abs(t)
            np.add.at(gr2[i], idx1[i], -t)
            np.add.at(a2[i], idx1[i], np.abs(t))
        if g2 is not None:
            t = 2.0 * np.asarray(g2[i], np.float64)[:, None] * (x2[i] - x1[i][idx2[i]])
            gr2[i] += t
            a2[i] += np.abs(t)
            np.add.at(gr1[i], idx2[i], -t)
            np.add.at(a1[i], idx2[i], np.abs(t))
    return gr1, gr2, a1, a2


def match_cost_grad(xyz1, xyz2, match, g=None):
    """-> (grad1 [b, n, 3], grad2 [b, m, 3], A1, A2) for match [b, m, n] and g [b] (default ones)."""
    x1, x2 = _f64(xyz1), _f64(xyz2)
    b = x1.shape[0]
    g = np.ones(b) if g is None else np.asarray(g, np.float64)
    out = [[], [], [], []]
    for i in range(b):
        mt = np.asarray(match[i], np.float64).T                        # [n, m]
        diff = x1[i][:, None, :] - x2[i][None, :, :]                   # [n, m, 3]
        d = np.sqrt(np.maximum((diff ** 2).sum(-1), 1e-20))
        t = g[i] * (mt / d)[:, :, None] * diff
        out[0].append(t.sum(1))
        out[1].append(-t.sum(0))
        out[2].append(np.abs(t).sum(1))
        out[3].append(np.abs(t).sum(0))
    return tuple(np.stack(o) for o in out)


def gather_point_grad(grad_out, idx, n_inp):
    """-> (grad_inp [n_inp, c], A) for grad_out [m, c] and idx [m] (repeated indices sum)."""
    go = np.asarray(grad_out, np.float64)
    gi, a = np.zeros((n_inp, go.shape[1])), np.zeros((n_inp, go.shape[1]))
    np.add.at(gi, np.asarray(idx), go)
    np.add.at(a, np.asarray(idx), np.abs(go))
    return gi, a


def nn_distance_value(xyz1, xyz2, g1, g2, idx1, idx2):
    """sum g1 . dist1 + g2 . dist2 with the indices held (for finite differences)."""
    x1, x2 = _f64(xyz1), _f64(xyz2)
    v = 0.0
    for i in range(x1.shape[0]):
        v += (np.asarray(g1[i]) * ((x1[i] - x2[i][idx1[i]]) ** 2).sum(-1)).sum()
        v += (np.asarray(g2[i]) * ((x2[i] - x1[i][idx2[i]]) ** 2).sum(-1)).sum()
    return v


def chamfer(y_true, y_pred):
    """nn_distance.py:141-148 in float64: [b] mean(dist(pred -> true)) + mean(dist(true -> pred))."""
    d1, _, d2, _ = R.nn_distance(_f64(y_pred), _f64(y_true))
    return d1.mean(-1) + d2.mean(-1)


def chamfer_grad(y_true, y_pred):
    """-> (grad_true, grad_pred, A_true, A_pred) of chamfer(...).sum()."""
    b, n_t, n_p = len(y_true), np.shape(y_true)[1], np.shape(y_pred)[1]
    gp, gt, ap, at = nn_distance_grad(y_pred, y_true, np.full((b, n_p), 1.0 / n_p), np.full((b, n_t), 1.0 / n_t))
    return gt, gp, at, ap
