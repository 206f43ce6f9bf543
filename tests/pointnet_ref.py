"""Float64 NumPy restatements of PointNet's layer and model (the reference's models/pointnet.py), for the tests.

``layer_reference_order`` is the reference's own order: Dense on every input row, then the gather and the ragged sum
(pointnet.py:139-145), with the out-of-range rule of TensorFlow's GPU gather (an index >= n_in reads zeros: no features and
no bias).  ``layer_fused_order`` is the order of dmcf_neighbor_dense_forward: gather-sum first, then one product.
``layer_backward`` states the three gradients directly; the tests check it through the adjoint identities."""
import numpy as np


def _pairs(idx, rs, n_in):
    idx, rs = np.asarray(idx, np.int64), np.asarray(rs, np.int64)
    n_out = len(rs) - 1
    row = np.repeat(np.arange(n_out), np.diff(rs))
    j = idx[:rs[-1]]
    ok = (j >= 0) & (j < n_in)
    return row[ok], j[ok], n_out


def _act(x, relu):
    x = np.asarray(x, np.float64)
    return np.maximum(x, 0.0) if relu else x


def layer_reference_order(x, W, b, idx, rs, n_in=None, relu=True, residual=None):
    x = np.asarray(x, np.float64)
    n_in = len(x) if n_in is None else n_in
    W = np.asarray(W, np.float64)
    d = _act(x[:n_in], relu) @ W
    if b is not None:
        d = d + np.asarray(b, np.float64)
    row, j, n_out = _pairs(idx, rs, n_in)
    out = np.zeros((n_out, W.shape[1]))
    np.add.at(out, row, d[j])
    if residual is not None:
        out += np.asarray(residual, np.float64)
    return out


def aggregate(x, idx, rs, n_in=None, relu=True, absolute=False):
    """S [n_out, Cin] (the sum of act(x_j) over the in-range pairs of each row) and c [n_out] (their number)."""
    x = np.asarray(x, np.float64)
    n_in = len(x) if n_in is None else n_in
    row, j, n_out = _pairs(idx, rs, n_in)
    f = _act(x[:n_in], relu)
    if absolute:
        f = np.abs(f)
    S = np.zeros((n_out, x.shape[1]))
    np.add.at(S, row, f[j])
    c = np.bincount(row, minlength=n_out).astype(np.float64)
    return S, c


def layer_fused_order(x, W, b, idx, rs, n_in=None, relu=True, residual=None):
    S, c = aggregate(x, idx, rs, n_in, relu)
    out = S @ np.asarray(W, np.float64)
    if b is not None:
        out += c[:, None] * np.asarray(b, np.float64)[None, :]
    if residual is not None:
        out += np.asarray(residual, np.float64)
    return out


def layer_abs(x, W, b, idx, rs, n_in=None, relu=True, residual=None):
    """The output summed from absolute terms (the bar of the element-wise checks)."""
    S, c = aggregate(x, idx, rs, n_in, relu, absolute=True)
    out = S @ np.abs(np.asarray(W, np.float64))
    if b is not None:
        out += c[:, None] * np.abs(np.asarray(b, np.float64))[None, :]
    if residual is not None:
        out += np.abs(np.asarray(residual, np.float64))
    return out


def layer_backward(x, W, G, idx, rs, n_in=None, relu=True, absolute=False):
    """(dx [len(x), Cin], dW [Cin, Cout], db [Cout]) for G = dL/d out; rows of x past n_in get 0.  ``absolute``: the same
    sums of absolute terms (the bars)."""
    x = np.asarray(x, np.float64)
    n_in = len(x) if n_in is None else n_in
    W = np.asarray(W, np.float64)
    G = np.asarray(G, np.float64)
    if absolute:
        W, G = np.abs(W), np.abs(G)
    row, j, n_out = _pairs(idx, rs, n_in)
    T = np.zeros((len(x), G.shape[1]))
    np.add.at(T, j, G[row])
    dx = T @ W.T
    if relu and not absolute:
        dx = dx * (x > 0)
    S, c = aggregate(x, idx, rs, n_in, relu, absolute=absolute)
    return dx, S.T @ G, c @ G


class PointNetRef:
    """A direct transliteration of models/pointnet.py:38-195 (Dense-then-gather order, float64 after the float32 plumbing of
    the integration, which decides the neighbour set).  ``weights``: [(kernel, bias)] per layer; ``search(points, radius)``
    -> (index, row_splits) of the symmetric list with self."""

    def __init__(self, cfg, weights, search):
        self.cfg = dict(cfg)
        self.weights = weights
        self.search = search

    def step(self, data):
        cfg = self.cfg
        pos, vel, acc, feats, box, bfeats = data
        dt = np.float32(cfg.get("timestep", 0.01))
        if acc is None:
            acc = np.broadcast_to(np.float32([0.0, cfg.get("grav", -9.81), 0.0]), pos.shape)
        vel2 = (vel + dt * acc).astype(np.float32)
        pos2 = (pos + dt * vel2).astype(np.float32)  # integrate_pos_vel
        fluid = [np.ones_like(pos2[:, :1]), vel2]
        if cfg.get("use_acc", True):
            fluid.append(acc)
        fluid = np.concatenate(fluid, axis=-1).astype(np.float64)
        all_pos = np.concatenate([pos2, box], axis=0)
        P = all_pos if cfg.get("use_bnds", True) else pos2
        idx, rs = self.search(P, np.float32(cfg["particle_radii"][0]))
        ans = [fluid]
        for W, b in self.weights:
            d = layer_reference_order(ans[-1], W, b, idx, rs, relu=True)
            if d.shape[-1] == ans[-1].shape[-1]:
                d = d + ans[-1]
            ans.append(d)
        out = ans[-1]
        if cfg.get("out_activation") == "tanh":
            out = np.tanh(out)
        pcnt = len(pos2)
        self.num_fluid_neighbors = np.diff(np.asarray(rs, np.int64))[:pcnt].astype(np.float64)
        self.pos_correction = np.asarray(cfg["out_scale"], np.float64) * out[:pcnt]
        pos3 = pos2 + self.pos_correction  # compute_new_pos_vel
        vel3 = (pos3 - pos) / np.float64(dt)
        return pos3, vel3
