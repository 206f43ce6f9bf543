"""Float64 restatement of CConv / ASCC for the backward tests: the pair weights are constants (positions carry no gradient),
formed from the oracle's filter coordinates (oracle.filter_coordinates) and window functions (oracle.window); the layer is then
a dense torch float64 expression whose autograd gives the reference gradients.

``abs_mode=True`` evaluates the same expression on |weights|, |features|, |filters| (and the mirror without its sign), so that
the gradients it returns are the sums of the absolute values of the terms -- the scale of the element-wise error bar."""
import numpy as np
import torch

import oracle

INTERP = ("linear", "linear_border", "nearest_neighbor")


def _axis(x, s, interp):
    """(base cell, weight of base, weight of base + 1) per element, as the HIP kernels and Open3D define them."""
    x = x.astype(np.float64)
    bmax = max(s - 2, 0)
    if interp == "nearest_neighbor":
        c = np.sign(x) * np.floor(np.abs(x) + 0.5)  # roundf: half away from zero
        c = np.clip(c, 0, s - 1).astype(np.int64)
        b = np.minimum(c, bmax)
        w0 = (c == b).astype(np.float64)
        return b, w0, 1.0 - w0
    if interp == "linear":
        x = np.clip(x, 0.0, s - 1)
        xf = np.minimum(np.floor(x), bmax)
        a = x - xf
        if s == 1:
            return np.zeros_like(xf, dtype=np.int64), np.ones_like(x), np.zeros_like(x)
        return xf.astype(np.int64), 1.0 - a, a
    # linear_border
    xf = np.floor(x)
    a = x - xf
    c0, c1 = xf, xf + 1.0
    in0 = (c0 >= 0) & (c0 <= s - 1)
    in1 = (c1 >= 0) & (c1 <= s - 1)
    v0 = np.where(in0, 1.0 - a, 0.0)
    v1 = np.where(in1, a, 0.0)
    b = np.zeros(x.shape, dtype=np.int64)
    w0 = np.zeros_like(x)
    w1 = np.zeros_like(x)
    both = in0 & in1
    b[both], w0[both], w1[both] = c0[both].astype(np.int64), v0[both], v1[both]
    only0 = in0 & ~in1
    if s >= 2:
        b[only0], w0[only0], w1[only0] = s - 2, 0.0, v0[only0]
    else:
        b[only0], w0[only0], w1[only0] = 0, v0[only0], 0.0
    only1 = in1 & ~in0
    b[only1], w0[only1], w1[only1] = 0, v1[only1], 0.0
    return b, w0, w1


def rows_of(row_splits, n_pairs, row_count=None):
    """(output row, pair index) of every pair of a CSR or padded list; rows reaching past n_pairs are empty."""
    rs = np.asarray(row_splits, dtype=np.int64)
    n_out = rs.shape[0] - 1 if row_count is None else np.asarray(row_count).shape[0]
    ii, pp = [], []
    for i in range(n_out):
        b = rs[i]
        e = b + int(row_count[i]) if row_count is not None else rs[i + 1]
        if e > n_pairs:
            continue
        ii.extend([i] * int(e - b))
        pp.extend(range(int(b), int(e)))
    return np.asarray(ii, dtype=np.int64), np.asarray(pp, dtype=np.int64)


class PairWeights:
    """The constants of a layer call: per pair (i, j), the window value (psi term), the pair weight a_p (times s_j), and the
    8 (cell, interpolation weight) corners."""

    def __init__(self, out_pos, inp_pos, idx, row_splits, extent, full_dims, window=None, window_fac=1.0, nval=None,
                 inp_importance=None, align_corners=True, mapping="ball_to_cube_volume_preserving", interpolation="linear",
                 skip_self=False, row_count=None):
        out_pos = np.asarray(out_pos, dtype=np.float32)
        inp_pos = np.asarray(inp_pos, dtype=np.float32)
        idx = np.asarray(idx, dtype=np.int64)
        ii, pp = rows_of(row_splits, idx.shape[0], row_count)
        jj = idx[pp]
        self.i, self.j, self.p = ii, jj, pp
        rel = (inp_pos[jj] - out_pos[ii]).astype(np.float32)
        radius = np.float32(0.5) * np.float32(extent)
        if window is None:
            a = np.ones(len(pp))
        elif window == "explicit":
            a = np.asarray(nval, dtype=np.float32)[pp].astype(np.float64)
        else:
            if nval is not None:
                d2 = np.asarray(nval, dtype=np.float32)[pp]
            else:
                d2 = ((rel[:, 0] * rel[:, 0] + rel[:, 1] * rel[:, 1]) + rel[:, 2] * rel[:, 2]).astype(np.float32)
            a = oracle.window(window, d2 * (np.float32(1) / (radius * radius)), window_fac).astype(np.float64)
        if skip_self:
            a = np.where((ii == jj) | np.all(rel == 0, axis=1), 0.0, a)
        self.norm_term = a.copy()
        if inp_importance is not None:
            a = a * np.asarray(inp_importance, dtype=np.float32)[jj].astype(np.float64)
        self.a = a
        dz, dy, dx = full_dims
        c = oracle.filter_coordinates(rel, extent, (dz, dy, dx), align_corners, mapping) if len(pp) else np.zeros((0, 3), np.float32)
        bx, wx0, wx1 = _axis(c[:, 0], dx, interpolation)
        by, wy0, wy1 = _axis(c[:, 1], dy, interpolation)
        bz, wz0, wz1 = _axis(c[:, 2], dz, interpolation)
        cells, wts = [], []
        for t in range(8):
            tx, ty, tz = t & 1, (t >> 1) & 1, (t >> 2) & 1
            live = not ((tx and dx < 2) or (ty and dy < 2) or (tz and dz < 2))
            w = (wx1 if tx else wx0) * (wy1 if ty else wy0) * (wz1 if tz else wz0)
            # (a "+1" corner along an axis of size 1 does not exist: weight 0 on the base cell)
            cells.append(((bz + tz) * dy + (by + ty)) * dx + (bx + tx) if live else (bz * dy + by) * dx + bx)
            wts.append(w if live else np.zeros_like(w))
        self.cells = np.stack(cells, 1) if len(pp) else np.zeros((0, 8), np.int64)
        self.wts = np.stack(wts, 1) if len(pp) else np.zeros((0, 8))
        self.n_out = out_pos.shape[0]
        self.K = dz * dy * dx


def mirror(half, sym_axis, abs_mode=False):
    """utils/convolutions.py:410-412 on a torch tensor: concat([-flip_zyx(half), half], sym_axis)."""
    flipped = torch.flip(half, dims=(0, 1, 2))
    return torch.cat([flipped if abs_mode else -flipped, half], dim=sym_axis)


def conv(pw, filters, feats, normalize=False, symmetric=False, sym_axis=2, abs_mode=False):
    """out [n_out, Cout] in float64 (torch, differentiable in filters and feats)."""
    W = mirror(filters, sym_axis, abs_mode) if symmetric else filters
    cin, cout = W.shape[3], W.shape[4]
    Wk = W.reshape(pw.K, cin, cout)
    i = torch.from_numpy(pw.i)
    j = torch.from_numpy(pw.j)
    coef = torch.from_numpy(pw.a)
    if normalize:
        psi = np.zeros(pw.n_out)
        np.add.at(psi, pw.i, pw.norm_term)
        psi = np.where(psi != 0, psi, 1.0)
        coef = coef / torch.from_numpy(psi[pw.i])
    wts = torch.from_numpy(pw.wts) * coef[:, None]
    f = feats[j]
    if symmetric:
        f = (f.abs() + feats[i].abs()) if abs_mode else f + feats[i]
    if abs_mode:
        wts = wts.abs()
    M = torch.zeros(pw.n_out * pw.K, cin, dtype=torch.float64)
    rows = (i[:, None] * pw.K + torch.from_numpy(pw.cells)).reshape(-1)
    M = M.index_add(0, rows, (wts[:, :, None] * f[:, None, :]).reshape(-1, cin))
    return torch.einsum("ikc,kco->io", M.reshape(pw.n_out, pw.K, cin), Wk)


def grads(pw, filters, feats, grad_out, abs_mode=False, **kw):
    """(d filters, d feats) of <grad_out, conv(filters, feats)> in float64; abs_mode: the sums of absolute terms."""
    Wt = torch.as_tensor(np.asarray(filters), dtype=torch.float64)
    Ft = torch.as_tensor(np.asarray(feats), dtype=torch.float64)
    G = torch.as_tensor(np.asarray(grad_out), dtype=torch.float64)
    if abs_mode:
        Wt, Ft, G = Wt.abs(), Ft.abs(), G.abs()
    Wt.requires_grad_(True)
    Ft.requires_grad_(True)
    with torch.enable_grad():
        out = conv(pw, Wt, Ft if not abs_mode else Ft, abs_mode=abs_mode, **kw)
        (out * G).sum().backward()
    return Wt.grad.numpy(), Ft.grad.numpy(), out.detach().numpy()
