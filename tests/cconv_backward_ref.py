"""Float64 restatement of CConv / ASCC for the backward tests: the pair weights are constants (positions carry no gradient),
formed from the oracle's filter coordinates (oracle.filter_coordinates) and window functions (oracle.window); the layer is then
a dense torch float64 expression whose autograd gives the reference gradients.

``abs_mode=True`` evaluates the same expression on |weights|, |features|, |filters| (and the mirror without its sign), so that
the gradients it returns are the sums of the absolute values of the terms -- the scale of the element-wise error bar."""
import numpy as np
import torch

import oracle

# dmcf_amd/csrc/cconv_bwd.hip: the filter gradient's plan
BWD_CHUNK_FLOATS = 1 << 28  # kBwdChunkFloats: B chunk [R, K * Cin] of at most 2^28 floats
BWD_MAX_SLABS = 256         # kBwdMaxSlabs
BWD_SLAB_ROWS = 256         # kBwdSlabRows: at least this many rows per slab
BWD_LDS_FLOATS = 16384      # kBwdLdsFloats: K * max(Cin, Cout) limit

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


def _coordinates(rel, extent, dims, align_corners, mapping, f64):
    """oracle.filter_coordinates per pair; ``extent``: a scalar or one extent per pair."""
    if f64:
        return oracle.filter_coordinates(rel, extent, dims, align_corners, mapping, f64=True)
    if np.ndim(extent) == 0:
        return oracle.filter_coordinates(rel, extent, dims, align_corners, mapping)
    c = np.zeros(rel.shape, np.float32)
    for e in np.unique(extent):
        sel = extent == e
        c[sel] = oracle.filter_coordinates(rel[sel], e, dims, align_corners, mapping)
    return c


class PairWeights:
    """The constants of a layer call: per pair (i, j), the window value (psi term), the pair weight a_p (times s_j), and the
    8 (cell, interpolation weight) corners.  ``extent``: a scalar, or one extent per output row (dmcf_cconv_forward_extents).
    ``f64``: the filter coordinates (kept in ``coords``) and the window are evaluated in double from the float32 relative
    positions and squared distances, not taken from the float32 oracle."""

    def __init__(self, out_pos, inp_pos, idx, row_splits, extent, full_dims, window=None, window_fac=1.0, nval=None,
                 inp_importance=None, align_corners=True, mapping="ball_to_cube_volume_preserving", interpolation="linear",
                 skip_self=False, row_count=None, f64=False):
        out_pos = np.asarray(out_pos, dtype=np.float32)
        inp_pos = np.asarray(inp_pos, dtype=np.float32)
        idx = np.asarray(idx, dtype=np.int64)
        ii, pp = rows_of(row_splits, idx.shape[0], row_count)
        jj = idx[pp]
        self.i, self.j, self.p = ii, jj, pp
        rel = (inp_pos[jj] - out_pos[ii]).astype(np.float32)
        if np.ndim(extent) > 0:
            extent = np.asarray(extent, dtype=np.float32).reshape(-1)[ii]
        radius = np.float32(0.5) * np.asarray(extent, dtype=np.float32)
        if window is None:
            a = np.ones(len(pp))
        elif window == "explicit":
            a = np.asarray(nval, dtype=np.float32)[pp].astype(np.float64)
        else:
            if nval is not None:
                d2 = np.asarray(nval, dtype=np.float32)[pp]
            else:
                d2 = ((rel[:, 0] * rel[:, 0] + rel[:, 1] * rel[:, 1]) + rel[:, 2] * rel[:, 2]).astype(np.float32)
            if f64:
                a = oracle.window(window, d2.astype(np.float64) / np.square(radius.astype(np.float64)), window_fac, dtype=np.float64)
            else:
                a = oracle.window(window, d2 * (np.float32(1) / (radius * radius)), window_fac).astype(np.float64)
        if skip_self:
            a = np.where((ii == jj) | np.all(rel == 0, axis=1), 0.0, a)
        self.norm_term = a.copy()
        if inp_importance is not None:
            a = a * np.asarray(inp_importance, dtype=np.float32)[jj].astype(np.float64)
        self.a = a
        dz, dy, dx = full_dims
        c = _coordinates(rel, extent, (dz, dy, dx), align_corners, mapping, f64) if len(pp) else np.zeros((0, 3), np.float32)
        self.coords, self.dims = c, (dz, dy, dx)
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


def grads_blocked(pw, filters, feats, grad_out, abs_mode=False, normalize=False, symmetric=False, sym_axis=2,
                  block_floats=1 << 24):
    """grads() without the dense [n_out * K, Cin] matrix: the same (d filters, d feats) in float64, and with ``abs_mode`` the
    same sums of absolute terms.  Pairs are taken in blocks of ``block_floats / max(Cin, Cout)``; within a block, per corner t,
    the pairs are grouped by their filter cell and each cell takes two float64 matmuls:
        dW_cell += F'^T (x G_i),   dF'  = (x G_i) W_cell^T   (x = w_t a_p / psi_i; F' = f_j, or f_j + f_i for ASCC)
    Peak memory is a few blocks of doubles (about 1 GB at the default); the full-kernel gradient is folded onto the stored half
    by the autograd of mirror()."""
    Wt = torch.as_tensor(np.asarray(filters), dtype=torch.float64)
    Ft = torch.as_tensor(np.asarray(feats), dtype=torch.float64)
    G = torch.as_tensor(np.asarray(grad_out), dtype=torch.float64)
    if abs_mode:
        Wt, Ft, G = Wt.abs(), Ft.abs(), G.abs()
    Wfull = mirror(Wt, sym_axis, abs_mode) if symmetric else Wt
    K, cin, cout = pw.K, Wfull.shape[3], Wfull.shape[4]
    Wk = Wfull.reshape(K, cin, cout)
    coef = pw.a
    if normalize:
        psi = np.zeros(pw.n_out)
        np.add.at(psi, pw.i, pw.norm_term)
        psi = np.where(psi != 0, psi, 1.0)
        coef = coef / psi[pw.i]
    dWk = torch.zeros(K, cin, cout, dtype=torch.float64)
    dF = torch.zeros_like(Ft)
    n = pw.i.shape[0]
    step = max(1024, block_floats // max(cin, cout))
    for b0 in range(0, n, step):
        b1 = min(n, b0 + step)
        i = torch.from_numpy(pw.i[b0:b1])
        j = torch.from_numpy(pw.j[b0:b1])
        fp = Ft[j] + Ft[i] if symmetric else Ft[j]
        Gi = G[i]
        for t in range(8):
            x = pw.wts[b0:b1, t] * coef[b0:b1]
            if abs_mode:
                x = np.abs(x)
            live = np.nonzero(x)[0]
            if live.size == 0:
                continue
            cells = pw.cells[b0:b1, t][live]
            order = live[np.argsort(cells, kind="stable")]
            cs = pw.cells[b0:b1, t][order]
            starts = np.flatnonzero(np.r_[True, cs[1:] != cs[:-1]])
            ends = np.r_[starts[1:], cs.size]
            o = torch.from_numpy(order)
            Y = torch.from_numpy(x[order])[:, None] * Gi[o]
            Fo = fp[o]
            dFo = torch.empty(order.size, cin, dtype=torch.float64)
            for s, e in zip(starts.tolist(), ends.tolist()):
                c = int(cs[s])
                dWk[c] += Fo[s:e].T @ Y[s:e]
                dFo[s:e] = Y[s:e] @ Wk[c].T
            dF.index_add_(0, j[o], dFo)
            if symmetric:
                dF.index_add_(0, i[o], dFo)
    dW = dWk.reshape(Wfull.shape)
    if symmetric:
        half = Wt.clone().requires_grad_(True)
        with torch.enable_grad():
            mirror(half, sym_axis, abs_mode).backward(dW)
        dW = half.grad
    return dW.numpy(), dF.numpy()


def bwd_plan(n_out, K, cin, cout):
    """The filter gradient's geometry, as bwd_plan / dmcf_cconv_backward (cconv_bwd.hip) form it: chunk rows R, slab count S and
    rows per slab of a full chunk, and per chunk (row0, rows, rows per slab, slabs)."""
    M = K * cin
    R = min(max(n_out, 1), BWD_CHUNK_FLOATS // M)
    S = min(-(-R // BWD_SLAB_ROWS), BWD_MAX_SLABS)
    chunks = []
    for row0 in range(0, n_out, R):
        rows = min(R, n_out - row0)
        rps = -(-rows // S)
        chunks.append((row0, rows, rps, -(-rows // rps)))
    return dict(M=M, R=R, S=S, rows_per_slab=-(-R // S), chunks=chunks)


def bwd_supported(K, cin, cout):
    return K * cin <= BWD_LDS_FLOATS and K * cout <= BWD_LDS_FLOATS


def bwd_workspace_bytes(n_out, K, cin, cout, symmetric=False, want_features=True, want_filters=True):
    """dmcf_cconv_backward_workspace_bytes: aligned blocks psi [n_out], the expanded ASCC filter, B chunk [R, M], slabs [S, M,
    Cout] and the full-kernel gradient [M, Cout] (floats), + 256."""
    pl = bwd_plan(n_out, K, cin, cout)
    full = pl["M"] * cout
    blocks = [max(n_out, 1), full if symmetric and want_features else 0, pl["R"] * pl["M"] if want_filters else 0,
              pl["S"] * full if want_filters else 0, full if want_filters else 0]
    return sum(-(-4 * b // 256) * 256 for b in blocks) + 256


def float64_cconv(real):
    """ops.cconv_forward while autograd records, restated in float64 on the CPU (differentiable in filters and features); other
    calls go to ``real``.  ``monkeypatch.setattr(ops, "cconv_forward", float64_cconv(ops.cconv_forward))``."""
    def shim(filters, out_positions, extent, inp_positions, inp_features, neighbors_index, neighbors_row_splits,
             neighbors_value=None, window=None, window_fac=1.0, inp_importance=None, align_corners=True,
             coordinate_mapping="ball_to_cube_volume_preserving", interpolation="linear", normalize=False, symmetric=False,
             sym_axis=2, bias=None, out=None, accumulate=False, neighbors_row_count=None, skip_self=False, name_only=False,
             **kw):
        if name_only or not torch.is_grad_enabled() or not (filters.requires_grad or inp_features.requires_grad):
            return real(filters, out_positions, extent, inp_positions, inp_features, neighbors_index, neighbors_row_splits,
                        neighbors_value=neighbors_value, window=window, window_fac=window_fac, inp_importance=inp_importance,
                        align_corners=align_corners, coordinate_mapping=coordinate_mapping, interpolation=interpolation,
                        normalize=normalize, symmetric=symmetric, sym_axis=sym_axis, bias=bias, out=out, accumulate=accumulate,
                        neighbors_row_count=neighbors_row_count, skip_self=skip_self, name_only=name_only, **kw)
        dims = list(filters.shape[:3])
        if symmetric:
            dims[sym_axis] *= 2
        cpu = lambda t: None if t is None else t.detach().cpu().numpy()  # noqa: E731
        pw = PairWeights(cpu(out_positions), cpu(inp_positions), cpu(neighbors_index), cpu(neighbors_row_splits), extent, dims,
                         window=window, window_fac=window_fac, nval=cpu(neighbors_value), inp_importance=cpu(inp_importance),
                         align_corners=align_corners, mapping=coordinate_mapping, interpolation=interpolation,
                         skip_self=skip_self, row_count=cpu(neighbors_row_count))
        res = conv(pw, filters.double().cpu(), inp_features.double().cpu(), normalize=normalize, symmetric=symmetric,
                   sym_axis=sym_axis)
        res = res.to(filters.device).float()
        return res if bias is None else res + bias
    return shim


EPS = 2.0 ** -24
WORST = {}  # worst err / bar per group of the GPU backward tests (printed by their test_report_worst_ratio)


def check(name, got, want, bound, kbar):
    """|got - want| <= kbar * 2^-24 * bound element-wise; records the worst err / bar under ``name``."""
    got = np.asarray(got, dtype=np.float64)
    # (an element whose every term is zero must come out zero; a floor of 1e-6 of the largest A covers terms that are an
    # exact zero on one side and a rounding residue on the other, e.g. a clamped interpolation weight)
    bar = kbar * EPS * np.maximum(bound, 1e-6 * max(float(np.max(bound)) if bound.size else 0.0, 1e-30))
    err = np.abs(got - want)
    ratio = float(np.max(err / bar)) if err.size else 0.0
    WORST[name] = max(WORST.get(name, 0.0), ratio)
    assert np.all(err <= bar), f"{name}: worst err/bar {ratio:.3g}"
