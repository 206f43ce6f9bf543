"""The forward CConv / ASCC against a float64 reference with an element-wise error bar, and the deterministic cases both
tests/test_cconv_forward_ref_cpu.py (the float32 oracle: the bar is sound, seeded faults break it) and
tests/test_gpu_cconv_forward_bar.py (every dispatched HIP kernel) run.

    |got - ref| <= (kbar * A + C_GEO * A1) * 2^-24         element by element

ref  cconv_backward_ref.conv in float64 on PairWeights(f64=True): filter coordinates and window evaluated in double from the
     float32 relative positions and squared distances
A    the same sum over the absolute values of every term (+ |bias|, + |prior out| under accumulate): the scale of the roundings
     that are RELATIVE in a term; kbar = max(K_BAR, longest row + K * Cin + PER_TERM) as in test_gpu_cconv_backward_sets.py
A1   the absolute sum with every live corner's interpolation weight set to 1 and a distance window's value set to window_fac:
     the scale of errors that are ABSOLUTE in a weight.  A float32 rounding of the filter coordinate, or of d^2 / r^2, moves a
     weight by a few 2^-24 however small the weight itself is (a corner next to an integer coordinate, a pair at the window's
     edge).
"""
import copy

import numpy as np
import torch

import oracle
import cconv_backward_ref as ref
import primitive_edges_ref as pe
from cconv_backward_ref import EPS, WORST, PairWeights, conv  # noqa: F401

K_BAR = 256
PER_TERM = 64
# C_GEO: measured by test_cconv_forward_ref_cpu.py::test_c_geo_is_the_measured_constant on the float32 CPU oracle over every
# case of this file -- the worst (err - kbar * A * 2^-24) / (A1 * 2^-24) is MEASURED_C_GEO; times 4 (the GPU's sqrt, atan and
# division are a few ulp where the host's are correctly rounded; FMA contraction), rounded up to a power of two.
# What the measurement sees is what the matrix isolates: 0.0938 comes from row "Y" of the ``far_plane`` cases (a lone corner
# weight of 2^-13 formed from a float32 coordinate next to 2.0: 2750 * 2^-24 of its A where kbar is 960).  Row "X" (a lone pair
# at the window's edge, 1 - q = 1e-3) measures 2.8e-7 only, and lies below the floor of check() next to a 640-pair row.  In
# every other element the roundings that are absolute in a weight are covered by kbar * A.
MEASURED_C_GEO = 0.095
C_GEO = 0.5

DISTANCE_WINDOWS = ("poly6", "cubic", "linear", "peak", "cubic_grad")
NN_FRAGILE = 2.0 ** -18  # a nearest_neighbor coordinate this close (times the axis size) to x.5 may round to the other cell
NN_MAX_SHARE = 0.02


def _live_corners(dims):
    dz, dy, dx = dims
    return np.asarray([0.0 if ((t & 1 and dx < 2) or ((t >> 1) & 1 and dy < 2) or ((t >> 2) & 1 and dz < 2)) else 1.0
                       for t in range(8)])


def forward_bar(pw, filters, feats, normalize=False, symmetric=False, sym_axis=2, window=None, window_fac=1.0,
                inp_importance=None):
    """(ref, A, A1) [n_out, Cout] float64 of one call on the PairWeights ``pw``."""
    W = torch.as_tensor(np.asarray(filters), dtype=torch.float64)
    F = torch.as_tensor(np.asarray(feats), dtype=torch.float64)
    kw = dict(normalize=normalize, symmetric=symmetric, sym_axis=sym_axis)
    out = conv(pw, W, F, **kw).numpy()
    A = conv(pw, W.abs(), F.abs(), abs_mode=True, **kw).numpy()
    one = copy.copy(pw)
    one.wts = np.broadcast_to(_live_corners(pw.dims), pw.wts.shape).copy()
    if window in DISTANCE_WINDOWS:
        a1 = np.full(pw.a.shape, abs(float(window_fac)))
        if inp_importance is not None:
            a1 = a1 * np.abs(np.asarray(inp_importance, dtype=np.float64)[pw.j])
        one.a = a1  # (normalize: divided by the same psi_i as A's coefficient -- norm_term stays)
    A1 = conv(one, W.abs(), F.abs(), abs_mode=True, **kw).numpy()
    return out, A, A1


def kbar_of(pw, cin):
    """max(K_BAR, chain + PER_TERM), chain = the longest row + the contraction length K * Cin."""
    longest = int(np.bincount(pw.i, minlength=1).max()) if pw.i.size else 0
    return max(K_BAR, longest + pw.K * cin + PER_TERM)


def fragile_rows(pw, interpolation):
    """bool [n_out]: rows left out of the comparison.  Only nearest_neighbor has any: a row one of whose pairs has a float64
    filter coordinate within 2^-18 * s of a half-integer on an axis of size s."""
    bad = np.zeros(pw.n_out, dtype=bool)
    if interpolation != "nearest_neighbor" or not pw.i.size:
        return bad
    dz, dy, dx = pw.dims
    for k, s in enumerate((dx, dy, dz)):
        c = pw.coords[:, k].astype(np.float64)
        near = np.abs(c - np.floor(c) - 0.5) < NN_FRAGILE * s
        bad[pw.i[near]] = True
    return bad


def geo_ratio(got, want, A, A1, kbar, keep=None):
    """The worst (err - kbar * A * 2^-24) / (A1 * 2^-24): what the A part of the bar leaves to C_GEO."""
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    rest = err - kbar * EPS * A  # (without the floor of check(): it would hide every small element)
    r = np.where(A1 > 0, rest / np.maximum(A1 * EPS, 1e-300), 0.0)
    if keep is not None:
        r = r[keep]
    return max(float(r.max()) if r.size else 0.0, 0.0)


def check_forward(name, got, want, A, A1, kbar, keep=None, c_geo=None):
    """The assertion of this file's docstring (with the floor of cconv_backward_ref.check); worst err / bar under ``name``."""
    bound = kbar * A + (C_GEO if c_geo is None else c_geo) * A1
    got = np.asarray(got, dtype=np.float64)
    if keep is not None:
        got, want, bound = got[keep], want[keep], bound[keep]
    ref.check(name, got, want, bound, 1.0)


def within_bar(got, want, A, A1, kbar, keep=None):
    try:
        check_forward("_probe", got, want, A, A1, kbar, keep)
    except AssertionError:
        return False
    finally:
        WORST.pop("_probe", None)
    return True


# ---- deterministic clouds ------------------------------------------------------------------------------------------------------

ROW_LENGTHS = (1, 2, 63, 64, 65, 127, 128, 129, 640)
RADIUS = 0.23  # (not a power of two: 1 / extent and 1 / r^2 round)
# order of the output rows: E = a point without a neighbour (first, at tile rows 5 and 13, and last), then the probes
_HEAD = ("E", 1, 2, 63, 64, "E", 65, 127, 128, 129, 640, "X", "Y", "E")
ROW_X, ROW_Y = 11, 12
N_OUT_EDGES = (1, 15, 16, 17, 31, 33, 255, 257)
N_OUT_FULL = 420


def _embed(v, dim):
    """[n, dim] -> [n, 3]: 3-D as it is, 2-D in the x-y plane (z = 0), 1-D on the y axis, as the filters (1, 8, 8) / (1, 8, 1)."""
    p = np.zeros((v.shape[0], 3))
    if dim == 3:
        p[:] = v
    elif dim == 2:
        p[:, :2] = v
    else:
        p[:, 1] = v[:, 0]
    return p


def _ball(rng, n, dim, r):
    d = rng.normal(size=(n, dim))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return d * (r * rng.uniform(0, 1, size=(n, 1)) ** (1.0 / dim))


Y_T = 2 * (2 + 2.0 ** -13) / 3 - 1  # (0.5 + 0.5 t) * (4 - 1) = 2 + 2^-13; a pair on a filter axis at d has t = d / R in every mapping


def controlled_cloud(seed, dim=3, n_out=None, offset=0.0):
    """(inp [n_inp, 3], out [n_out, 3]) float32.  One clump of L input points per L of ROW_LENGTHS, spread through the ball of
    0.95 R around its probe (4 R from the next clump, so the probe's row has exactly L pairs), a random cloud of about 25
    neighbours per row, and far points without a neighbour; output rows in the order of _HEAD, then the random ones.  The
    single-pair row's pair is at R / 2, the 2-pair row's at 1e-3 R and R / 2; row "X" has a single pair too, at 0.9995 R (the
    window's edge: a weight of 1e-9, all of it rounding where d^2 / r^2 is formed in float32).  Row "Y" has a single pair on
    the y axis at Y_T * R: on a filter axis of 4 cells its coordinate is 2 + 2^-13, so cell 3 gets an interpolation weight
    of 2^-13 that a float32 coordinate (ulp 2^-22) moves by 1e-3 of itself (see the ``far_plane`` filters of Case).
    ``n_out``: truncated to n_out - 1 rows plus a last empty row (n_out = 1: the 65-pair row alone)."""
    rng = np.random.default_rng(seed)
    R = RADIUS
    axis = np.zeros(3)
    axis[1] = 1.0
    first = np.zeros((1, dim))
    first[0, -1 if dim == 1 else 1] = 1.0  # (a direction inside the subspace)
    inp, probes = [], {}
    for k, L in enumerate(ROW_LENGTHS):
        c = axis * (4 * R * k)
        if L == 1:
            pts = first * (0.5 * R)
        elif L == 2:
            pts = np.concatenate([first * (1e-3 * R), -first * (0.5 * R)])
        else:
            pts = _ball(rng, L, dim, 0.95 * R)
        inp.append(_embed(pts, dim) + c)
        probes[L] = c
    probes["X"] = axis * (4 * R * len(ROW_LENGTHS))
    inp.append(_embed(-first * (0.9995 * R), dim) + probes["X"])
    probes["Y"] = axis * (4 * R * (len(ROW_LENGTHS) + 1))
    inp.append(_embed(first * (Y_T * R), dim) + probes["Y"])
    side = {3: 5.86, 2: 12.3, 1: 96.0}[dim] * R
    lo = axis * (4 * R * (len(ROW_LENGTHS) + 3))
    inp.append(_embed(rng.uniform(0, side, size=(1200, dim)), dim) + lo)
    rand = _embed(rng.uniform(-R, side + R, size=(N_OUT_FULL, dim)), dim) + lo
    empty = lambda k: -axis * (10 * R + 3 * R * k)  # noqa: E731
    rows, r, e = [], 0, 0
    for h in _HEAD:
        if h == "E":
            rows.append(empty(e))
            e += 1
        elif h == "R":
            rows.append(rand[r])
            r += 1
        else:
            rows.append(probes[h])
    out = np.concatenate([np.asarray(rows), rand[r:]])[:N_OUT_FULL]
    if n_out == 1:
        out = probes[65][None]
    elif n_out is not None:
        out = np.concatenate([out[:n_out - 1], empty(7)[None]])
    return ((np.concatenate(inp) + offset).astype(np.float32), (out + offset).astype(np.float32))


def padded_list(idx, rs, val, cut):
    """The CSR list as a padded one (rows at a fixed stride of the longest row + 3, begins + counts) whose pair buffer ends
    before the last ``cut`` rows: they reach past it, and count as empty (include/dmcf_hip.h, dmcf_cconv_args.n_pairs)."""
    n = rs.shape[0] - 1
    cnt = np.diff(rs).astype(np.int32)
    stride = int(cnt.max()) + 3 if n else 3
    begin = np.arange(n + 1, dtype=np.int64) * stride
    ibuf = np.zeros(n * stride, np.int32)
    vbuf = np.zeros(n * stride, np.float32)
    dst = np.repeat(begin[:-1], cnt) + (np.arange(idx.shape[0]) - np.repeat(rs[:-1], cnt))
    ibuf[dst], vbuf[dst] = idx, val
    cap = (n - cut) * stride
    return ibuf[:cap], begin, vbuf[:cap], cnt


class Case:
    """One forward call: its arrays (numpy), options and float64 bar.  ``spec`` keys: shape (the stored filter's), cin, cout,
    window (None | 'explicit' | 'poly6' | 'cubic' | 'peak' ...), dist (a distance window reads the list's squared distances),
    imp, normalize, bias, accumulate, sym_axis (None: plain CConv), padded, n_out, mask, offset, mapping, interp, align,
    zero_channel, seed, extents (one extent per output row), far_plane (the filter is zero except in its last y plane: row "Y"
    of the cloud then holds nothing but a corner weight of 2^-13; its input point's features are scaled by 64, which keeps
    the row above the floor of the bar)."""

    DEFAULTS = dict(window="poly6", dist=False, imp=False, normalize=False, bias=False, accumulate=False, sym_axis=None,
                    padded=False, n_out=None, mask=False, offset=0.0, mapping="ball_to_cube_volume_preserving", interp="linear",
                    align=True, zero_channel=None, seed=1, window_fac=1.0, extents=False, far_plane=False)

    def __init__(self, **spec):
        s = dict(self.DEFAULTS)
        s.update(spec)
        self.spec = s
        self.__dict__.update(s)
        shape, cin, cout = tuple(s["shape"]), s["cin"], s["cout"]
        self.symmetric = s["sym_axis"] is not None
        full = list(shape)
        if self.symmetric:
            full[s["sym_axis"]] *= 2
        self.full = tuple(full)
        self.K = full[0] * full[1] * full[2]
        dim = 3 - sum(1 for d in full if d == 1)
        rng = np.random.default_rng(1000 + s["seed"])
        inp, out = controlled_cloud(s["seed"], dim, None if self.symmetric else s["n_out"], s["offset"])
        if self.symmetric:  # the same set: the outputs are the first n_out inputs, the list ignores the query point
            inp = inp[rng.permutation(inp.shape[0])]
            out = inp[:s["n_out"] or N_OUT_FULL]
        self.inp_pos, self.out_pos = inp, out
        n_inp, n_out = inp.shape[0], out.shape[0]
        self.extent = float(np.float32(2) * np.float32(RADIUS))
        idx, rs, d2 = oracle.fixed_radius_search(inp, out, RADIUS, self.symmetric, bruteforce=True)
        self.csr_counts = np.diff(rs)
        self.row_extents = None
        if s["extents"]:  # per-row extents over a factor of 4, none larger than the list's reach
            self.row_extents = (self.extent * rng.uniform(0.25, 1.0, size=n_out)).astype(np.float32)
        val = d2
        if s["window"] == "explicit":
            val = rng.uniform(0.1, 1.0, size=idx.shape[0]).astype(np.float32)
        self.count = None
        self.cut = 0
        if s["padded"]:
            # (cut at least the last two rows, and as many as it takes to cut one that is not empty)
            filled = np.flatnonzero(np.diff(rs))
            self.cut = max(2, n_out - int(filled[-1])) if n_out > 2 and filled.size else 0
            idx, rs, val, self.count = padded_list(idx, rs, val, self.cut)
            assert self.cut == 0 or (self.cut < n_out and self.count[-self.cut:].sum() > 0), "no row cut off by the capacity"
        self.idx, self.rs = idx, rs
        self.nval = val if (s["window"] == "explicit" or (s["window"] is not None and s["dist"])) else None
        self.feat = rng.normal(size=(n_inp, cin)).astype(np.float32)
        filt = rng.uniform(-1, 1, size=(*shape, cin, cout)).astype(np.float32)
        self.tile_mask = None
        if s["mask"]:  # block-diagonal: channels [0, ca) -> [0, 16), [ca, cin) -> [16, cout)
            ca = max(4, cin // 2 // 4 * 4)
            assert cin >= 8 and cout > 16
            filt[..., :ca, 16:] = 0
            filt[..., ca:, :16] = 0
            self.tile_mask = [(0, ca, 0, 16), (ca, cin, 16, cout)]
        if s["far_plane"]:
            filt[:, :shape[1] - 1] = 0
            self.feat[idx[rs[ROW_Y]]] *= 64
        if s["zero_channel"] is not None:
            filt[..., s["zero_channel"]] = 0
        self.filt = filt
        self.bias_v = rng.normal(size=cout).astype(np.float32) if s["bias"] else None
        self.prior = rng.normal(size=(n_out, cout)).astype(np.float32) if s["accumulate"] else None
        self.imp_v = rng.uniform(0.2, 2.0, size=n_inp).astype(np.float32) if s["imp"] else None
        self.pw = self.pair_weights(f64=True)

    def pair_weights(self, f64):
        return PairWeights(self.out_pos, self.inp_pos, self.idx, self.rs, self.extent if self.row_extents is None else
                           self.row_extents, self.full, window=self.window, window_fac=self.window_fac, nval=self.nval,
                           inp_importance=self.imp_v, align_corners=self.align, mapping=self.mapping, interpolation=self.interp,
                           row_count=self.count, f64=f64)

    def bar(self):
        """(ref, A, A1, kbar, rows compared) with bias and prior content added to ref and A."""
        if getattr(self, "_bar", None) is None:
            out, A, A1 = forward_bar(self.pw, self.filt, self.feat, normalize=self.normalize, symmetric=self.symmetric,
                                     sym_axis=self.sym_axis if self.symmetric else 2, window=self.window,
                                     window_fac=self.window_fac, inp_importance=self.imp_v)
            if self.bias_v is not None:
                out, A = out + self.bias_v, A + np.abs(self.bias_v)
            if self.prior is not None:
                out, A = out + self.prior, A + np.abs(self.prior)
            self._bar = (out, A, A1, kbar_of(self.pw, self.cin), ~fragile_rows(self.pw, self.interp))
        return self._bar

    def effective_csr(self):
        """(index, row splits, per-pair value or None) of the pairs the call really has (cut rows are empty)."""
        cnt = np.bincount(self.pw.i, minlength=self.out_pos.shape[0])
        rs = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
        return self.idx[self.pw.p].astype(np.int32), rs, None if self.nval is None else self.nval[self.pw.p]

    def importance(self, idx, rs, val, out_pos=None, extent=None):
        """The per-pair importance the float32 oracle takes: the explicit values, or the window of the squared distances (the
        list's, or re-formed from the positions as the search forms them)."""
        if self.window is None:
            return None
        if self.window == "explicit":
            return val
        if val is None:
            row = np.repeat(np.arange(rs.shape[0] - 1), np.diff(rs))
            rel = self.inp_pos[idx] - (self.out_pos if out_pos is None else out_pos)[row]
            val = (rel[:, 0] * rel[:, 0] + rel[:, 1] * rel[:, 1]) + rel[:, 2] * rel[:, 2]
        r = np.float32(0.5) * np.float32(self.extent if extent is None else extent)
        return oracle.window(self.window, val / (r * r), self.window_fac)

    def oracle32(self, idx=None, rs=None, val=None, imp="own", full=None):
        """The float32 CPU oracle's result (oracle.continuous_conv; ContinuousConvRef's two passes for ASCC) + bias + prior.
        ``idx, rs, val`` / ``imp`` / ``full`` replace the case's list, importances and mirrored ASCC filter (the seeded faults)."""
        if idx is None:
            idx, rs, val = self.effective_csr()
        imp = self.imp_v if isinstance(imp, str) else imp
        filt = self.filt
        if self.row_extents is not None:  # (the oracle takes one extent: a call per row)
            assert not self.symmetric
            y = np.zeros((self.out_pos.shape[0], self.cout), np.float32)
            kw = dict(align_corners=self.align, coordinate_mapping=self.mapping, interpolation=self.interp, normalize=self.normalize)
            for i in np.flatnonzero(np.diff(rs)):
                sl = slice(rs[i], rs[i + 1])
                one = np.asarray([0, rs[i + 1] - rs[i]], np.int64)
                v = None if val is None else val[sl]
                nimp = self.importance(idx[sl], one, v, self.out_pos[i:i + 1], self.row_extents[i])
                y[i] = oracle.continuous_conv(filt, self.out_pos[i:i + 1], self.row_extents[i], self.inp_pos, self.feat, idx[sl],
                                              one, nimp, inp_importance=imp, **kw)[0]
            return self._epilogue(y)
        nimp = self.importance(idx, rs, val)
        kw = dict(align_corners=self.align, coordinate_mapping=self.mapping, interpolation=self.interp, normalize=self.normalize)
        if self.symmetric:
            assert imp is None
            full = oracle.mirror_kernel(filt, self.sym_axis) if full is None else full
            args = dict(out_positions=self.out_pos, extents=self.extent, inp_positions=self.inp_pos, neighbors_index=idx,
                        neighbors_row_splits=rs, neighbors_importance=nimp, **kw)
            y = oracle.continuous_conv(full, inp_features=self.feat, **args)
            w = oracle.continuous_conv(full.reshape(*full.shape[:3], 1, -1), inp_features=np.ones_like(self.feat[:, :1]), **args)
            n_out = self.out_pos.shape[0]
            y = y + np.einsum("nc,nco->no", self.feat[:n_out], w.reshape(n_out, self.cin, self.cout)).astype(np.float32)
        else:
            y = oracle.continuous_conv(filt, self.out_pos, self.extent, self.inp_pos, self.feat, idx, rs, nimp,
                                       inp_importance=imp, **kw)
        return self._epilogue(y)

    def _epilogue(self, y):
        if self.bias_v is not None:
            y = y + self.bias_v
        if self.prior is not None:
            y = y + self.prior
        return y.astype(np.float32)

    def __repr__(self):
        return ",".join(f"{k}={v}" for k, v in self.spec.items() if k not in self.DEFAULTS or self.DEFAULTS[k] != v)


# ---- the matrix -----------------------------------------------------------------------------------------------------------------

WINDOW_FORMS = ((None, False), ("explicit", False), ("poly6", True), ("poly6", False), ("peak", True), ("cubic", False))
S444, S188, S181, S352 = (4, 4, 4), (1, 8, 8), (1, 8, 1), (3, 5, 2)
QUADS = (4, 8, 16, 24, 32)
# per forced kernel: what its eligibility function accepts (dmcf_amd/csrc/cconv_*.hip) of the options of this file
#   shapes, cins, couts; normalize; sym: (stored shape, axis) forms; mask: filter_tile_mask is honoured
# (every kernel that takes ASCC takes the three axes: none of the eligibility functions reads sym_axis, each packer does)
KERNELS = {
    "lds": dict(name="cconv_kernel<", shapes=(S444, S188, S181, S352), cins=(1, 3, 4, 5, 8, 9, 16, 17, 24, 32, 33),
                couts=(1, 3, 15, 16, 17, 32, 33, 64), normalize=True, sym=(((4, 4, 2), 2), ((2, 4, 4), 0), ((1, 4, 8), 1))),
    "mfma": dict(name="cconv_mfma_kernel", shapes=(S444, S188, S181, S352), cins=(1, 3, 4, 5, 8, 9, 16, 17, 24, 32, 33),
                 couts=(1, 3, 15, 16, 17, 32, 33, 64), normalize=True, sym=(((4, 4, 2), 2), ((4, 2, 4), 1), ((2, 4, 4), 0))),
    "blk": dict(name="cconv_blk_kernel<", shapes=(S444,), cins=QUADS + (36,), couts=(1, 3, 15, 16, 17, 32, 33, 64),
                sym=(((4, 4, 2), 2), ((4, 2, 4), 1), ((2, 4, 4), 0))),
    "cls": dict(name="cconv_cls_kernel<", shapes=(S444,), cins=QUADS + (36,), couts=(1, 3, 15, 16, 17, 32, 33, 64),
                sym=(((4, 4, 2), 2), ((4, 2, 4), 1), ((2, 4, 4), 0)), mask=True),
    "z3": dict(name="cconv_z3_kernel<", shapes=(S444,), cins=QUADS, couts=(1, 3, 15, 16, 17, 32, 33, 64), mask=True),
    "pair": dict(name="cconv_pair_kernel<", shapes=(S444,), cins=QUADS, couts=(1, 3, 15, 16, 17, 32, 33, 64), mask=True),
    "ws": dict(name="cconv_ws_kernel<", shapes=(S444,), cins=QUADS, couts=(1, 3, 15, 16, 17, 32)),
    "g16": dict(name="cconv_p16_kernel<", shapes=(S444,), cins=(4, 8, 16), couts=(1, 3, 15, 16, 17, 32, 33, 64), mask=True),
    "direct": dict(name="cconv_direct_kernel<", shapes=(S444, S188, S181, S352), cins=(1, 3, 4, 5, 8, 9, 16, 17, 24, 32),
                   couts=(1, 2, 3, 4), normalize=True, sym=(((6, 3, 6), 1), ((4, 4, 2), 2), ((2, 4, 4), 0), ((1, 4, 8), 1))),
}
# the automatic dispatch: (spec, the kernel its rules pick) -- cconv.hip's chain without DMCF_CCONV_KERNEL
AUTO = (
    (dict(shape=S444, cin=32, cout=32), "cconv_z3_kernel<"), (dict(shape=S444, cin=16, cout=17), "cconv_cls_kernel<"),
    (dict(shape=S444, cin=8, cout=3), "cconv_cls_kernel<"), (dict(shape=S444, cin=4, cout=33), "cconv_kernel<"),
    (dict(shape=S444, cin=16, cout=16, normalize=True), "cconv_mfma_kernel"),
    (dict(shape=(6, 3, 6), sym_axis=1, cin=32, cout=3, window="peak", dist=True), "cconv_direct_kernel<"),
    (dict(shape=S188, cin=5, cout=15), "cconv_kernel<"), (dict(shape=S188, cin=17, cout=64), "cconv_mfma_kernel"),
    (dict(shape=S352, cin=5, cout=1, normalize=True), "cconv_kernel<"),
)


def _kernel_cases(kernel):
    """A covering set for one forced kernel: every option it accepts appears with both list forms and at an n_out edge."""
    k = KERNELS[kernel]
    cins, couts, shapes = k["cins"], k["couts"], k["shapes"]
    cases = []
    t = 0

    def add(**kw):
        nonlocal t
        spec = dict(shape=shapes[t % len(shapes)], cin=cins[t % len(cins)], cout=couts[(5 * t + 1) % len(couts)], seed=1 + t % 3)
        spec.update(kw)
        cases.append(spec)
        t += 1
    edges = list(N_OUT_EDGES)
    # windows x list forms, at the full size and at an edge
    for w, (win, dist) in enumerate(WINDOW_FORMS):
        for padded in (False, True):
            add(window=win, dist=dist, padded=padded, n_out=None if (w + padded) % 2 else edges[(2 * w + padded) % len(edges)],
                bias=bool((w + padded) % 2), imp=w % 3 == 2)
    # every single option with both list forms, the padded one at an edge
    opts = [dict(imp=True), dict(bias=True), dict(accumulate=True), dict(bias=True, accumulate=True, imp=True)]
    if k.get("normalize"):
        opts += [dict(normalize=True), dict(normalize=True, window=None), dict(normalize=True, imp=True, dist=True)]
    for i, o in enumerate(opts):
        add(padded=False, n_out=edges[(i + 3) % len(edges)], **o)
        add(padded=True, n_out=edges[(i + 5) % len(edges)] if i % 2 else None, **o)
        if i % 2 == 0:
            add(padded=True, n_out=edges[(i + 6) % len(edges)], **o)
    for i, (shape, axis) in enumerate(k.get("sym", ())):
        cin = [c for c in cins if kernel != "direct" or c >= 8][(2 * i + 1) % 3]
        for padded in (False, True):
            add(shape=shape, sym_axis=axis, cin=cin, cout=couts[i % len(couts)] if kernel == "direct" else (3, 17, 4, 15)[i],
                window="peak", dist=True, padded=padded, n_out=(None, 257, 33, 17, 255, 31, 16, None)[2 * i + padded], bias=bool(i % 2))
    if k.get("mask"):
        for i, (cin, cout) in enumerate(((8, 32), (16, 33), (min(cins[-1], 32), 64))):
            add(shape=S444, cin=cin, cout=cout, mask=True, padded=bool(i % 2), n_out=(None, 33, 17)[i])
        add(shape=S444, cin=8, cout=17, mask=True, padded=False, n_out=31)
        add(shape=S444, cin=min(cins[-1], 32), cout=32, mask=True, padded=True, n_out=None)
    # every chunk edge of the channel counts once more, and every shape; positions far from the origin
    for i in range(max(len(cins), len(couts))):
        add(cin=cins[i % len(cins)], cout=couts[i % len(couts)], padded=bool(i % 2), n_out=edges[i % len(edges)] if i % 3 else None)
    # nothing but a corner weight of 2^-13 in row "Y" (4 cells on the y axis), no window: the absolute error of a weight
    c4 = [c for c in cins if c >= 4][0]
    add(shape=shapes[0], cin=c4, cout=couts[1], window=None, far_plane=True, n_out=17)
    add(shape=shapes[0], cin=c4, cout=couts[2], window="poly6", far_plane=True, padded=True, n_out=33)
    # an output channel whose filter slice is zero: inside a 16-channel tile and as its last channel
    zc = 4 if kernel == "direct" else 17
    for ch in (1, zc - 1):
        add(shape=shapes[0], cin=cins[-1], cout=zc, bias=True, zero_channel=ch, n_out=33, dist=True)
    add(offset=6.0, dist=False)
    add(offset=60.0, dist=True, padded=True, n_out=33)
    return cases


def matrix():
    """[(id, forced kernel or None, expected kernel-name prefix, spec)]: every neighbour-list case of the GPU file."""
    out = []
    for kernel in KERNELS:
        for n, spec in enumerate(_kernel_cases(kernel)):
            out.append((f"{kernel}-{n}", kernel, KERNELS[kernel]["name"], spec))
    for n, (spec, name) in enumerate(AUTO):
        for padded in (False, True):
            out.append((f"auto-{n}-{'padded' if padded else 'csr'}", None, name,
                        dict(spec, padded=padded, n_out=N_OUT_EDGES[(2 * n + padded) % 8] if (n + padded) % 2 else None,
                             bias=bool(n % 2), accumulate=n % 3 == 0)))
    # the generic kernel's option matrix at one odd n_out
    n = 0
    for mapping in ("ball_to_cube_radial", "ball_to_cube_volume_preserving", "identity"):
        for interp in ("linear", "linear_border", "nearest_neighbor"):
            for align, normalize in ((True, False), (False, True)):
                out.append((f"options-{mapping}-{interp}-{int(align)}", "lds", "cconv_kernel<",
                            dict(shape=(4, 3, 5), cin=4, cout=6, mapping=mapping, interp=interp, align=align, normalize=normalize,
                                 imp=True, dist=True, n_out=257, padded=bool(n % 2), seed=2)))
                n += 1
    # the other kernels with a generic instantiation: a few of the same options
    for kernel, shape, cin, cout in (("mfma", (4, 3, 5), 5, 17), ("direct", (3, 5, 2), 9, 3)):
        for mapping, interp, align in (("ball_to_cube_radial", "linear_border", False), ("identity", "nearest_neighbor", True),
                                       ("identity", "linear", False)):
            out.append((f"options-{kernel}-{mapping}-{interp}", kernel, KERNELS[kernel]["name"],
                        dict(shape=shape, cin=cin, cout=cout, mapping=mapping, interp=interp, align=align, n_out=255, seed=3)))
    # packed filters above the cap of their packer's grid (tests/primitive_edges_ref.py, G): the grid-stride loop of pack_filter /
    # pack_filter_cls runs a second time.  The smallest 4x4x4 shape each form accepts above 2048 x 256 packed elements; the
    # antisymmetric form of the same size once (the packers mirror in the same loop)
    for kernel, shapes in pe.PACKER_CASES.items():
        for n, (cin, cout) in enumerate(shapes):
            out.append((f"packer-{kernel}-{cin}", kernel, KERNELS[kernel]["name"],
                        dict(shape=S444, cin=cin, cout=cout, n_out=33, padded=bool(n % 2), bias=True, seed=2)))
    out.append(("packer-cls-132-sym", "cls", KERNELS["cls"]["name"],
                dict(shape=(4, 4, 2), sym_axis=2, cin=132, cout=49, n_out=33, window="peak", dist=True, seed=3)))
    # dmcf_cconv_forward_extents: per-row extents over a factor of 4
    for cin in (3, 9):
        for padded, dist in ((False, False), (True, True)):
            out.append((f"extents-{cin}-{'padded' if padded else 'csr'}", None, "cconv_ext_kernel<",
                        dict(shape=S444, cin=cin, cout=17, extents=True, padded=padded, dist=dist, bias=True, normalize=padded)))
    return out


LATTICE_CASES = ("same", "fine_to_coarse", "coarse_same", "coarse_to_fine", "over_cap")


def _lattice(rng, dims, occupancy, voxel, center, step=1):
    """Random subset of the cells of a lattice box -> (cells int32 [n, 3] (x, y, z), positions float(cell) * voxel + center)."""
    g = np.stack(np.meshgrid(*[np.arange(d, dtype=np.int32) for d in dims], indexing="ij"), -1).reshape(-1, 3)
    g = g[rng.random(g.shape[0]) < occupancy]
    g = g[rng.permutation(g.shape[0])]
    pos = g.astype(np.float32) * (np.float32(voxel) * np.float32(step)) + center.astype(np.float32)
    return g, pos.astype(np.float32)


def lattice_case(case):
    """The point sets, features, 4x4x4 filter and bias of tests/test_gpu_ops.py::test_lattice_conv_matches_neighbour_list_form."""
    rng = np.random.default_rng(21)
    h = 0.05
    center = rng.uniform(-0.5, 0.5, size=3)
    if case == "same":            # s1 -> s1, R = 0.2
        cin, cout, radius = 8, 16, 0.2
        icell, ipos = _lattice(rng, (14, 12, 13), 0.85, h, center)
        ocell, opos = icell[: icell.shape[0] // 2 + 7], ipos[: icell.shape[0] // 2 + 7]
        ivox, ovox = h, h
    elif case == "fine_to_coarse":  # s1 -> s2, R = 0.4: outputs on every second cell
        cin, cout, radius = 8, 8, 0.4
        icell, ipos = _lattice(rng, (20, 18, 16), 0.8, h, center)
        ocell, opos = _lattice(rng, (10, 9, 8), 0.7, h, center, step=2)
        ivox, ovox = h, 2 * h
    elif case == "coarse_same":    # s2 -> s2, R = 0.4, spacing 0.1
        cin, cout, radius = 4, 8, 0.4
        icell, ipos = _lattice(rng, (12, 11, 10), 0.9, 2 * h, center)
        ocell, opos = icell, ipos
        ivox, ovox = 2 * h, 2 * h
    elif case == "over_cap":       # R = 10.2 voxels: 4,457 stencil offsets x 256 packed floats, above lat_build_filters' grid cap
        cin, cout, radius = pe.LAT_OVER_CAP["cin"], pe.LAT_OVER_CAP["cout"], pe.LAT_OVER_CAP["radius"]
        icell, ipos = _lattice(rng, (14, 12, 13), 0.85, h, center)
        ocell, opos = icell[:64], ipos[:64]  # (every output sees most of the inputs: few rows keep the float64 reference small)
        ivox, ovox = h, h
    else:                          # s2 -> s1, R = 0.4: outputs on the finer lattice
        cin, cout, radius = 4, 16, 0.4
        icell, ipos = _lattice(rng, (10, 9, 8), 0.8, h, center, step=2)
        ocell, opos = _lattice(rng, (19, 17, 15), 0.75, h, center)
        ivox, ovox = 2 * h, h
    return dict(center=center.astype(np.float32), icell=icell, ipos=ipos, ocell=ocell, opos=opos, ivox=ivox, ovox=ovox,
                cin=cin, cout=cout, radius=radius, ratio=0.5 if case == "coarse_to_fine" else round(ovox / ivox),
                feat=rng.normal(size=(ipos.shape[0], cin)).astype(np.float32),
                filt=rng.uniform(-1, 1, size=(4, 4, 4, cin, cout)).astype(np.float32),
                bias=rng.normal(size=cout).astype(np.float32))


def lattice_bar(L, idx, rs):
    """(ref, A, A1, kbar) of a lattice case on the equivalent neighbour list (poly6 on re-formed distances, bias)."""
    pw = PairWeights(L["opos"], L["ipos"], idx, rs, 2 * L["radius"], (4, 4, 4), window="poly6", f64=True)
    want, A, A1 = forward_bar(pw, L["filt"], L["feat"], window="poly6")
    return want + L["bias"], A + np.abs(L["bias"]), A1, kbar_of(pw, L["cin"])
