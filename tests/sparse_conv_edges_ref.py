"""The voxel convolution (csrc/sparse_conv.hip: sparse_conv_kernel, sparse_pair_geometry, sparse_filter_grad,
sparse_filter_reduce) at its chunk, tile, slab and flag edges: the cases, a float64 reference (tests/sparse_conv_ref.py's gather,
gather_grads and cells, wrapped for sign = -1 and for W_TRANSPOSED), a float32 emulation in the kernels' order of operations
with seeded faults, the bars, and a restatement of the slab plan -- shared by tests/test_sparse_conv_edges_cpu.py (no device)
and tests/test_gpu_sparse_conv_edges.py (the HIP kernels through ops.sparse_gather / ops.sparse_gather_backward).

A case is a dict: W [kz, ky, kx, c3, c4], row_pos [n_rows, 3], col_pos [n_cols, 3], x [n_cols, Cin], G [n_rows, Cout], idx int32,
row_splits int64, row_scale, col_scale, bias (or None), offset (x, y, z), voxel, extent, flags, out0 (what ``out`` holds before
an ACCUMULATE call, else None).  Cin and Cout are the channels of x and of out: (c3, c4) = (Cin, Cout), and (Cout, Cin) under
W_TRANSPOSED, where x has filter_dims[4] channels.  A list entry outside [0, n_cols) contributes nothing.

    out[r] = rs[r] * sum_{p in row r} cs[j_p] * W[cell(sign * (col_pos[j_p] - row_pos[r]))]^T x[j_p] (+ bias) (+ out0[r])

Geometry.  Rows sit on lattice points n(r) and columns on m(j) + u(j), |u| <= 0.29 per axis, scaled so that the filter
coordinate of the pair (r, j) is t = m(j) - sign * n(r) + u(j) on every axis: the pair's cell is clamp(m - sign * n) whatever
the list says, every coordinate is at least 0.2 from a half-integer (``margins``; the CPU test asserts it), and the clamp
engages wherever m - sign * n leaves [0, k).  ``pair_cells`` holds the cells the builder planned (integer arithmetic) and
``hits`` the set of them; the CPU test shows that sparse_conv_ref.cells finds the same from the float32 positions.

Left out: row_splits that reach past n_pairs (the header documents them for the kernel, but invert_neighbors_list promises
nothing about them), and non-finite filters.

Bars: |got - ref| <= k * 2^-24 * A element by element, A the same sum over absolute terms, k the roundings a term can see:
    out[r], L_r in-range pairs     one rounding for s * x; up to L_r - 1 adds into the row's image in LDS; the contraction chain
                                   over the non-zero k-steps, at most min(K, L_r) cells of round_up(Cin, 4) channels; the row
                                   scale, the bias and the accumulate add:   k = L_r + min(K, L_r) * round_up(Cin, 4) + 4
    dF[j], L'_j pairs refer to j   the same kernel on the inverted list, Cout channels in, neither bias nor accumulate:
                                   k = L'_j + min(K, L'_j) * round_up(Cout, 4) + 4
    dW[c], n_c pairs in cell c     rs * cs, s * u, (s u) * v: three roundings; n_c adds into the slab's partial sum, nslabs adds of
                                   the partial sums:   k = n_c + nslabs + 3
Each k is capped by the bar of tests/sparse_conv_ref.py, max(256, longest row + K * channels + 64): the asserted bar never
exceeds the old one.

Exact: a row without in-range pairs is the bias, or 0, or under ACCUMULATE out0 (+ bias); with ACCUMULATE out is
float32(plain + out0) bit for bit, plain the same call without the flag; dW is 0 in every cell no pair touches; dF is 0 for a
column no in-range pair refers to.  (Two identical calls give identical bits: the GPU test calls twice.)"""
import functools
import zlib

import numpy as np

import sparse_conv_ref as sr

F = np.float32
EPS = sr.EPS
NEGATE, W_TRANSPOSED, ACCUMULATE = 1, 2, 4
VOXEL = 0.5     # a power of two: extent = VOXEL * kx is exact
JITTER = 0.29
ORIGIN = np.array([1.5, -2.25, 0.75])

# the kernels' constants (csrc/sparse_conv.hip)
TILE_ROWS, IMG_CHUNK, COL_TILES_PER_PASS = 16, 240, 4
SLAB_PAIRS_MIN, SLABS_MAX, GRAD_CHUNK, STAGE, BATCH_MAX = 512, 512, 8192, 4096, 256


def _up(a, b):
    return -(-a // b) * b


# ---- the restated plans ---------------------------------------------------------------------------------------------------------

def fwd_plan(cin, cout, K):
    """The image plan of sparse_conv_kernel for Cin channels in, Cout out and K cells: channels per chunk CW, channel chunks
    ncc, cells per chunk cpc, cell chunks, 16-column tiles and passes over the list."""
    cin4 = _up(cin, 4)
    CW = min(IMG_CHUNK, cin4)
    cpc = IMG_CHUNK // CW
    tiles = -(-cout // 16)
    return dict(CW=CW, ncc=-(-cin4 // CW), cpc=cpc, cell_chunks=-(-K // cpc), col_tiles=tiles, passes=-(-tiles // COL_TILES_PER_PASS))


def slab_plan(n_pairs, filter_dims):
    """The filter gradient's plan: (slab_pairs, nslabs, batch, dW chunks, workspace bytes)."""
    T = int(np.prod([int(d) for d in filter_dims], dtype=np.int64))
    slab_pairs = max(SLAB_PAIRS_MIN, -(-n_pairs // SLABS_MAX))
    nslabs = max(1, -(-n_pairs // slab_pairs))
    batch = min(BATCH_MAX, STAGE // (int(filter_dims[3]) + int(filter_dims[4])))
    per = _up(max(n_pairs, 1) * 4, 256)
    return slab_pairs, nslabs, batch, -(-T // GRAD_CHUNK), 3 * per + _up(nslabs * T * 4, 256)


# ---- lists ------------------------------------------------------------------------------------------------------------------------

def transpose(idx, rs, n_cols):
    """The inverted list, as invert_neighbors_list gives it for an in-range list: row j (of n_cols) holds the rows r that refer
    to j, in the list's pair order (a stable sort of the in-range pairs by index).  -> (idx int32, row_splits int64)."""
    idx, rs = np.asarray(idx, np.int64), np.asarray(rs, np.int64)
    row = np.repeat(np.arange(len(rs) - 1), np.diff(rs))
    j = idx[:rs[-1]]
    ok = (j >= 0) & (j < n_cols)
    row, j = row[ok], j[ok]
    order = np.argsort(j, kind="stable")
    t_rs = np.concatenate([[0], np.cumsum(np.bincount(j, minlength=n_cols))]).astype(np.int64)
    return row[order].astype(np.int32), t_rs


def _in_range(case):
    """(row, col, position in the list) of the in-range pairs, in list order."""
    idx, rs = np.asarray(case["idx"], np.int64), case["row_splits"]
    row = np.repeat(np.arange(len(rs) - 1), np.diff(rs))
    ok = (idx >= 0) & (idx < len(case["col_pos"]))
    return row[ok], idx[ok], np.flatnonzero(ok)


# ---- float64 reference ------------------------------------------------------------------------------------------------------------

def sign_of(case):
    return -1.0 if case["flags"] & NEGATE else 1.0


def rel(case, i, j):
    """sign * (col_pos[j] - row_pos[i]) in float64."""
    return sign_of(case) * (case["col_pos"][j].astype(np.float64) - case["row_pos"][i].astype(np.float64))


def pairs_of(case):
    """The terms of the case as a sparse_conv_ref.Pairs (out-of-range entries dropped)."""
    i, j, _ = _in_range(case)
    cell = sr.cells(rel(case, i, j), case["kernel"], case["voxel"], case["offset"])
    coef = np.ones(len(i))
    if case["row_scale"] is not None:
        coef = coef * case["row_scale"][i].astype(np.float64)
    if case["col_scale"] is not None:
        coef = coef * case["col_scale"][j].astype(np.float64)
    return sr.Pairs(i, j, cell, coef, len(case["row_pos"]), len(case["col_pos"]))


def _w64(case):
    """The filter as [kz, ky, kx, Cin, Cout] float64, whichever way it is stored."""
    W = case["W"].astype(np.float64)
    return W.swapaxes(3, 4) if case["flags"] & W_TRANSPOSED else W


def margins(case):
    """(smallest distance of a filter coordinate from a half-integer, does the clamp engage at the low end of each axis, at the
    high end) over the in-range pairs; axes in (x, y, z) order."""
    i, j, _ = _in_range(case)
    k = np.asarray(case["kernel"][::-1])
    if not len(i):
        return np.inf, np.zeros(3, bool), np.zeros(3, bool)
    t = sr.filter_coords(rel(case, i, j), case["kernel"], case["voxel"], case["offset"])
    r = np.floor(t + 0.5)
    return float(np.abs(t - np.floor(t) - 0.5).min()), (r < 0).any(axis=0), (r > k - 1).any(axis=0)


def reference(case, gradients=True):
    """-> dict(out=(ref, A), dW=(ref, A), dF=(ref, A)) in float64; dW in the filter's stored layout."""
    pr = pairs_of(case)
    ap = sr.Pairs(pr.i, pr.j, pr.cell, np.abs(pr.coef), pr.n_out, pr.n_inp)
    W, x = _w64(case), case["x"].astype(np.float64)
    out, A = sr.gather(pr, W, x), sr.gather(ap, np.abs(W), np.abs(x))
    for extra in (case["bias"], case["out0"] if case["flags"] & ACCUMULATE else None):
        if extra is not None:
            out = out + extra.astype(np.float64)
            A = A + np.abs(extra.astype(np.float64))
    res = dict(out=(out, A))
    if gradients:
        G = case["G"].astype(np.float64)
        dW, dF, _ = sr.gather_grads(pr, W, x, G)
        aW, aF, _ = sr.gather_grads(ap, np.abs(W), np.abs(x), np.abs(G))
        if case["flags"] & W_TRANSPOSED:
            dW, aW = dW.swapaxes(3, 4), aW.swapaxes(3, 4)
        res["dW"], res["dF"] = (dW, aW), (dF, aF)
    return res


def bar_factors(case):
    """-> (k_out [n_rows], k_dF [n_cols], k_dW [K]) as the module docstring derives them, each capped by the old bar."""
    pr = pairs_of(case)
    cin, cout, K = case["cin"], case["cout"], case["K"]
    L = np.bincount(pr.i, minlength=pr.n_out)
    Lc = np.bincount(pr.j, minlength=pr.n_inp)
    n_c = np.bincount(pr.cell, minlength=K)
    nslabs = slab_plan(len(case["idx"]), case["W"].shape)[1]
    old_rows = max(sr.K_BAR, pr.longest_row() + K * cin + sr.PER_TERM)
    old_cols = max(sr.K_BAR, pr.longest_col() + K * cout + sr.PER_TERM)
    k_out = np.minimum(L + np.minimum(K, L) * _up(cin, 4) + 4, old_rows)
    k_dF = np.minimum(Lc + np.minimum(K, Lc) * _up(cout, 4) + 4, old_cols)
    k_dW = np.minimum(n_c + nslabs + 3, old_rows)
    return k_out, k_dF, k_dW


def bars(case, gradients=True):
    """-> dict(out=(ref, bar), dW=(ref, bar), dF=(ref, bar))."""
    R = reference(case, gradients)
    k_out, k_dF, k_dW = bar_factors(case)
    res = dict(out=(R["out"][0], k_out[:, None] * EPS * R["out"][1]))
    if gradients:
        res["dF"] = (R["dF"][0], k_dF[:, None] * EPS * R["dF"][1])
        res["dW"] = (R["dW"][0], k_dW.reshape(*case["kernel"], 1, 1) * EPS * R["dW"][1])
    return res


WORST = {}  # (group, what) -> worst err / bar, printed by the report tests of the two test files


def check(group, name, what, got, ref, bar):
    got = np.asarray(got)
    assert got.dtype == F and got.shape == ref.shape, (name, what, got.dtype, got.shape, ref.shape)
    assert np.all(np.isfinite(got)), f"{name} {what}: not finite"
    err = np.abs(got.astype(np.float64) - ref)
    pos = bar > 0
    r = float((err[pos] / bar[pos]).max()) if pos.any() else 0.0
    WORST[(group, what)] = max(WORST.get((group, what), 0.0), r)
    bad = err > bar
    assert not bad.any(), f"{name} {what}: {int(bad.sum())} elements over the bar, worst err/bar {r:.3g} at {np.argwhere(bad)[0].tolist()}"


def check_exact(case, got):
    """The exact-result rules of the module docstring on got = dict(out[, plain, dW, dF])."""
    pr = pairs_of(case)
    name = case["name"]
    if got.get("out") is not None:
        out = np.asarray(got["out"])
        empty = np.bincount(pr.i, minlength=pr.n_out) == 0
        want = np.zeros(out.shape, F) if case["bias"] is None else np.broadcast_to(case["bias"], out.shape)
        if case["flags"] & ACCUMULATE:
            want = case["out0"] if case["bias"] is None else (case["out0"] + case["bias"]).astype(F)
            assert got.get("plain") is not None, "an ACCUMULATE case needs the same call without the flag"
            both = (np.asarray(got["plain"]) + case["out0"]).astype(F)
            assert np.array_equal(out.view(np.int32), both.view(np.int32)), f"{name}: out is not float32(plain + out0) bit for bit"
        assert np.array_equal(out[empty], want[empty]), f"{name}: a row without in-range pairs is not exactly the bias / 0 / out0 (+ bias)"
    if got.get("dW") is not None:
        dW = np.asarray(got["dW"]).reshape(case["K"], -1)
        untouched = np.bincount(pr.cell, minlength=case["K"]) == 0
        assert np.all(dW[untouched] == 0), f"{name}: dW is not 0 in a cell no pair touches"
    if got.get("dF") is not None:
        lonely = np.bincount(pr.j, minlength=pr.n_inp) == 0
        assert np.all(np.asarray(got["dF"])[lonely] == 0), f"{name}: dF is not 0 for a column no in-range pair refers to"


def check_case(case, got, group=None):
    """Every bar and exact rule of a case on host arrays got = dict(out[, plain, dW, dF]) (None / absent: not computed)."""
    B = bars(case, gradients=any(got.get(k) is not None for k in ("dW", "dF")))
    g = group or case["group"]
    for what in ("out", "dW", "dF"):
        if got.get(what) is not None:
            check(g, case["name"], what, got[what], B[what][0], B[what][1])
    check_exact(case, got)


# ---- cases ------------------------------------------------------------------------------------------------------------------------

CHANNELS = ((1, 1), (3, 5), (4, 16), (5, 17), (16, 15), (33, 64), (60, 65), (61, 3), (120, 7), (121, 4), (240, 16), (241, 9), (243, 5),
            (481, 6), (7, 129), (65, 241))
CELLS = ((32, (1, 1, 7)), (32, (2, 2, 2)), (32, (1, 2, 7)), (32, (1, 3, 5)),
         (5, (3, 3, 3)), (5, (2, 3, 5)), (5, (1, 1, 31)), (5, (4, 4, 4)),
         (1, (3, 4, 5)), (1, (4, 4, 4)), (1, (5, 5, 5)))
CELLS_COUT = {32: 5, 5: 7, 1: 3}
OFFSET_XYZ = (0.25, -0.5, 0.125)            # of [2, 3, 5] and [3, 4, 5]: differs on all three axes
ROWS_N = (1, 15, 16, 17, 63, 64, 65, 129)
ROW_LENGTHS = (0, 1, 2, 3, 4, 5, 63, 64, 65, 300, 0, 0, 7, 40, 9, 0, 3, 1, 5, 7)
ROW_300, ROW_40, ROW_ALL_BAD, ROW_LAST_ONLY = 9, 13, 18, 19
SLAB_PAIRS = (1, 255, 256, 257, 511, 512, 513, 1024, 1025, 1537)
SLAB_WIDTHS = ((5, 7), (4, 13), (65, 241))
LATTICE = ((0, 0, 0), (1, 0, 0), (0, -1, 0), (0, 0, 1), (-1, 1, 0))
GROUPS = ("channels", "cells", "rows", "slabs", "accumulate")


def _kname(kernel):
    return "x".join(str(k) for k in kernel)


def case_names(group):
    if group == "channels":
        return [f"{ci}x{co}_cpc{fwd_plan(ci, co, 8)['cpc']}_ncc{fwd_plan(ci, co, 8)['ncc']}_nt{fwd_plan(ci, co, 8)['col_tiles']}_f{f}"
                for ci, co in CHANNELS for f in (0, W_TRANSPOSED)]
    if group == "cells":
        names = []
        for ci, k in CELLS:
            flags = range(8) if k == (2, 3, 5) else (0,)
            names += [f"c{ci}_k{_kname(k)}_K{int(np.prod(k))}_cpc{fwd_plan(ci, 1, 1)['cpc']}_f{f}" for f in flags]
        return names
    if group == "rows":
        return [f"n{n}" for n in ROWS_N] + ["lengths", "lengths_oob"]
    if group == "slabs":
        return [f"p{p}_{ci}x{co}_batch{slab_plan(p, (2, 2, 2, ci, co))[2]}" for p in SLAB_PAIRS for ci, co in SLAB_WIDTHS] + \
            ["p1537_5x7_dead_slab", "p1025_5x7_cell_in_second_slab"]
    if group == "accumulate":
        return ["bias_f4", "nobias_f4", "bias_negate_transposed_f7", "no_pairs_bias_f4", "no_pairs_nobias_f4", "no_pairs_bias_f0"]
    raise KeyError(group)


def _rng(*key):
    return np.random.default_rng(zlib.crc32("/".join(str(k) for k in key).encode()))


def _flat(t, kernel):
    """Flat cell (z, y, x order) of lattice coordinates t [.., 3] in (x, y, z) order, clamped."""
    k = np.asarray(kernel[::-1], np.int64)
    c = np.clip(np.asarray(t, np.int64), 0, k - 1)
    return (c[..., 2] * k[1] + c[..., 1]) * k[0] + c[..., 0]


def _unflat(c, kernel):
    kz, ky, kx = kernel
    return (c % kx, (c // kx) % ky, c // (kx * ky))


def _csr(lengths):
    return np.concatenate([[0], np.cumsum(np.asarray(lengths, np.int64))]).astype(np.int64)


def _assemble(name, group, kernel, cin, cout, n, m, idx, rs, flags, offset=(0.0, 0.0, 0.0), scales=True, bias=True, only=None):
    """The case over rows at lattice points n [n_rows, 3] and columns at m [n_cols, 3] (x, y, z), the list as given."""
    kernel = tuple(int(k) for k in kernel)
    rng = _rng(group, name)
    sign = -1.0 if flags & NEGATE else 1.0
    k = np.asarray(kernel[::-1], np.float64)
    n, m = np.asarray(n, np.int64).reshape(-1, 3), np.asarray(m, np.int64).reshape(-1, 3)
    n_rows, n_cols = len(n), len(m)
    ext = float(sr.extent(kernel, VOXEL))
    step = ext / k
    off = np.asarray(offset, np.float64)
    u = rng.uniform(-JITTER, JITTER, size=(n_cols, 3))
    row_pos = (ORIGIN + n * step).astype(F)
    col_pos = (ORIGIN + sign * (m + u - (k - 1.0) / 2.0 - off) * step).astype(F)
    c3, c4 = (cout, cin) if flags & W_TRANSPOSED else (cin, cout)
    idx, rs = np.asarray(idx, np.int32), np.asarray(rs, np.int64)
    c = dict(name=name, group=group, kernel=kernel, K=int(np.prod(kernel)), cin=cin, cout=cout, flags=int(flags), voxel=VOXEL, extent=ext,
             offset=off, row_pos=row_pos, col_pos=col_pos, idx=idx, row_splits=rs, only=only,
             W=rng.uniform(-1, 1, size=(*kernel, c3, c4)).astype(F),
             x=rng.normal(size=(n_cols, cin)).astype(F), G=rng.normal(size=(n_rows, cout)).astype(F),
             row_scale=rng.uniform(0.5, 1.5, size=n_rows).astype(F) if scales else None,
             col_scale=rng.uniform(0.5, 1.5, size=n_cols).astype(F) if scales else None,
             bias=rng.normal(size=cout).astype(F) if bias else None,
             out0=rng.normal(size=(n_rows, cout)).astype(F) if flags & ACCUMULATE else None)
    row = np.repeat(np.arange(n_rows), np.diff(rs))
    ok = (idx >= 0) & (idx < n_cols)
    c["pair_cells"] = _flat(m[idx[ok]] - int(sign) * n[row[ok]], kernel)
    c["hits"] = frozenset(int(v) for v in np.unique(c["pair_cells"]))
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def _bad(kind, n_cols):
    return (-1, n_cols, n_cols + 7)[kind % 3]


@functools.lru_cache(maxsize=None)
def _random_geometry(key, kernel, n_rows, n_cols, max_len, total=None):
    """Lattice points and a random list: rows of 0 to max_len pairs (or ``total`` pairs dealt to the rows at random), the first
    and the last row non-empty, row 3 empty where there is one, the last column referred to by nobody."""
    rng = _rng("geometry", key, kernel, n_rows, n_cols, max_len, total)
    kx, ky, kz = kernel[::-1]
    n = rng.integers(-1, 2, size=(n_rows, 3))
    m = np.stack([rng.integers(-1, k + 1, size=n_cols) for k in (kx, ky, kz)], axis=1)
    if total is None:
        lengths = rng.integers(0, max_len + 1, size=n_rows)
        lengths[0], lengths[-1] = max(lengths[0], 1), max_len
        if n_rows > 4:
            lengths[3] = 0
    else:
        lengths = np.bincount(rng.integers(0, n_rows, size=total), minlength=n_rows)
    rs = _csr(lengths)
    idx = rng.integers(0, max(n_cols - 1, 1), size=int(rs[-1])).astype(np.int32)
    return n, m, idx, rs


def _placed(rows, flags):
    """Rows of targets -> (n, m, idx, row_splits).  A target is (tx, ty, tz, dup): the pair's lattice coordinate before the clamp
    and which of the columns at that point it is; or ("bad", kind): an out-of-range entry.  Row r sits at LATTICE[r % 5]."""
    sign = -1 if flags & NEGATE else 1
    n = np.asarray([LATTICE[r % len(LATTICE)] for r in range(len(rows))], np.int64).reshape(-1, 3)
    pool, m, idx = {}, [], []
    for r, targets in enumerate(rows):
        for t in targets:
            if t[0] == "bad":
                idx.append(-1000 - t[1])
                continue
            key = (t[0] + sign * n[r, 0], t[1] + sign * n[r, 1], t[2] + sign * n[r, 2], t[3])
            if key not in pool:
                pool[key] = len(m)
                m.append(key[:3])
            idx.append(pool[key])
    m.append((0, 0, 0))  # one column nobody refers to
    idx = np.asarray(idx, np.int64)
    bad = idx <= -1000
    idx[bad] = [_bad(int(-1000 - v), len(m)) for v in idx[bad]]
    return n, np.asarray(m, np.int64), idx.astype(np.int32), _csr([len(t) for t in rows])


def _cells_rows(cin, kernel, rng):
    """The targets of a ``cells`` case: every chunk edge straddled by one row, every cell hit, the clamp at both ends of every
    axis with more than one cell, two empty rows."""
    K = int(np.prod(kernel))
    cpc = fwd_plan(cin, 1, K)["cpc"]
    ks = kernel[::-1]

    def inside():
        return tuple(int(rng.integers(0, k)) for k in ks)

    rows = []
    for e in range(cpc, K, cpc):
        row = [_unflat(e - 1, kernel), _unflat(e, kernel), inside(), inside()]
        rows.append([row[i] for i in rng.permutation(4)])
    rows.insert(min(1, len(rows)), [])
    allc = rng.permutation(K)
    rows += [[_unflat(int(c), kernel) for c in allc[b:b + 9]] for b in range(0, K, 9)]
    rows.append([])
    for a, k in enumerate(ks):
        if k > 1:
            lo, hi = list(inside()), list(inside())
            lo[a], hi[a] = -1, k
            rows.append([tuple(lo), tuple(hi), inside()])
    return [[(*t, int(rng.integers(0, 2))) for t in row] for row in rows]


def _lengths_rows(kernel, oob, rng):
    """ROW_LENGTHS: the row of 300 in one cell (over six columns), the row of 40 one column forty times; ``oob``: about a tenth
    of the other entries out of range, one row all out of range, one whose only in-range entry is its last."""
    ks = kernel[::-1]
    rows = []
    for r, length in enumerate(ROW_LENGTHS):
        if r == ROW_300:
            rows.append([(1, 2, 1, q % 6) for q in range(length)])
        elif r == ROW_40:
            rows.append([(4, 0, 0, 3)] * length)
        else:
            rows.append([(*(int(rng.integers(-1, k + 1)) for k in ks), int(rng.integers(0, 3))) for _ in range(length)])
    if oob:
        kind = 0
        for r, row in enumerate(rows):
            if r in (ROW_ALL_BAD, ROW_LAST_ONLY):
                for q in range(len(row) - (r == ROW_LAST_ONLY)):
                    row[q] = ("bad", q)
                continue
            for q in range(len(row) - 1):  # (the last entry of every row stays in range)
                if rng.uniform() < 0.1:
                    row[q] = ("bad", kind)
                    kind += 1
    return rows


@functools.lru_cache(maxsize=512)
def case(group, name):
    """The case's operands as read-only numpy arrays (see the module docstring)."""
    tok = name.split("_")
    flags = int(tok[-1][1:]) if tok[-1][0] == "f" and tok[-1][1:].isdigit() else 0
    if group == "channels":
        cin, cout = (int(v) for v in tok[0].split("x"))
        n, m, idx, rs = _random_geometry("channels", (2, 2, 2), 40, 40, 12)
        return _assemble(name, group, (2, 2, 2), cin, cout, n, m, idx, rs, flags, offset=(-0.5, -0.5, -0.5))
    if group == "cells":
        cin, kernel = int(tok[0][1:]), tuple(int(v) for v in tok[1][1:].split("x"))
        n, m, idx, rs = _placed(_cells_rows(cin, kernel, _rng("cells", cin, kernel)), flags)
        off = OFFSET_XYZ if kernel in ((2, 3, 5), (3, 4, 5)) else tuple(sr.default_offset(kernel))
        return _assemble(name, group, kernel, cin, CELLS_COUT[cin], n, m, idx, rs, flags, offset=off)
    if group == "rows":
        kernel = (2, 3, 5)
        if name.startswith("lengths"):
            n, m, idx, rs = _placed(_lengths_rows(kernel, name.endswith("oob"), _rng("lengths")), 0)
        else:
            n, m, idx, rs = _random_geometry("rows", kernel, int(name[1:]), 30, 6)
        return _assemble(name, group, kernel, 5, 7, n, m, idx, rs, 0, offset=OFFSET_XYZ)
    if group == "slabs":
        kernel = (2, 2, 2)
        p = int(tok[0][1:])
        cin, cout = (int(v) for v in tok[1].split("x"))
        n, m, idx, rs = _random_geometry("slabs", kernel, 40, 40, 0, total=p)
        idx = np.array(idx)
        if "dead" in name:          # the second slab: nothing in range
            idx[512:1024] = [_bad(q, 40) for q in range(512)]
        if "cell" in name:          # cell 7 = (1, 1, 1) only from the second slab: rows at the origin, column 38 alone in it
            n, m = np.zeros_like(n), np.array(m)
            m[:, 0] = np.minimum(m[:, 0], 0)
            m[38] = (1, 1, 1)
            idx[idx == 38] = 5
            idx[600:1000:7] = 38
        return _assemble(name, group, kernel, cin, cout, n, m, idx, rs, 0, offset=(-0.5, -0.5, -0.5), only=("dW",))
    if group == "accumulate":
        n, m, idx, rs = _random_geometry("accumulate", (2, 2, 2), 40, 40, 12)
        if name.startswith("no_pairs"):
            idx, rs = idx[:0], np.zeros_like(rs)
        return _assemble(name, group, (2, 2, 2), 5, 7, n, m, idx, rs, flags, offset=(-0.5, -0.5, -0.5), bias="nobias" not in name)
    raise KeyError(group)


def all_cases():
    return [(g, n) for g in GROUPS for n in case_names(g)]


def derive(c, name, **changes):
    """A case with some operands replaced (the arrays stay read-only; the planned cells are dropped: they may no longer hold)."""
    d = dict(c, name=name, **changes)
    d.pop("pair_cells", None), d.pop("hits", None)
    return d


def layer_cases():
    """(case for ops.sparse_conv, case for ops.sparse_conv_transpose) twice: 65x241 and a [3, 3, 3] cells case.  SparseConv:
    flags 0, the column scale as inp_importance, normalize (the row scale is 1 / |row|, 0 for an empty row).  The transpose:
    NEGATE, the row scale as out_importance, no column scale.  (2 * offset is an integer in both, so the negated coordinates
    keep their distance from the half-integers.)"""
    res = []
    for group, name in (("channels", "65x241_cpc3_ncc1_nt16_f0"), ("cells", "c5_k3x3x3_K27_cpc30_f0")):
        c = case(group, name)
        cnt = np.diff(c["row_splits"]).astype(F)
        norm = np.where(cnt > 0, F(1) / np.maximum(cnt, F(1)), F(0)).astype(F)
        res.append((derive(c, name + "_SparseConv", row_scale=norm, group="layers"),
                    derive(c, name + "_SparseConvTranspose", flags=NEGATE, col_scale=None, group="layers")))
    return res


def from_sparse_conv_ref(c, transposed):
    """A tests/sparse_conv_ref.py Case as a case of this module: SparseConv over its list, or SparseConvTranspose over the
    inversion of the input points' list.  (The scale of ``normalize`` stays in float64, as that module takes it.)"""
    n_out, n_inp = len(c.out), len(c.inp)
    if transposed:
        tidx, trs = c.transpose_list
        idx, rs = transpose(tidx, trs, n_out)
        cnt = np.diff(trs).astype(np.float64)
        row_scale = c.out_importance
        col_scale = (1.0 / np.maximum(cnt, 1.0) * (cnt > 0)) if c.normalize else None
    else:
        idx, rs = c.conv_list
        cnt = np.diff(rs).astype(np.float64)
        row_scale = (1.0 / np.maximum(cnt, 1.0) * (cnt > 0)) if c.normalize else None
        col_scale = c.inp_importance
    return dict(name=c.name, group="sparse_conv_ref", kernel=tuple(c.kernel_size), K=c.K, cin=c.cin, cout=c.cout,
                flags=NEGATE if transposed else 0, voxel=c.voxel, extent=float(sr.extent(c.kernel_size, c.voxel)), offset=c.offset,
                row_pos=c.out, col_pos=c.inp, idx=idx, row_splits=rs, only=None, W=c.W, x=c.F, G=c.G, row_scale=row_scale,
                col_scale=col_scale, bias=c.bias, out0=None)


# ---- float32 emulation in the kernels' order ------------------------------------------------------------------------------------------

MUTATIONS = ("drop_second_channel_chunk", "drop_last_cell_chunk", "carry_acc_across_column_passes", "stop_at_cout_64", "read_past_cin",
             "swap_ky_kx", "ignore_negate", "filter_grad_ignores_transposed", "drop_cell_part_across_dw_chunk", "drop_last_batch",
             "drop_last_slab", "keep_out_of_range_pairs", "accumulate_overwrites")


def _fma(a, b, c):
    """float32 fma(a, b, c): the product of two float32 is exact in float64; one rounding of the float64 sum apart, exact."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)


def _flat_read(a, index):
    """a.ravel()[index], 0 where the index is past the array (what a read past the end is taken to give)."""
    flat = np.asarray(a).ravel()
    index = np.asarray(index, np.int64)
    ok = (index >= 0) & (index < flat.size)
    return np.where(ok, flat[np.where(ok, index, 0)], F(0)).astype(F)


def _params(case, mutate=None):
    """SparseParams of the forward call."""
    flags = case["flags"]
    W = case["W"]
    tr = bool(flags & W_TRANSPOSED)
    return dict(W=W, kernel=case["kernel"], cw_in=W.shape[3], cw_out=W.shape[4], transposed=tr, cin=case["cin"], cout=case["cout"],
                row_pos=case["row_pos"], col_pos=case["col_pos"], x=case["x"], rsc=case["row_scale"], csc=case["col_scale"],
                idx=np.asarray(case["idx"], np.int64), rs=case["row_splits"], n_cols=len(case["col_pos"]),
                inv_extent=F(1) / F(case["extent"]), sign=F(-1) if (flags & NEGATE and mutate != "ignore_negate") else F(1),
                off=np.asarray(case["offset"], F), bias=case["bias"], out0=case["out0"] if flags & ACCUMULATE else None)


def emulate_cells(P, r, j, mutate=None):
    """sparse_cell in float32 for the pairs (r, j)."""
    kz, ky, kx = P["kernel"]
    d = (P["sign"] * (P["col_pos"][j] - P["row_pos"][r]).astype(F)).astype(F).reshape(-1, 3)
    c = []
    for a, k in enumerate((kx, ky, kz)):
        t = (d[:, a] * P["inv_extent"]).astype(F)
        t = (t * F(k) + F(k // 2)).astype(F)
        if k % 2 == 0:
            t = (t - F(0.5)).astype(F)
        t = (t + P["off"][a]).astype(F)
        q = np.where(t >= 0, np.floor(t + F(0.5)), np.ceil(t - F(0.5))).astype(np.int64)  # roundf
        c.append(np.clip(q, 0, k - 1))
    if mutate == "swap_ky_kx":
        return (c[2] * kx + c[1]) * ky + c[0]
    return (c[2] * ky + c[1]) * kx + c[0]


def emulate_gather(P, mutate=None):
    """sparse_conv_kernel: -> out float32 [n_rows, cout].  Per tile of 16 rows the image of every row is summed in pair order;
    per pass of four 16-column tiles the accumulators start at zero and take, cell chunk after cell chunk and channel chunk
    after channel chunk, the k-steps of four channels that are not all zero, the four products of a step in order."""
    kz, ky, kx = P["kernel"]
    K, cin, cout, n_cols = kz * ky * kx, P["cin"], P["cout"], P["n_cols"]
    plan = fwd_plan(cin, cout, K)
    CW, ncc, cpc, NT = plan["CW"], plan["ncc"], plan["cpc"], plan["col_tiles"]
    cin4 = _up(cin, 4)
    idx, rs = P["idx"], P["rs"]
    n_rows = len(rs) - 1
    past = mutate == "read_past_cin"
    # the filter as the contraction reads it: [K, cin4, 16 NT], zero where the guard ch < cin && co < cout says so
    ch, co = np.meshgrid(np.arange(cin4), np.arange(16 * NT), indexing="ij")
    e = co * P["cw_out"] + ch if P["transposed"] else ch * P["cw_out"] + co
    guard = ((ch < cin) | past) & (co < cout)
    wcell = P["cw_in"] * P["cw_out"]
    M = np.stack([np.where(guard, _flat_read(P["W"], c * wcell + e), F(0)) for c in range(K)]).astype(F)
    out = np.zeros((n_rows, cout), F) if P["out0"] is None else np.array(P["out0"], F)
    old = out.copy()
    for tile0 in range(0, n_rows, TILE_ROWS):
        rows = range(tile0, min(n_rows, tile0 + TILE_ROWS))
        img = np.zeros((TILE_ROWS, K, cin4), F)
        for r in rows:
            for q in range(int(rs[r]), int(rs[r + 1])):
                j = int(idx[q])
                if j < 0 or j >= n_cols:
                    if mutate != "keep_out_of_range_pairs":
                        continue
                    j = min(max(j, 0), n_cols - 1)
                cell = int(emulate_cells(P, r, j, mutate)[0])
                s = P["csc"][j] if P["csc"] is not None else F(1)
                g = np.arange(cin4)
                xj = np.where((g < cin) | past, _flat_read(P["x"], j * cin + g), F(0)).astype(F)
                img[r - tile0, cell] = (img[r - tile0, cell] + (s * xj).astype(F)).astype(F)
        live = (img.reshape(TILE_ROWS, K, cin4 // 4, 4) != 0).any(axis=(0, 3))  # the wave ballot of every k-step
        acc = None
        for n0 in range(0, NT, COL_TILES_PER_PASS):
            if mutate == "stop_at_cout_64" and n0 > 0:
                break
            cols = slice(16 * n0, 16 * min(NT, n0 + COL_TILES_PER_PASS))
            width = cols.stop - cols.start
            if acc is None or mutate != "carry_acc_across_column_passes":
                acc = np.zeros((TILE_ROWS, width), F)
            acc = np.ascontiguousarray(acc[:, :width])
            chunks = list(range(0, K, cpc))
            for c0 in chunks:
                if mutate == "drop_last_cell_chunk" and len(chunks) > 1 and c0 == chunks[-1]:
                    continue
                for cc in range(ncc):
                    if mutate == "drop_second_channel_chunk" and cc == 1:
                        continue
                    ch0 = cc * CW
                    cw = min(CW, cin4 - ch0)
                    for c in range(c0, min(K, c0 + cpc)):
                        for qd in range(cw // 4):
                            g0 = ch0 + 4 * qd
                            if not live[c, g0 // 4]:
                                continue
                            for kq in range(4):
                                acc = _fma(img[:, c, g0 + kq:g0 + kq + 1], M[c, g0 + kq:g0 + kq + 1, cols], acc)
            for r in rows:
                v = acc[r - tile0]
                v = (v * (P["rsc"][r] if P["rsc"] is not None else F(1))).astype(F)
                lo, hi = cols.start, min(cols.stop, cout)
                v = v[:hi - lo]
                if P["bias"] is not None:
                    v = (v + P["bias"][lo:hi]).astype(F)
                if P["out0"] is not None and mutate != "accumulate_overwrites":
                    v = (v + old[r, lo:hi]).astype(F)
                out[r, lo:hi] = v
    return out


def emulate_feature_grad(P, G, mutate=None):
    """The feature gradient: sparse_conv_kernel on the inverted list, rows and columns swapped, the other sign, W the other way."""
    inv_idx, inv_rs = transpose(P["idx"], P["rs"], P["n_cols"])
    T = dict(P, transposed=not P["transposed"], cin=P["cout"], cout=P["cin"], row_pos=P["col_pos"], col_pos=P["row_pos"], x=G,
             rsc=P["csc"], csc=P["rsc"], idx=np.asarray(inv_idx, np.int64), rs=inv_rs, n_cols=len(P["rs"]) - 1, sign=F(-P["sign"]),
             bias=None, out0=None)
    return emulate_gather(T, mutate)


def emulate_filter_grad(P, G, mutate=None):
    """sparse_pair_geometry, sparse_filter_grad, sparse_filter_reduce: per slab of pairs and chunk of dW the slab's pairs batch by
    batch and in order, each clipped to the chunk; then the slabs in order.  -> dW in the filter's stored shape."""
    kz, ky, kx = P["kernel"]
    K, cu, cv, n_cols = kz * ky * kx, P["cw_in"], P["cw_out"], P["n_cols"]
    CC = cu * cv
    T = K * CC
    idx, rs = P["idx"], P["rs"]
    n_pairs = len(idx)
    slab_pairs, nslabs, batch, nchunks, _ = slab_plan(n_pairs, P["W"].shape)
    pair_row = np.full(n_pairs, -1, np.int64)
    pair_cell = np.zeros(n_pairs, np.int64)
    pair_scale = np.zeros(n_pairs, F)
    for r in range(len(rs) - 1):
        rsv = P["rsc"][r] if P["rsc"] is not None else F(1)
        for q in range(int(rs[r]), int(rs[r + 1])):
            j = int(idx[q])
            if j < 0 or j >= n_cols:
                if mutate != "keep_out_of_range_pairs":
                    continue
                j = min(max(j, 0), n_cols - 1)
            pair_row[q], pair_cell[q] = r, int(emulate_cells(P, r, j, mutate)[0])
            pair_scale[q] = F(rsv * (P["csc"][j] if P["csc"] is not None else F(1)))
    from_g_u = P["transposed"] and mutate != "filter_grad_ignores_transposed"
    total = np.zeros(T, F)
    for s in range(nslabs):
        part = np.zeros(T, F)
        q0, q1 = s * slab_pairs, min(n_pairs, (s + 1) * slab_pairs)
        nbatches = -(-(q1 - q0) // batch)
        if mutate == "drop_last_slab" and nslabs > 1 and s == nslabs - 1:
            q1 = q0
        for chunk in range(nchunks):
            e0, e1 = chunk * GRAD_CHUNK, min(T, (chunk + 1) * GRAD_CHUNK)
            for q in range(q0, q1):
                if pair_row[q] < 0:
                    continue
                if mutate == "drop_last_batch" and nbatches > 1 and (q - q0) // batch == nbatches - 1:
                    continue
                cbase = int(pair_cell[q]) * CC
                if cbase >= e1 or cbase + CC <= e0:
                    continue
                if mutate == "drop_cell_part_across_dw_chunk" and not e0 <= cbase < e1:
                    continue
                lo, hi = max(cbase, e0), min(cbase + CC, e1)
                ab = np.arange(lo - cbase, hi - cbase)
                a, bb = ab // cv, ab % cv
                r, j = int(pair_row[q]), min(max(int(idx[q]), 0), n_cols - 1)
                # U has cw_in channels, V cw_out: x and grad_out, or the other way round with W_TRANSPOSED
                U = _flat_read(G, r * cu + a) if from_g_u else _flat_read(P["x"], j * cu + a)
                V = _flat_read(P["x"], j * cv + bb) if from_g_u else _flat_read(G, r * cv + bb)
                part[lo:hi] = (part[lo:hi] + ((pair_scale[q] * U).astype(F) * V).astype(F)).astype(F)
        total = (total + part).astype(F)
    return total.reshape(P["W"].shape)


def emulate(case, mutate=None):
    """The forward and both gradients as the kernels order them: -> dict(out, plain, dW, dF) in float32 (``plain``: the call
    without ACCUMULATE, for a case with it; a case with ``only`` gets just those)."""
    only = case["only"] or ("out", "dW", "dF")
    P = _params(case, mutate)
    got = {}
    if "out" in only:
        got["out"] = emulate_gather(P, mutate)
        if case["flags"] & ACCUMULATE:
            got["plain"] = emulate_gather(dict(P, out0=None), mutate)
    B = dict(P, bias=None, out0=None)
    if "dW" in only:
        got["dW"] = emulate_filter_grad(B, case["G"], mutate)
    if "dF" in only:
        got["dF"] = emulate_feature_grad(B, case["G"], mutate)
    return got
