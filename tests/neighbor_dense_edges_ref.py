"""PointNet's neighbour-sum kernels (csrc/pointnet.hip: nd_gather_mfma<1|2>, nd_bwd_weight, nd_bwd_weight_reduce) at their row,
tile and slab edges: the cases, a float64 reference for CSR and padded lists, a float32 emulation in the kernels' order of
operations, and the bars -- shared by tests/test_neighbor_dense_edges_cpu.py (the bars hold for the emulation and catch seeded
faults of it, without a GPU) and tests/test_gpu_neighbor_dense_edges.py (the HIP kernels against the float64 reference).

A list is (idx int32 [P], begin int64 [n_out], count int32 [n_out], n_in): row r holds idx[begin[r] : begin[r] + count[r]].  A
CSR list has begin = row_splits[:-1], count = diff(row_splits); the padded form has begins a fixed stride apart and slots past
a row's count that hold valid-looking indices.  A pair whose index is outside [0, n_in) contributes nothing.

What the kernel does per output row r (c_r its in-range pairs, in list order):
    S_r   = ((act(x_j1) + act(x_j2)) + ...)                  c_r - 1 float32 adds per channel
    out_r = fma chain over the channels 0 .. cin_p - 1 of S_r W   cin (+ at most 3 exact zeros of padding)
            + c_r * b  + residual_r                          two roundings, one rounding
The input gradient is the same kernel on the inverted list with G for x and W^T for W, masked by x > 0; the weight gradient
sums S_r^T G_r over slabs of rows (rows_per_slab a multiple of 4, four rows per matrix instruction) and then over the slabs,
with the count c_r as channel cin of [S | c].

Bars: k * 2^-24 * A, A the same sum over absolute terms, k the roundings a term can see plus 2 for second-order terms:
    out[r]   k = c_r + cin + 4      (c_r - 1) + (cin + 1) + 2 + 1 and the margin: = c_r + cin + 3, one unit spare
    dx[j]    k = c'_j + cout + 4    c'_j the pairs referring to j
    dW       k = Lmax + n_nz + 4    Lmax the longest in-range row, n_nz the rows of G that are not all zero
    db       k = n_nz + 4           A = sum_r c_r |G_r|
Exact: a row without in-range pairs is the residual or 0; dx is 0 where x <= 0 under relu and in rows past n_in."""
import functools

import numpy as np

F = np.float32
EPS = 2.0 ** -24

# ---- the row-length list ------------------------------------------------------------------------------------------------------

EDGE_LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 640, 0, 3, 5, 0, 64, 1, 130, 0, 0, 7)
EDGE_N_IN, EDGE_X_ROWS = 300, 320
PAD_STRIDE = 656
ROW_65, ROW_640, ROW_130 = 5, 9, 16


def _csr(lengths):
    lengths = np.asarray(lengths, np.int64)
    rs = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return rs[:-1].copy(), lengths.astype(np.int32), rs


@functools.lru_cache(maxsize=None)
def edge_rows(oob=True):
    """-> (idx, begin, count, row_splits) of EDGE_ROWS over n_in = 300.  ``oob``: about a tenth of the entries are -1, n_in or
    n_in + 7, the first 64 entries of the row of 130 are all out of range and the row of 65 has only its last entry in range;
    without it every entry is in range (the rows then have exactly EDGE_LENGTHS in-range pairs)."""
    rng = np.random.default_rng(20)
    begin, count, rs = _csr(EDGE_LENGTHS)
    n = EDGE_N_IN
    idx = rng.integers(0, n, size=int(rs[-1])).astype(np.int32)
    idx[rs[ROW_640 + 1] - 1] = n - 1  # the last pair of the longest row reads the last row of x ...
    idx[rs[ROW_640]] = 0              # ... and its first the first
    if oob:
        bad = np.flatnonzero(rng.uniform(size=idx.size) < 0.1)
        idx[bad] = np.asarray([-1, n, n + 7], np.int32)[np.arange(bad.size) % 3]
        b = rs[ROW_130]
        idx[b:b + 64] = np.asarray([-1, n, n + 7], np.int32)[np.arange(64) % 3]
        idx[b + 64:b + 130] = rng.integers(0, n, size=66)
        b = rs[ROW_65]
        idx[b:b + 64] = np.asarray([n + 7, -1, n], np.int32)[np.arange(64) % 3]
        idx[b + 64] = 17
        idx[rs[ROW_640 + 1] - 1] = n - 1
        idx[rs[7 + 1] - 1] = 5        # the last pairs of the rows of 128 and 129 are in range
        idx[rs[8 + 1] - 1] = 6
    for a in (idx, begin, count, rs):
        a.setflags(write=False)
    return idx, begin, count, rs


@functools.lru_cache(maxsize=None)
def edge_rows_padded():
    """The same rows a stride of 656 apart; every slot past a row's count holds a valid in-range index."""
    idx, begin, count, rs = edge_rows(True)
    rng = np.random.default_rng(21)
    n_out = len(count)
    pidx = rng.integers(0, EDGE_N_IN, size=n_out * PAD_STRIDE).astype(np.int32)
    pbegin = (np.arange(n_out, dtype=np.int64) * PAD_STRIDE)
    for r in range(n_out):
        pidx[pbegin[r]:pbegin[r] + count[r]] = idx[begin[r]:begin[r] + count[r]]
    for a in (pidx, pbegin):
        a.setflags(write=False)
    return pidx, pbegin, count


def transpose(idx, rs, n_in):
    """The list whose inversion is the given one: row j (of n_in) holds the rows r of the given list that refer to j, in the
    given list's pair order (a stable sort of the in-range pairs by index).  -> (idx int32, row_splits int64 [n_in + 1]);
    its indices range over the given list's rows."""
    idx, rs = np.asarray(idx, np.int64), np.asarray(rs, np.int64)
    row = np.repeat(np.arange(len(rs) - 1), np.diff(rs))
    j = idx[:rs[-1]]
    ok = (j >= 0) & (j < n_in)
    row, j = row[ok], j[ok]
    order = np.argsort(j, kind="stable")
    t_rs = np.concatenate([[0], np.cumsum(np.bincount(j, minlength=n_in))]).astype(np.int64)
    return row[order].astype(np.int32), t_rs


def random_rows(rng, n_out, n_in, max_len, oob=0.1):
    lengths = rng.integers(0, max_len + 1, size=n_out)
    begin, count, rs = _csr(lengths)
    idx = rng.integers(0, n_in, size=int(rs[-1])).astype(np.int32)
    if oob:
        bad = np.flatnonzero(rng.uniform(size=idx.size) < oob)
        idx[bad] = np.asarray([-1, n_in, n_in + 7], np.int32)[np.arange(bad.size) % 3]
    return idx, begin, count, rs


# ---- float64 reference ----------------------------------------------------------------------------------------------------------

def pairs(idx, begin, count, n_in, extra=0):
    """(row, j) of the in-range pairs in list order.  ``extra``: read that many entries past every row's count."""
    idx, begin = np.asarray(idx, np.int64), np.asarray(begin, np.int64)
    count = np.asarray(count, np.int64) + extra
    n_out = len(count)
    row = np.repeat(np.arange(n_out), count)
    within = np.arange(int(count.sum())) - np.repeat(np.cumsum(count) - count, count)
    j = idx[begin[row] + within]
    ok = (j >= 0) & (j < n_in)
    return row[ok], j[ok]


def _row_sums(vals, row, n_out):
    """Sum of vals [m, C] per row; ``row`` ascending."""
    out = np.zeros((n_out, vals.shape[1]))
    if len(row):
        first = np.flatnonzero(np.concatenate([[True], row[1:] != row[:-1]]))
        out[row[first]] = np.add.reduceat(vals, first, axis=0)
    return out


def _act(x, relu):
    x = np.asarray(x, np.float64)
    return np.maximum(x, 0.0) if relu else x


def aggregate(x, idx, begin, count, n_in, relu, absolute=False):
    row, j = pairs(idx, begin, count, n_in)
    f = _act(np.asarray(x)[:n_in], relu)
    if absolute:
        f = np.abs(f)
    n_out = len(count)
    return _row_sums(f[j], row, n_out), np.bincount(row, minlength=n_out).astype(np.float64)


def forward(x, W, b, idx, begin, count, n_in, relu, residual=None, absolute=False):
    """out [n_out, Cout] in float64 (``absolute``: the same sum over absolute terms) and c [n_out]."""
    S, c = aggregate(x, idx, begin, count, n_in, relu, absolute)
    W = np.asarray(W, np.float64)
    out = S @ (np.abs(W) if absolute else W)
    if b is not None:
        b = np.asarray(b, np.float64)
        out += c[:, None] * (np.abs(b) if absolute else b)[None, :]
    if residual is not None:
        r = np.asarray(residual, np.float64)
        out += np.abs(r) if absolute else r
    return out, c


def backward(x, W, G, idx, begin, count, n_in, relu, absolute=False):
    """(dx [len(x), Cin], dW, db, c' [len(x)]: the pairs referring to each input row)."""
    x = np.asarray(x, np.float64)
    W, G = np.asarray(W, np.float64), np.asarray(G, np.float64)
    if absolute:
        W, G = np.abs(W), np.abs(G)
    row, j = pairs(idx, begin, count, n_in)
    order = np.argsort(j, kind="stable")
    T = _row_sums(G[row[order]], j[order], len(x))
    dx = T @ W.T
    if relu and not absolute:
        dx = dx * (x > 0)
    S, c = aggregate(x, idx, begin, count, n_in, relu, absolute)
    return dx, S.T @ G, c @ G, np.bincount(j, minlength=len(x)).astype(np.float64)


# ---- bars -------------------------------------------------------------------------------------------------------------------------

def bars(case, gradients=True):
    """-> dict(out=(ref, bar, c), dx=(ref, bar), dW=(ref, bar), db=(ref, bar)) in float64; ``gradients`` False: out only.
    The sums of forward() and backward(), plain and over absolute terms, from one walk of the list."""
    x, W, b, res = case["x"], np.asarray(case["W"], np.float64), case["b"], case["residual"]
    n_in, n_out = case["n_in"], len(case["count"])
    cin, cout = W.shape
    row, j = pairs(case["idx"], case["begin"], case["count"], n_in)
    f = _act(np.asarray(x)[:n_in], case["relu"])
    S = _row_sums(f[j], row, n_out)
    Sa = S if case["relu"] else _row_sums(np.abs(f)[j], row, n_out)  # (relu: the terms are non-negative already)
    c = np.bincount(row, minlength=n_out).astype(np.float64)
    ref, A = S @ W, Sa @ np.abs(W)
    if b is not None:
        b = np.asarray(b, np.float64)
        ref += c[:, None] * b[None, :]
        A += c[:, None] * np.abs(b)[None, :]
    if res is not None:
        ref += np.asarray(res, np.float64)
        A += np.abs(np.asarray(res, np.float64))
    out = dict(out=(ref, (c[:, None] + cin + 4) * EPS * A, c))
    if gradients:
        G = np.asarray(case["G"], np.float64)
        order = np.argsort(j, kind="stable")
        T = _row_sums(G[row[order]], j[order], len(x))
        Ta = _row_sums(np.abs(G)[row[order]], j[order], len(x))
        dx, Ax = T @ W.T, Ta @ np.abs(W).T
        if case["relu"]:
            dx = dx * (np.asarray(x) > 0)
        cj = np.bincount(j, minlength=len(x)).astype(np.float64)
        n_nz = int(np.any(G != 0, axis=1).sum())
        lmax = int(c.max()) if c.size else 0
        out["dx"] = (dx, (cj[:, None] + cout + 4) * EPS * Ax)
        out["dW"] = (S.T @ G, (lmax + n_nz + 4) * EPS * (Sa.T @ np.abs(G)))
        out["db"] = (c @ G, (n_nz + 4) * EPS * (c @ np.abs(G)))
    return out


WORST = {}  # group -> worst err / bar, printed by the GPU file's test_report_worst_ratio


def check(group, what, got, ref, bar):
    got = np.asarray(got)
    assert got.dtype == F and got.shape == ref.shape, (what, got.dtype, got.shape, ref.shape)
    assert np.all(np.isfinite(got)), f"{what}: not finite"
    err = np.abs(got.astype(np.float64) - ref)
    pos = bar > 0
    r = float((err[pos] / bar[pos]).max()) if pos.any() else 0.0
    WORST[group] = max(WORST.get(group, 0.0), r)
    bad = err > bar
    assert not bad.any(), f"{what}: {int(bad.sum())} elements over the bar, worst err/bar {r:.3g} at {np.argwhere(bad)[0].tolist()}"


def check_exact(case, out, dx=None):
    """The exact-result rules: a row without in-range pairs is the residual or 0; dx is 0 where x <= 0 under relu and in the
    rows past n_in."""
    _, c = aggregate(case["x"], case["idx"], case["begin"], case["count"], case["n_in"], case["relu"])
    empty = c == 0
    want = np.zeros_like(out) if case["residual"] is None else case["residual"]
    assert np.array_equal(np.asarray(out)[empty], want[empty]), "a row without in-range pairs is not exactly the residual / 0"
    if dx is not None:
        dx = np.asarray(dx)
        assert dx.shape == case["x"].shape
        assert np.all(dx[case["n_in"]:] == 0), "a row of dx past n_in is not 0"
        if case["relu"]:
            assert np.all(dx[:case["n_in"]][case["x"][:case["n_in"]] <= 0] == 0), "dx is not 0 where x <= 0"


# ---- cases ------------------------------------------------------------------------------------------------------------------------

WIDTHS = ((1, 1), (2, 17), (3, 16), (5, 15), (61, 31), (63, 65), (64, 64), (65, 33), (66, 127), (127, 48), (128, 1))
TILE_N_OUT = (1, 15, 16, 17, 31, 33, 129)
TILE_WIDTHS = ((7, 64), (128, 128))
DX_WIDTHS = ((7, 64), (65, 33), (128, 128))
SLAB_N_OUT = (1, 3, 4, 5, 127, 128, 129, 131, 132, 133, 257)
SLAB_WIDTHS = ((7, 64), (63, 17), (64, 16), (127, 3), (128, 128))
ONE_HOT_ROWS = (0, ROW_640, 15, ROW_130, 19)
SLAB_CAP_N_OUT = 2048 * 128 + 5
PERSISTENT_WIDTHS = ((8, 16), (128, 128))

SLAB_ROWS, MAX_SLABS = 128, 2048  # kNdSlabRows, kNdMaxSlabs


def bwd_plan(n_out):
    """nd_bwd_plan restated: -> (rows_per_slab, nslabs)."""
    S = max(1, min(-(-n_out // SLAB_ROWS), MAX_SLABS))
    rps = (-(-n_out // S) + 3) & ~3
    return rps, max(1, -(-n_out // max(rps, 1)))


def workspace_bytes(n_out, cin, cout):
    return 4 * bwd_plan(n_out)[1] * (cin + 1) * cout


def gather_name(cin):
    return "nd_gather_mfma<2>" if cin > 64 else "nd_gather_mfma<1>"


def launch_plan(cin, cout, n_cu):
    """nd_launch restated: -> (lds bytes, workgroups per CU, resident waves)."""
    cin_p, cout_p = (cin + 3) & ~3, (cout + 15) & ~15
    lds = 4 * (cin_p * (cout_p + 16) + 128 * (cin_p + 2) + 128)
    per_cu = max(1, min(4, 163840 // lds))
    return lds, per_cu, 8 * n_cu * per_cu


def persistent_n_out(cin, cout, n_cu):
    return 16 * (2 * launch_plan(cin, cout, n_cu)[2] + 3) + 5


def _operands(rng, x_rows, n_out, cin, cout, bias, residual, zeros=True):
    x = rng.normal(size=(x_rows, cin)).astype(F)
    if zeros and x.size >= 4:  # exact zeros of both signs: relu'(0) = 0
        flat = x.reshape(-1)
        flat[rng.permutation(flat.size)[:max(2, flat.size // 16)]] = F(0.0)
        flat[rng.permutation(flat.size)[:max(2, flat.size // 16)]] = F(-0.0)
    W = (rng.normal(size=(cin, cout)) / np.sqrt(cin)).astype(F)
    b = rng.normal(size=cout).astype(F) if bias else None
    r = rng.normal(size=(n_out, cout)).astype(F) if residual else None
    G = rng.normal(size=(n_out, cout)).astype(F)
    return x, W, b, r, G


def _case(name, group, lst, n_in, x, W, b, r, G, relu, **more):
    idx, begin, count, rs = lst
    c = dict(name=name, group=group, idx=np.asarray(idx), begin=np.asarray(begin), count=np.asarray(count), row_splits=rs,
             n_in=n_in, x=x, W=W, b=b, residual=r, G=G, relu=bool(relu), **more)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def _seed(*key):
    """One seed per case: the group's number (1 widths ... 7 persistent), then the case's own numbers."""
    return int(np.random.SeedSequence([int(k) for k in key]).generate_state(1)[0])


def case_names(group):
    if group == "widths":
        return [f"{ci}x{co}_{'relu' if relu else 'lin'}" for ci, co in WIDTHS for relu in (True, False)]
    if group == "tiles":
        return [f"n{n}_{ci}x{co}" for n in TILE_N_OUT for ci, co in TILE_WIDTHS]
    if group == "dx_rows":
        return [f"{ci}x{co}_{'relu' if relu else 'lin'}_{kind}" for ci, co in DX_WIDTHS for relu in (True, False)
                for kind in ("inrange", "oob")]
    if group == "slabs":
        return [f"n{n}_{ci}x{co}" for n in SLAB_N_OUT for ci, co in SLAB_WIDTHS]
    if group == "one_hot_G":
        return [f"row{r}" for r in ONE_HOT_ROWS]
    if group == "slab_cap":
        return ["cap"]
    raise KeyError(group)


SMALL_GROUPS = ("widths", "tiles", "dx_rows", "slabs", "one_hot_G")


def _parse_widths(tok):
    a, b = tok.split("x")
    return int(a), int(b)


@functools.lru_cache(maxsize=256)
def case(group, name):
    """The case's operands as read-only numpy arrays: x [x_rows, Cin], W, b (or None), residual (or None), G, the list (idx,
    begin, count, row_splits -- None for padded lists), n_in, relu."""
    tok = name.split("_")
    if group == "widths":
        cin, cout = _parse_widths(tok[0])
        relu = tok[1] == "relu"
        w = WIDTHS.index((cin, cout))
        rng = np.random.default_rng(_seed(1, cin, cout, relu))
        lst = edge_rows(True)
        x, W, b, r, G = _operands(rng, EDGE_X_ROWS, len(EDGE_LENGTHS), cin, cout, bias=w % 3 != 0, residual=w % 2 == 0)
        pidx, pbegin, pcount = edge_rows_padded()
        return _case(name, group, lst, EDGE_N_IN, x, W, b, r, G, relu, padded=(pidx, pbegin, pcount))
    if group == "tiles":
        n_out = int(tok[0][1:])
        cin, cout = _parse_widths(tok[1])
        rng = np.random.default_rng(_seed(2, n_out, cin, cout))
        lst = random_rows(rng, n_out, 40, 3)
        x, W, b, r, G = _operands(rng, 44, n_out, cin, cout, bias=True, residual=TILE_N_OUT.index(n_out) % 2 == 0)
        return _case(name, group, lst, 40, x, W, b, r, G, True)
    if group == "dx_rows":
        cin, cout = _parse_widths(tok[0])
        relu = tok[1] == "relu"
        eidx, _, _, ers = edge_rows(tok[2] == "oob")
        t_idx, t_rs = transpose(eidx, ers, EDGE_N_IN)
        n_in, n_out = len(EDGE_LENGTHS), EDGE_N_IN  # the roles swap: the 20 controlled rows are the layer's input rows
        rng = np.random.default_rng(_seed(3, cin, cout, relu, tok[2] == "oob"))
        x, W, b, r, G = _operands(rng, n_in + 4, n_out, cin, cout, bias=True, residual=False, zeros=False)
        if relu:  # a few exact zeros, most of every row kept: a masked element says nothing about the row's sum
            x[1, 0], x[ROW_640, cin - 1] = F(0.0), F(-0.0)
        lst = (t_idx, t_rs[:-1].copy(), np.diff(t_rs).astype(np.int32), t_rs)
        return _case(name, group, lst, n_in, x, W, b, r, G, relu)
    if group == "slabs":
        n_out = int(tok[0][1:])
        cin, cout = _parse_widths(tok[1])
        rng = np.random.default_rng(_seed(4, n_out, cin, cout))
        lst = random_rows(rng, n_out, 50, 5)
        x, W, b, r, G = _operands(rng, 50, n_out, cin, cout, bias=True, residual=False)
        return _case(name, group, lst, 50, x, W, b, r, G, SLAB_N_OUT.index(n_out) % 2 == 0)
    if group == "one_hot_G":
        hot = int(tok[0][3:])
        cin, cout = 65, 33
        rng = np.random.default_rng(_seed(5, hot))
        x, W, b, r, G = _operands(rng, EDGE_X_ROWS, len(EDGE_LENGTHS), cin, cout, bias=True, residual=False)
        keep = G[hot].copy()
        G[:] = 0
        G[hot] = keep
        return _case(name, group, edge_rows(True), EDGE_N_IN, x, W, b, r, G, True, hot=hot)
    if group == "slab_cap":
        n_out, cin, cout, n_in = SLAB_CAP_N_OUT, 5, 3, 1000
        assert bwd_plan(n_out) == (132, 1986)
        rng = np.random.default_rng(_seed(6))
        lst = random_rows(rng, n_out, n_in, 2)
        x, W, b, r, G = _operands(rng, n_in, n_out, cin, cout, bias=True, residual=False)
        hot = np.unique(np.concatenate([[0, 131, 132, n_out - 1], rng.integers(0, n_out, size=20)]))
        keep = G[hot].copy()
        G[:] = 0
        G[hot] = keep
        return _case(name, group, lst, n_in, x, W, b, r, G, True, hot=hot)
    raise KeyError(group)


def persistent_case(cin, cout, n_cu):
    """n_out = 16 (2 resident + 3) + 5 rows of 0 to 3 pairs -- every 97th has 65, every 1009th 130 -- over n_in = n_out."""
    n_out = persistent_n_out(cin, cout, n_cu)
    rng = np.random.default_rng(_seed(7, cin, cout, n_cu))
    lengths = rng.integers(0, 4, size=n_out)
    lengths[::97] = 65
    lengths[::1009] = 130
    begin, count, rs = _csr(lengths)
    idx = rng.integers(0, n_out, size=int(rs[-1])).astype(np.int32)
    bad = np.flatnonzero(rng.uniform(size=idx.size) < 0.05)
    idx[bad] = np.asarray([-1, n_out, n_out + 7], np.int32)[np.arange(bad.size) % 3]
    x, W, b, r, G = _operands(rng, n_out, n_out, cin, cout, bias=True, residual=cin == cout)
    return _case(f"{cin}x{cout}", "persistent", (idx, begin, count, rs), n_out, x, W, b, r, G, True)


# ---- float32 emulation in the kernels' order ------------------------------------------------------------------------------------------

def _fma(a, b, c):
    """float32 fma(a, b, c): the product of two float32 is exact in float64; one rounding of the float64 sum apart, exact."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)


def emulate_gather(x, W, b, idx, begin, count, n_in, relu, residual=None, mask=None, mutate=None):
    """nd_gather_mfma: -> (out, S, c) in float32.  Rows are summed in pair order; the contraction is an fma chain over the
    channels in ascending order (the matrix instruction's four products per step taken in order).  ``mutate``: a seeded fault."""
    x = np.asarray(x, F)
    W = np.asarray(W, F)
    idx, begin, count = np.asarray(idx, np.int64), np.asarray(begin, np.int64), np.asarray(count, np.int64)
    n_out, cin, cout = len(count), W.shape[0], W.shape[1]
    f = np.maximum(x, F(0)) if relu else x
    S = np.zeros((n_out, cin), F)
    c = np.zeros(n_out, F)
    for r in range(n_out):
        n = int(count[r])
        if mutate == "stop_at_64":
            n = min(n, 64)
        if mutate == "drop_last_long" and n > 64:
            n -= 1
        if mutate == "read_past_count":
            n += 1
        acc = np.zeros(cin, F)
        if mutate == "carry_S" and r >= 16:
            acc = S[r - 16].copy()
        cnt = 0
        for j in idx[begin[r]:begin[r] + n]:
            if 0 <= j < n_in:
                acc = (acc + f[j]).astype(F)
                cnt += 1
            elif mutate == "bias_oob":
                cnt += 1
        S[r], c[r] = acc, cnt
    d = np.zeros((n_out, cout), F)
    for k in range(cin):
        d = _fma(S[:, k:k + 1], W[k:k + 1, :], d)
    if b is not None:
        d = _fma(c[:, None], np.asarray(b, F)[None, :], d)
    if residual is not None:
        d = (d + np.asarray(residual, F)).astype(F)
    if mask is not None:
        d = np.where(np.asarray(mask) > 0, d, F(0)).astype(F)
    return d, S, c


def emulate_weight(S, c, G, mutate=None):
    """nd_bwd_weight + nd_bwd_weight_reduce: -> (dW, db).  Per slab an fma chain over its rows in order, then the slabs in
    order."""
    S, c, G = np.asarray(S, F), np.asarray(c, F), np.asarray(G, F)
    n_out, cin = S.shape
    cout = G.shape[1]
    SC = np.concatenate([S, c[:, None]], axis=1)
    if mutate == "drop_count_channel" and cin % 64 == 0:
        SC[:, cin] = 0
    n_rows = n_out - n_out % 4 if mutate == "drop_tail_rows" else n_out
    rps, nslabs = bwd_plan(n_out)
    total = np.zeros((cin + 1, cout), F)
    for s in range(nslabs):
        part = np.zeros((cin + 1, cout), F)
        for r in range(s * rps, min(n_rows, (s + 1) * rps)):
            part = _fma(SC[r][:, None], G[r][None, :], part)
        total = (total + part).astype(F)
    return total[:cin], total[cin]


def emulate(case, mutate=None, padded=False):
    """The whole layer and its gradients as the kernels order them: -> dict(out, dx, dW, db) in float32."""
    if padded:
        idx, begin, count = case["padded"]
    else:
        idx, begin, count = case["idx"], case["begin"], case["count"]
    n_in, relu = case["n_in"], case["relu"]
    fwd_mut = mutate if mutate in ("stop_at_64", "drop_last_long", "read_past_count", "carry_S", "bias_oob") else None
    out, S, c = emulate_gather(case["x"], case["W"], case["b"], idx, begin, count, n_in, relu, case["residual"], mutate=fwd_mut)
    # the inverted list: what dmcf_invert_neighbors_list gives (a stable sort of the in-range pairs by index)
    row, j = pairs(idx, begin, count, n_in)
    order = np.argsort(j, kind="stable")
    inv_idx = row[order]
    inv_rs = np.concatenate([[0], np.cumsum(np.bincount(j, minlength=n_in))]).astype(np.int64)
    inv_count = np.diff(inv_rs)
    dx = np.zeros(case["x"].shape, F)
    dxi, _, _ = emulate_gather(case["G"], case["W"].T, None, inv_idx, inv_rs[:-1], inv_count, len(case["G"]), False,
                               mask=case["x"][:n_in] if relu else None, mutate=fwd_mut if fwd_mut != "read_past_count" else None)
    dx[:n_in] = dxi
    dW, db = emulate_weight(S, c, case["G"], mutate=mutate)
    return dict(out=out, dx=dx, dW=dW, db=db)


MUTATIONS = ("drop_last_long", "stop_at_64", "bias_oob", "read_past_count", "carry_S", "drop_count_channel", "drop_tail_rows")


def check_case(case, got, group=None):
    """Every bar and exact rule of a case on host arrays ``got`` = dict(out[, dx, dW, db])."""
    B = bars(case, gradients=any(got.get(k) is not None for k in ("dx", "dW", "db")))
    g = group or case["group"]
    for what in ("out", "dx", "dW", "db"):
        if what in got and got[what] is not None:
            check(g, f"{case['name']}: {what}", got[what], B[what][0], B[what][1])
    check_exact(case, got["out"], got.get("dx"))
