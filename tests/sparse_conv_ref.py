"""SparseConv / SparseConvTranspose in float64 numpy: brute-force max-norm pair sets, both forwards and all gradients, each with
the sum of the absolute values of its terms (A), and the deterministic cases tests/test_sparse_conv_ref_cpu.py and
tests/test_gpu_sparse_conv.py share.

    SparseConv           out_i = s_i sum_{j in N(out_i - offset v)} imp_j W[cell(inp_j - out_i)]^T f_j + bias
    SparseConvTranspose  out_i = oimp_i sum_{j : i in N_T(j)} n_j W[cell(out_i - inp_j)]^T f_j + bias,  N_T(j) = N(inp_j - offset v)
                         over the OUTPUT points
    N(q) = { p : max_a |p_a - q_a| <= R },  R = kernel_size[-1] * v * 0.51 (float32),  E = v * kernel_size[-1]
    cell(d): per axis t = d_a / E * k_a + (k_a - 1) / 2 + offset_a, the cell is clamp(round(t), 0, k_a - 1)

The bar of the GPU tests is the project's element-wise one (tests/cconv_forward_ref.py) without its geometric term -- the
weights here are exactly 1:   |got - ref| <= kbar * 2^-24 * A,   kbar = max(256, longest row + K * Cin + 64).

The cases keep every pair at least 0.15 voxel from the search threshold and every filter coordinate at least 0.2 from a
half-integer (``margins`` measures both; the CPU test asserts them), so the pair sets and the cells are the same in float32 and
float64 and no row is excused.
"""
import functools

import numpy as np

EPS = 2.0 ** -24
K_BAR = 256
PER_TERM = 64
VOXEL = 0.37


def default_offset(kernel_size):
    return np.zeros(3) if kernel_size[0] % 2 else np.full(3, -0.5)


def search_radius(kernel_size, voxel):
    return np.float32(np.float32(np.float32(kernel_size[-1]) * np.float32(voxel)) * np.float32(0.51))


def extent(kernel_size, voxel):
    return np.float32(voxel) * np.float32(kernel_size[-1])


def pair_sets(points, queries, radius, ignore_query_point=False):
    """Brute force: CSR (index int32 ascending in a row, row_splits int64) of { p : max_a |p_a - q_a| <= radius } in float32
    differences, inclusive.  Every query is tested against every point whose x lies within the x range of its block of 256
    queries (taken in x order) widened by the radius and a slack far above rounding: O(n m) tests short of a constant."""
    P = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    Q = np.asarray(queries, dtype=np.float32).reshape(-1, 3)
    r = np.float32(radius)
    porder = np.argsort(P[:, 0], kind="stable")
    px = P[porder, 0].astype(np.float64)
    qorder = np.argsort(Q[:, 0], kind="stable")
    slack = 1e-3 * float(r) + 1e-5 * (float(np.abs(P).max()) if P.size else 0.0)
    qs, ps = [], []
    for b in range(0, Q.shape[0], 256):
        qi = qorder[b:b + 256]
        q = Q[qi]
        lo = np.searchsorted(px, float(q[:, 0].min()) - float(r) - slack, side="left")
        hi = np.searchsorted(px, float(q[:, 0].max()) + float(r) + slack, side="right")
        cand = porder[lo:hi]
        C = P[cand]
        hit = np.abs(C[None, :, 0] - q[:, None, 0]) <= r
        hit &= np.abs(C[None, :, 1] - q[:, None, 1]) <= r
        hit &= np.abs(C[None, :, 2] - q[:, None, 2]) <= r
        if ignore_query_point:
            hit &= ~((C[None, :, 0] == q[:, None, 0]) & (C[None, :, 1] == q[:, None, 1]) & (C[None, :, 2] == q[:, None, 2]))
        a, c = np.nonzero(hit)
        qs.append(qi[a])
        ps.append(cand[c])
    qa = np.concatenate(qs) if qs else np.zeros(0, dtype=np.int64)
    pa = np.concatenate(ps) if ps else np.zeros(0, dtype=np.int64)
    o = np.lexsort((pa, qa))
    counts = np.bincount(qa, minlength=Q.shape[0])
    return pa[o].astype(np.int32), np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def filter_coords(d, kernel_size, voxel, offset):
    """[P, 3] (x, y, z) float64 filter coordinates of the relative positions d [P, 3]."""
    k = np.asarray(kernel_size[::-1], dtype=np.float64)  # (kx, ky, kz)
    return np.asarray(d, dtype=np.float64) / float(extent(kernel_size, voxel)) * k + (k - 1.0) / 2.0 + np.asarray(offset, dtype=np.float64)


def cells(d, kernel_size, voxel, offset):
    """Flat filter cell (z, y, x order) of each relative position."""
    k = np.asarray(kernel_size[::-1], dtype=np.int64)
    t = filter_coords(d, kernel_size, voxel, offset)
    c = np.clip(np.floor(t + 0.5).astype(np.int64), 0, k - 1)
    return (c[:, 2] * k[1] + c[:, 1]) * k[0] + c[:, 0]


class Pairs:
    """The terms of one operator: output row i, input row j, filter cell and coefficient of every pair."""

    def __init__(self, i, j, cell, coef, n_out, n_inp):
        self.i, self.j, self.cell, self.coef, self.n_out, self.n_inp = i, j, cell, coef, n_out, n_inp

    def longest_row(self):
        return int(np.bincount(self.i, minlength=1).max()) if self.i.size else 0

    def longest_col(self):
        return int(np.bincount(self.j, minlength=1).max()) if self.j.size else 0


def gather(pr, W, F):
    """out [n_out, Cout] = sum_p coef_p W[cell_p]^T F[j_p]."""
    K = int(np.prod(W.shape[:3]))
    Wc = W.reshape(K, W.shape[3], W.shape[4])
    out = np.zeros((pr.n_out, W.shape[4]))
    for c in np.unique(pr.cell):
        m = pr.cell == c
        np.add.at(out, pr.i[m], (F[pr.j[m]] * pr.coef[m, None]) @ Wc[c])
    return out


def gather_grads(pr, W, F, G):
    """(dW, dF, dcoef-per-pair) of sum(gather * G)."""
    K = int(np.prod(W.shape[:3]))
    Wc = W.reshape(K, W.shape[3], W.shape[4])
    dW = np.zeros_like(Wc)
    dF = np.zeros_like(F)
    dcoef = np.zeros(pr.i.shape[0])
    for c in np.unique(pr.cell):
        m = pr.cell == c
        Fi, Gi, co = F[pr.j[m]], G[pr.i[m]], pr.coef[m]
        dW[c] = (Fi * co[:, None]).T @ Gi
        np.add.at(dF, pr.j[m], (Gi @ Wc[c].T) * co[:, None])
        dcoef[m] = ((Fi @ Wc[c]) * Gi).sum(axis=1)
    return dW.reshape(W.shape), dF, dcoef


class Case:
    """One problem: point sets, kernel, features and options; the reference results are cached on the object."""

    def __init__(self, name, kernel_size, cin, cout, inp, out, seed, importance=False, normalize=False, bias=False, voxel=VOXEL,
                 offset=None):
        rng = np.random.default_rng(seed)
        self.name, self.kernel_size, self.cin, self.cout, self.voxel = name, list(kernel_size), cin, cout, voxel
        self.inp = np.ascontiguousarray(inp, dtype=np.float32)
        self.out = np.ascontiguousarray(out, dtype=np.float32)
        self.offset = default_offset(kernel_size) if offset is None else np.asarray(offset, dtype=np.float64)
        self.normalize = normalize
        self.W = rng.uniform(-1, 1, size=(*kernel_size, cin, cout)).astype(np.float32)
        self.F = rng.normal(size=(self.inp.shape[0], cin)).astype(np.float32)
        self.G = rng.normal(size=(self.out.shape[0], cout)).astype(np.float32)
        self.bias = rng.normal(size=cout).astype(np.float32) if bias else None
        self.inp_importance = rng.uniform(0.5, 1.5, size=self.inp.shape[0]).astype(np.float32) if importance else None
        self.out_importance = rng.uniform(0.5, 1.5, size=self.out.shape[0]).astype(np.float32) if importance else None
        self.K = int(np.prod(kernel_size))

    @property
    def radius(self):
        return search_radius(self.kernel_size, self.voxel)

    def shift(self):
        """offset * voxel in float32, as the layers subtract it from the queries."""
        return (self.offset.astype(np.float32) * np.float32(self.voxel)).astype(np.float32)

    @functools.cached_property
    def conv_list(self):
        """SparseConv's list: for every output point the inputs in N(out - offset v)."""
        return pair_sets(self.inp, self.out - self.shift(), self.radius)

    @functools.cached_property
    def transpose_list(self):
        """SparseConvTranspose's list (nns_inp): for every INPUT point the outputs in N(inp - offset v)."""
        return pair_sets(self.out, self.inp - self.shift(), self.radius)

    @functools.cached_property
    def conv_pairs(self):
        idx, rs = self.conv_list
        cnt = np.diff(rs)
        i = np.repeat(np.arange(self.out.shape[0]), cnt)
        j = idx.astype(np.int64)
        d = self.inp[j].astype(np.float64) - self.out[i].astype(np.float64)
        coef = np.ones(i.shape[0])
        if self.inp_importance is not None:
            coef = coef * self.inp_importance[j].astype(np.float64)
        if self.normalize:
            coef = coef / cnt[i]
        return Pairs(i, j, cells(d, self.kernel_size, self.voxel, self.offset), coef, self.out.shape[0], self.inp.shape[0])

    @functools.cached_property
    def transpose_pairs(self):
        idx, rs = self.transpose_list
        cnt = np.diff(rs)
        j = np.repeat(np.arange(self.inp.shape[0]), cnt)
        i = idx.astype(np.int64)
        d = self.out[i].astype(np.float64) - self.inp[j].astype(np.float64)
        coef = np.ones(i.shape[0])
        if self.out_importance is not None:
            coef = coef * self.out_importance[i].astype(np.float64)
        if self.normalize:
            coef = coef / cnt[j]
        return Pairs(i, j, cells(d, self.kernel_size, self.voxel, self.offset), coef, self.out.shape[0], self.inp.shape[0])

    def pairs(self, transpose):
        return self.transpose_pairs if transpose else self.conv_pairs

    @functools.lru_cache(maxsize=None)
    def forward(self, transpose=False):
        """(out, A) float64 [n_out, Cout], bias included."""
        pr = self.pairs(transpose)
        W, F = self.W.astype(np.float64), self.F.astype(np.float64)
        out = gather(pr, W, F)
        absp = Pairs(pr.i, pr.j, pr.cell, np.abs(pr.coef), pr.n_out, pr.n_inp)
        A = gather(absp, np.abs(W), np.abs(F))
        if self.bias is not None:
            out = out + self.bias.astype(np.float64)
            A = A + np.abs(self.bias.astype(np.float64))
        return out, A

    @functools.lru_cache(maxsize=None)
    def grads(self, transpose=False):
        """((dW, A), (dF, A), (dbias, A), (dimportance, A)) of sum(out * G): the importance is inp_importance of SparseConv, out_importance
        of the transpose (None without importance)."""
        pr = self.pairs(transpose)
        W, F, G = self.W.astype(np.float64), self.F.astype(np.float64), self.G.astype(np.float64)
        dW, dF, dcoef = gather_grads(pr, W, F, G)
        absp = Pairs(pr.i, pr.j, pr.cell, np.abs(pr.coef), pr.n_out, pr.n_inp)
        aW, aF, acoef = gather_grads(absp, np.abs(W), np.abs(F), np.abs(G))
        imp = self.out_importance if transpose else self.inp_importance
        dimp = None
        if imp is not None:
            who = pr.i if transpose else pr.j
            n = pr.n_out if transpose else pr.n_inp
            scale = pr.coef / imp[who].astype(np.float64)  # d coef / d importance
            dimp = (np.bincount(who, weights=dcoef * scale, minlength=n), np.bincount(who, weights=acoef * np.abs(scale), minlength=n))
        return (dW, aW), (dF, aF), (G.sum(axis=0), np.abs(G).sum(axis=0)), dimp

    def kbar(self, transpose=False, chain_channels=None, columns=False):
        """max(256, longest row + K * Cin + 64); ``columns``: the longest row of the inverted list (the feature gradient)."""
        pr = self.pairs(transpose)
        longest = pr.longest_col() if columns else pr.longest_row()
        return max(K_BAR, longest + self.K * (self.cin if chain_channels is None else chain_channels) + PER_TERM)

    def margins(self):
        """(smallest distance of a pair or non-pair from the search threshold, in voxels, capped at 1; smallest distance of a
        filter coordinate from a half-integer; does the clamp engage) over both operators.  The threshold distance is taken
        over every point within one voxel of the box along x (the others are further than that from the threshold), queries in
        x order, 256 at a time."""
        thr, half, clamp = 1.0, np.inf, False
        k = np.asarray(self.kernel_size[::-1])
        R = float(self.radius)
        for pts, qs, tr in ((self.inp, self.out, False), (self.out, self.inp, True)):
            q = (qs - self.shift()).astype(np.float64)
            P = pts.astype(np.float64)
            porder = np.argsort(P[:, 0], kind="stable")
            px = P[porder, 0]
            qorder = np.argsort(q[:, 0], kind="stable")
            for b in range(0, q.shape[0], 256):
                qb = q[qorder[b:b + 256]]
                lo = np.searchsorted(px, qb[:, 0].min() - R - self.voxel, side="left")
                hi = np.searchsorted(px, qb[:, 0].max() + R + self.voxel, side="right")
                C = P[porder[lo:hi]]
                if C.size and qb.size:
                    d = np.maximum(np.maximum(np.abs(C[None, :, 0] - qb[:, None, 0]), np.abs(C[None, :, 1] - qb[:, None, 1])),
                                   np.abs(C[None, :, 2] - qb[:, None, 2]))
                    thr = min(thr, float(np.abs(d - R).min()) / self.voxel)
            pr = self.pairs(tr)
            if pr.i.size:
                d = (self.out[pr.i].astype(np.float64) - self.inp[pr.j]) * (1.0 if tr else -1.0)
                t = filter_coords(d, self.kernel_size, self.voxel, self.offset)
                half = min(half, float(np.abs(t - np.floor(t) - 0.5).min()))
                r = np.floor(t + 0.5)
                clamp |= bool(((r < 0) | (r > k - 1)).any())
        return thr, half, clamp


def lattice_points(rng, dims, voxel=VOXEL, occupancy=0.6, jitter=0.15, origin=(0, 0, 0)):
    """(cell + 0.5 + u) * voxel, |u| <= jitter per axis, for the occupied cells of a dims = (nx, ny, nz) box."""
    nx, ny, nz = dims
    zz, yy, xx = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    cell = np.stack([xx.ravel(), yy.ravel(), zz.ravel()], axis=1) + np.asarray(origin)
    cell = cell[rng.random(cell.shape[0]) < occupancy]
    u = rng.uniform(-jitter, jitter, size=cell.shape) if jitter > 0 else np.zeros(cell.shape)
    return ((cell + 0.5 + u) * voxel).astype(np.float32)


BOX = (7, 6, 5)


def _case(name, kernel_size, cin, cout, seed, dims=BOX, jitter=0.15, twins=False, lonely=False, **kw):
    rng = np.random.default_rng(1000 + seed)
    inp = lattice_points(rng, dims, jitter=jitter)
    out = lattice_points(rng, dims, jitter=jitter)
    if twins:  # two inputs in one voxel: a second point in the cells of the first five inputs, with its own jitter
        base = np.floor(inp[:5] / np.float32(VOXEL))
        inp = np.concatenate([inp, ((base + 0.5 + rng.uniform(-0.15, 0.15, size=base.shape)) * VOXEL).astype(np.float32)])
    if lonely:  # output rows without neighbours (and, for the transpose, inputs that reach no output)
        out = np.concatenate([out[:3] + np.float32(100 * VOXEL), out, out[-2:] - np.float32(100 * VOXEL)])
        inp = np.concatenate([inp, inp[:2] + np.float32(300 * VOXEL)])
    return Case(name, kernel_size, cin, cout, inp, out, seed, **kw)


@functools.lru_cache(maxsize=None)
def small_cases():
    return (
        _case("k2_c1", [2, 2, 2], 1, 1, 1),
        _case("k3_c5x7_imp_norm_bias", [3, 3, 3], 5, 7, 2, importance=True, normalize=True, bias=True, twins=True),
        _case("k4_c8x16_bias", [4, 4, 4], 8, 16, 3, bias=True, lonely=True),
        _case("k3_c32x32", [3, 3, 3], 32, 32, 4, twins=True, lonely=True),
        _case("k2_c5x7_norm", [2, 2, 2], 5, 7, 5, normalize=True, lonely=True),
        _case("k4_c32x32_imp", [4, 4, 4], 32, 32, 6, importance=True),
        _case("k133_planar_c8x16", [1, 3, 3], 8, 16, 7, dims=(7, 6, 1), bias=True, normalize=True),
        _case("k3_zero_jitter_c8x16", [3, 3, 3], 8, 16, 8, jitter=0.0, importance=True, bias=True),
        # an explicit offset that differs per axis, (x, y, z) = (-0.5, -0.5, 0), where the default of [1, 2, 2] is zero (its first
        # size is odd): only even axes can take -0.5 without putting the lattice's coordinates on half-integers, and the search
        # radius follows kernel_size[-1] alone, so the odd axis is the planar one
        _case("k122_planar_offset_xy_c5x7", [1, 2, 2], 5, 7, 10, dims=(7, 6, 1), bias=True, importance=True, offset=(-0.5, -0.5, 0.0)),
    )


@functools.lru_cache(maxsize=None)
def big_case():
    """About 20 000 points a side: the filter gradient spans several slabs of pairs."""
    return _case("k3_c8x16_20k", [3, 3, 3], 8, 16, 9, dims=(32, 32, 32), normalize=True, bias=True)


def all_cases():
    return small_cases() + (big_case(),)


def check(got, ref, A, kbar, what):
    """Element-wise bar; returns the worst err / bar."""
    got, ref, A = np.asarray(got, dtype=np.float64), np.asarray(ref), np.asarray(A)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bar = kbar * EPS * A
    err = np.abs(got - ref)
    worst = float((err / np.maximum(bar, 1e-300)).max()) if err.size else 0.0
    bad = err > bar
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements above the bar, worst err/bar {worst:.3g} (kbar {kbar})"
    return worst
