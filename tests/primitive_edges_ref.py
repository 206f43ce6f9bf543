"""The row, list and scan primitives at their grid caps and tile edges: the case lists and the plain numpy / float64 references
shared by tests/test_primitive_edges_cpu.py (every condition a case must meet, without a GPU) and
tests/test_gpu_primitive_edges.py (the HIP kernels against these references).  Every input is valid under the operation's
documented contract.

A  dmcf_invert_neighbors_list (cconv_bwd.hip) against np.argsort(kind="stable"): list lengths either side of the two size
   thresholds of rocPRIM's radix_sort_pairs (SORT_BLOCK_ITEMS, SORT_MERGE_LIMIT) and of the 4096-block cap of invert_init /
   invert_gather (GRID_FOR_CAP), key widths either side of a power of two (the sentinel key n_inp then needs one bit more
   than the largest valid key), invalid entries, a buffer longer than its rows, the padded form, one key, descending keys.
B  reduce_subarrays_sum / neighbor_counts (misc.hip): 16 lanes per row, 16 rows per block; float64 sums and the bar
   (ceil(len / 16) + 5) * 2^-24 * sum |v| per row -- a lane adds at most ceil(len / 16) terms in sequence, four butterfly steps
   follow, one unit is margin.  |v| in [0.5, 1]: min |v| > 2 * bar in every row, so one element dropped or counted twice fails.
C  scan_counts_to_row_splits (misc.hip: tiles of 2048 elements, 256 block sums per round) through the public search: queries
   whose neighbour count is known by construction.
D  dmcf_dense_forward (misc.hip, dense_rows): the grid is capped at 2048 blocks x 4 waves x 16 rows = DENSE_ROWS_PER_PASS rows.
E  farthest point sampling (fps.hip: 1024 threads, points 0 .. 8191 in registers, the rest in the workspace) with exact ties
   that straddle the two stores, and gather_point at several channel counts.
F  dmcf_cconv_backward past the cap of grid_for (GRID_FOR_CAP elements): the smallest accepted shape whose full filter
   gradient K * Cin * Cout exceeds it.
G  the forward filter packers.  Each runs a grid-stride loop over its packed elements on a capped grid; the table says which
   caps a shape the form accepts can exceed (``packer_table``; the arithmetic per packer):

   packer              cap (elements)        largest count an accepted shape reaches         smallest accepted shape above
   pack_filter (lds)   2048 * 256 = 524,288  unbounded: nchunks = ceil(Cin / 8) has no limit 4x4x4, see LDS_OVER_CAP
   pack_filter (mfma)  524,288               unbounded in Cin (K <= 64, Cout <= 64)          4x4x4, Cin 129, Cout 49: 589,824
   pack_filter (blk)   524,288               unbounded in Cin (4x4x4, Cin % 4 = 0)           Cin 132, Cout 49: 589,824
   pack_filter_cls     524,288               unbounded in Cin (4x4x4, Cin % 4 = 0)           Cin 116, Cout 49: 524,304
   pack_direct         1024 * 256 = 262,144  8,959 float4 entries -- UNREACHABLE             --
   lat_build_filters   4096 * 256 = 1,048,576  unbounded: 256 * n_offsets, set by radius / voxel   radius 10.2 voxels, see LAT_OVER_CAP

   pack_filter: packed = nchunks * nblocks * NT * 256 floats.  mfma: nblocks = 16 * ceil(K / 16) <= 64, NT <= 4, so the cap
   needs nchunks = ceil(Cin / 16) >= 9.  blk: nblocks = 64, the same.  cls: 65,536 * nchunks + 16 floats at NT = 4 -- at
   nchunks = 8 (Cin 116) the packed filter itself is exactly the cap and the second pass writes the 16 zeros that follow it,
   at Cin 132 it writes filter entries; both are cases.  The generic form: nblocks depends on the padded plane stride
   make_cfg picks, restated in ``lds_cfg``.
   pack_direct: direct_cfg accepts an LDS image of at most (160 KiB - 8 waves * 2,560 B) / 16 B - 1 = 8,959 float4 entries,
   a thirtieth of the cap of 262,144: no accepted layer takes the loop a second time, and the kernel is left alone.
   lat_build_filters: lat_validate accepts Cin 4 or 8 and Cout <= 32, so at most 2 * 2 * 64 = 256 floats per stencil offset;
   the cap needs more than 4,096 offsets, a radius of ten voxels (the models' lattices have 257 at four voxels).  The lattice
   form is no row of matrix(): its case is cconv_forward_ref.lattice_case("over_cap"), run by the same GPU and CPU files."""
import functools

import numpy as np

F = np.float32
EPS = 2.0 ** -24

# ---- A: dmcf_invert_neighbors_list -----------------------------------------------------------------------------------------

SORT_BLOCK_SIZE, SORT_ITEMS_PER_THREAD = 256, 4
SORT_BLOCK_ITEMS = 1024        # block_sort_config::block_size * items_per_thread: the single-block sort up to here
SORT_MERGE_LIMIT = 1 << 20     # radix_sort_config's MergeSortLimit = 1024 * 1024: merge sort up to here, onesweep above
GRID_FOR_CAP = 4096 * 256      # grid_for(n, 256) is capped at 4096 blocks
INT32_MAX = 2 ** 31 - 1

# name -> (P: length of the index buffer, n_inp, kind, options)
INVERT_CASES = {
    "p1_k1": (1, 1, "csr", {}),
    "p2_k2": (2, 2, "csr", {}),
    "p1023_k3": (1023, 3, "csr", {}),
    "p1024_k255": (1024, 255, "csr", {}),
    "p1025_k256_invalid": (1025, 256, "csr", dict(invalid=0.1)),
    "p4097_k257": (4097, 257, "csr", {}),
    "p1023_k65535": (1023, 65535, "csr", {}),
    "p4097_k65536_invalid": (4097, 65536, "csr", dict(invalid=0.1)),
    "p1025_k65537": (1025, 65537, "csr", {}),
    "p1048575_k257": (1_048_575, 257, "csr", {}),
    "p1048576_k65537": (1_048_576, 65537, "csr", {}),
    "p1048577_k256_invalid": (1_048_577, 256, "csr", dict(invalid=0.05)),
    "p1300003_k65536_invalid": (1_300_003, 65536, "csr", dict(invalid=0.05)),
    "slack_p1025_k256": (1025, 256, "csr", dict(covered=900)),
    "slack_p1048577_k65536": (1_048_577, 65536, "csr", dict(covered=1_040_000)),
    "padded_p1025": (1025, 257, "padded", {}),
    "one_key_p1025": (1025, 1, "csr", dict(one_key=True)),
    "one_key_p1048577": (1_048_577, 1, "csr", dict(one_key=True)),
    "descending_p1025": (1025, 1025, "csr", dict(descending=True)),
    "n_out_0": (7, 3, "csr", dict(n_out=0)),
    "p0_k257": (0, 257, "csr", {}),
}


def _row_splits(rng, n_out, covered):
    """n_out rows over [0, covered): random cut points, so some rows are empty and some long."""
    if n_out == 0:
        return np.zeros(1, np.int64)
    cuts = np.sort(rng.integers(0, covered + 1, size=n_out - 1))
    return np.concatenate([[0], cuts, [covered]]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def invert_case(name):
    """-> dict(n_inp, index int32 [P], row_splits int64 [n_out + 1] (row begins of the padded form), row_count int32 [n_out]
    or None, attr float32 [P], and the expected result: m, pair_index / neighbors_index / neighbors_attributes [:m],
    neighbors_row_splits [n_inp + 1]; valid_pos, valid_row, valid_j: the valid pairs in list order).  Read-only arrays."""
    P, n_inp, kind, opt = INVERT_CASES[name]
    rng = np.random.default_rng(sorted(INVERT_CASES).index(name) + 100)
    attr = rng.uniform(-1, 1, size=P).astype(F)
    count = None
    if kind == "padded":
        stride = 7
        n_out = P // stride + 4
        count = rng.integers(0, stride + 1, size=n_out).astype(np.int32)
        count[-4:] = [4, 0, 5, 2]  # row n_out - 4 begins inside the buffer and ends past it; the last three begin past it
        begin = (np.arange(n_out + 1) * stride).astype(np.int64)
        index = np.zeros(P, np.int32)  # the padding slots hold 0, a valid-looking index
        pos, row = [], []
        for i in range(n_out):
            if begin[i] + count[i] <= P:  # (a row that reaches past the buffer is empty as a whole)
                pos.append(begin[i] + np.arange(count[i]))
                row.append(np.full(count[i], i))
        pos, row = np.concatenate(pos).astype(np.int64), np.concatenate(row).astype(np.int64)
        index[pos] = rng.integers(0, n_inp, size=pos.size)
        index[pos[:2]] = [0, n_inp - 1]
        rs = begin
    else:
        covered = opt.get("covered", P)
        n_out = opt.get("n_out", max(1, min(P, P // 8 + 1)))
        rs = _row_splits(rng, n_out, covered if n_out else 0)
        index = np.zeros(P, np.int32)  # the slack past the rows holds 0, a valid-looking index
        c = int(rs[-1])
        if opt.get("one_key"):
            j = np.zeros(c, np.int64)
        elif opt.get("descending"):
            j = np.arange(c - 1, -1, -1, dtype=np.int64)
        else:
            j = rng.integers(0, n_inp, size=c)
            if c >= 2:
                j[rng.permutation(c)[:2]] = [0, n_inp - 1]
            elif c == 1:
                j[0] = 0
        if opt.get("invalid"):
            bad = rng.permutation(c)[2:2 + int(opt["invalid"] * c)]  # (never the two pinned entries: draw them again below)
            j[bad] = np.asarray([-1, n_inp, INT32_MAX])[np.arange(bad.size) % 3]
            ok = np.flatnonzero((j >= 0) & (j < n_inp))
            j[ok[0]], j[ok[-1]] = 0, n_inp - 1
        index[:c] = j
        pos = np.arange(c, dtype=np.int64)
        row = np.repeat(np.arange(n_out, dtype=np.int64), np.diff(rs))
    jj = index[pos].astype(np.int64)
    valid = (jj >= 0) & (jj < n_inp)
    pos, row, jj = pos[valid], row[valid], jj[valid]
    order = np.argsort(jj, kind="stable")
    out = dict(name=name, n_inp=n_inp, index=index, row_splits=rs, row_count=count, attr=attr, m=int(pos.size),
               valid_pos=pos, valid_row=row, valid_j=jj,
               pair_index=pos[order].astype(np.int32), neighbors_index=row[order].astype(np.int32),
               neighbors_attributes=attr[pos[order]],
               neighbors_row_splits=np.concatenate([[0], np.cumsum(np.bincount(jj, minlength=n_inp))]).astype(np.int64))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def check_invert(case, index, row_splits, attributes, pair_index):
    """The five conditions of the exact comparison, on host arrays."""
    m, name = case["m"], case["name"]
    assert np.array_equal(row_splits, case["neighbors_row_splits"]), f"{name}: neighbors_row_splits"
    assert int(row_splits[-1]) == m
    assert np.array_equal(pair_index[:m], case["pair_index"]), f"{name}: pair_index is not the stable order"
    assert np.array_equal(index[:m], case["neighbors_index"]), f"{name}: neighbors_index is not rows[order]"
    assert np.array_equal(attributes[:m], case["neighbors_attributes"]), f"{name}: neighbors_attributes is not attr[order]"
    assert np.all(index[m:] == -1) and np.all(pair_index[m:] == -1), f"{name}: an entry past row_splits[-1] is not -1"


# ---- B: reduce_subarrays_sum / neighbor_counts ----------------------------------------------------------------------------------

ROW_LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33, 255, 256, 257, 4101)
# (rows, position in ROW_LENGTHS of row 0): the lengths cycle, so empty rows sit between long ones; the single rows are a long
# and a short one
REDUCE_CASES = ((1, 11), (1, 4), (15, 0), (16, 5), (17, 0), (4097, 0))


@functools.lru_cache(maxsize=None)
def reduce_case(n_rows, start):
    """-> (values float32, row_splits int64, ref float64 [n_rows], bar [n_rows], lengths); |v| in [0.5, 1], random sign."""
    rng = np.random.default_rng(1000 * n_rows + start)
    lengths = np.asarray([ROW_LENGTHS[(start + r) % len(ROW_LENGTHS)] for r in range(n_rows)], np.int64)
    rs = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    v = (rng.uniform(0.5, 1.0, size=rs[-1]) * rng.choice([-1.0, 1.0], size=rs[-1])).astype(F)
    row = np.repeat(np.arange(n_rows), lengths)
    ref = np.bincount(row, weights=v.astype(np.float64), minlength=n_rows)
    absum = np.bincount(row, weights=np.abs(v).astype(np.float64), minlength=n_rows)
    bar = (np.ceil(lengths / 16) + 5) * EPS * absum
    for a in (v, rs, ref, bar, lengths):
        a.setflags(write=False)
    return v, rs, ref, bar, lengths


WORST = {}  # worst err / bar of B ("reduce") and D ("dense"), printed by the GPU file's test_report_worst_ratio


def _keep_worst(group, err, bar):
    pos = bar > 0
    r = float((err[pos] / bar[pos]).max()) if pos.any() else 0.0
    WORST[group] = max(WORST.get(group, 0.0), r)


def check_reduce(got, ref, bar, lengths):
    got = np.asarray(got)
    assert got.dtype == F and got.shape == ref.shape
    assert np.all(got[lengths == 0] == 0), "an empty row is not exactly 0"
    err = np.abs(got.astype(np.float64) - ref)
    _keep_worst("reduce", err, bar)
    i = int(np.argmax(err - bar))
    assert err[i] <= bar[i], f"row {i} (length {lengths[i]}): err {err[i]:.3g}, bar {bar[i]:.3g}"


# ---- C: the scans, through the public search ---------------------------------------------------------------------------------------

SCAN_TILE = 2048               # kScanTile
SCAN_ROUND = 256 * SCAN_TILE   # elements whose block sums one round of scan_sums_inplace handles
SCAN_SIZES = (2047, 2048, 2049, 4096, 524_287, 524_288, 524_289)
SCAN_RADIUS = 0.1
SITE_COUNTS = np.asarray([1, 2, 3, 4, 0], np.int64)  # points at each site; the fifth has none
POINT_SITE = np.repeat(np.arange(5), SITE_COUNTS)     # the cluster of every point


def scan_points():
    """Ten points: clusters of 1, 2, 3 and 4 at x = 0, 1, 2, 3 (ten radii apart), spread 1e-3 (a hundredth of the radius)."""
    p = np.zeros((POINT_SITE.size, 3), F)
    p[:, 0] = POINT_SITE
    k = np.arange(POINT_SITE.size) - np.concatenate([[0], np.cumsum(SITE_COUNTS)])[POINT_SITE]  # position in the cluster
    p[:, 1] = F(1e-3) * k.astype(F)
    p[:, 2] = F(-5e-4) * k.astype(F)
    return p


def scan_sites(m):
    i = np.arange(m, dtype=np.int64)
    return (7 * i + i // SCAN_TILE) % 5


def scan_queries(m):
    """Query i at site (7 i + i // 2048) % 5, moved off the centre by up to 2e-3 (i % 5 steps)."""
    i = np.arange(m, dtype=np.int64)
    q = np.zeros((m, 3), F)
    q[:, 0] = scan_sites(m)
    q[:, 1] = F(5e-4) * (i % 5).astype(F)
    q[:, 2] = F(2.5e-4) * (i % 3).astype(F)
    return q


def scan_expected(m):
    """(counts, row_splits) by construction."""
    counts = SITE_COUNTS[scan_sites(m)]
    return counts, np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def scan_sample(m, size=4096):
    """min(m, size) query indices, ascending: the first and last 1024, the first tile edge, the rest drawn at random."""
    parts = [np.arange(min(m, 1024)), np.arange(max(m - 1024, 0), m), np.arange(max(SCAN_TILE - 8, 0), min(SCAN_TILE + 8, m)),
             np.random.default_rng(m).permutation(m)[:size]]
    allc = np.concatenate(parts)
    first = np.sort(np.unique(allc, return_index=True)[1])  # (first occurrences, in the order above)
    return np.sort(allc[first][:size])


# ---- D: dense_forward ---------------------------------------------------------------------------------------------------------------

DENSE_ROWS_PER_PASS = 2048 * 4 * 16  # the capped grid's waves x 16 rows: 131,072
DENSE_N = (15, 16, 17, 63, 64, 65, 131_072, 131_073, 262_147)
DENSE_KM = ((32, 32), (64, 64), (12, 4), (20, 40))
DENSE_BAR = 4e-7  # test_dense_forward_against_float64's


def dense_case(n, k, m):
    rng = np.random.default_rng(n * 7 + k * 100 + m)
    x = rng.normal(size=(n, k)).astype(F)
    W = rng.normal(size=(k, m)).astype(F)
    b = rng.normal(size=(m,)).astype(F)
    r = rng.normal(size=(n, m)).astype(F)
    ref = x.astype(np.float64) @ W.astype(np.float64)
    scale = np.abs(x).astype(np.float64) @ np.abs(W).astype(np.float64)
    return x, W, b, r, ref, scale


def check_dense(y, yb, b, r, ref, scale):
    err, bar = np.abs(y - ref), DENSE_BAR * scale + 1e-30
    _keep_worst("dense", err, bar)
    assert (err <= bar).all(), f"plain: worst err / bar {(err / bar).max():.3g} in row {int(np.argmax((err / bar).max(1)))}"
    err, bar = np.abs(yb - (ref + b + r)), DENSE_BAR * (scale + np.abs(b) + np.abs(r)) + 1e-30
    _keep_worst("dense", err, bar)
    assert (err <= bar).all(), f"bias + residual: worst err / bar {(err / bar).max():.3g} in row {int(np.argmax((err / bar).max(1)))}"


# ---- E: farthest point sampling and gather_point -------------------------------------------------------------------------------------

FPS_THREADS = 1024
FPS_REG_POINTS = 8 * FPS_THREADS  # points 0 .. 8191 live in registers, the rest in the workspace
FPS_SIZES = (1023, 1024, 1025, 8191, 8192, 8193)
FPS_SAMPLES = 40
COPIES_OF = (5, 300, 700)
FPS_TIES = (("copies", 8193), ("mirror", 8193), ("lattice", 8193), ("copies", 9000), ("lattice", 9000))


def fps_cloud(n):
    return np.random.default_rng(n).uniform(-1, 1, size=(n, 3)).astype(F)


def _lattice(n, pairs, others):
    """The first n points of a 21 x 21 x 21 lattice (spacing 1 / 8, centred) reordered: its centre is point 0, the corner pairs
    (c, -c) sit at the index pairs ``pairs`` -- a multiple of 512 apart, on either side of 8192 -- and the remaining corners
    at ``others``.  From the centre all eight corners are equally far: sample 1 is a tie among them."""
    g = (np.arange(21, dtype=F) - F(10)) * F(0.125)
    p = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)

    def place(point, at):
        src = int(np.flatnonzero(np.all(p == np.asarray(point, F), axis=1))[0])
        p[[src, at]] = p[[at, src]]
    place((0, 0, 0), 0)
    corners = [(sx * 1.25, sy * 1.25, sz * 1.25) for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)]
    half = corners[:4]  # (+, ., .): their mirror images are the other four
    spots = []
    for c, (lo, hi) in zip(half, pairs):
        spots += [(c, lo), (tuple(-v for v in c), hi)]
    rest = [c for c in corners if c not in [s[0] for s in spots]]
    spots += list(zip(rest, others))
    for c, at in spots:
        place(c, at)
    return np.ascontiguousarray(p[:n])


@functools.lru_cache(maxsize=None)
def fps_tie_points(kind, n):
    if kind == "copies":
        # point k + 8192 is an exact copy of point k: far outliers, so that sampling reaches them (and ties) early
        p = fps_cloud(n)
        for t, k in enumerate(k for k in COPIES_OF if k + FPS_REG_POINTS < n):
            p[k] = F([3.0 + t, -2.0 * t, 1.5])
            p[k + FPS_REG_POINTS] = p[k]
        if n == FPS_REG_POINTS + 1:  # (one workspace point only: the copy of point 0, which is sample 0)
            p[FPS_REG_POINTS] = p[0]
    elif kind == "mirror":
        # points 1 and 8192 are mirror images about point 0 and the farthest from it: 8192 & 511 = 0 < 1 wins
        p = F(0.5) * fps_cloud(n)
        p[0] = 0
        p[1], p[FPS_REG_POINTS] = F([3, 0, 0]), F([-3, 0, 0])
    else:
        if n == FPS_REG_POINTS + 1:
            p = _lattice(n, [(512, 8192)], [1, 2, 3, 4, 5, 6])
        else:
            p = _lattice(n, [(1, 8193), (2, 8194), (3, 8195), (4, 8196)], [])
    p.setflags(write=False)
    return p


def fps_replay(p, m):
    """Farthest point sampling restated with its tie sets: -> (indices int32 [m], [candidates of step j] for j = 1 .. m - 1).
    Un-fused float32 (dx dx + dy dy) + dz dz, running minimum; among equal maxima the smallest (i & 511, i)."""
    p = np.asarray(p, F)
    n = p.shape[0]
    idx, ties = np.zeros(m, np.int32), []
    temp = np.full(n, F(1e38), F)
    k = np.arange(n)
    old = 0
    for j in range(1, m):
        d = p - p[old]
        d2 = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).astype(F) + d[:, 2] * d[:, 2]).astype(F)
        temp = np.minimum(temp, d2)
        cand = np.flatnonzero(temp == temp.max())
        old = int(cand[np.lexsort((cand, cand & 511))[0]])
        idx[j] = old
        ties.append(cand)
    return idx, ties


# (m, channels): m * channels at 255, 256, 257 (257 is prime) and next to them
GATHER_CASES = ((255, 1), (256, 1), (257, 1), (85, 3), (86, 3), (51, 5), (52, 5), (3, 64), (4, 64), (5, 64))
GATHER_N = 37  # rows to gather from: fewer than any m but the 64-channel ones', so indices repeat


def gather_case(m, ch):
    rng = np.random.default_rng(m * 100 + ch)
    feats = rng.normal(size=(GATHER_N, ch)).astype(F)
    idx = rng.integers(0, GATHER_N, size=m).astype(np.int32)
    idx[-1] = idx[0]  # a repeat whatever m
    return feats, idx


# ---- F: the backward past the cap of grid_for ----------------------------------------------------------------------------------------

# (stored filter shape, sym_axis or None, Cin, Cout, accumulate): the full kernel is (4, 4, 4) in all.  The third accumulates into
# non-zero gradients: a second pass of cconv_bwd_filter_store that re-visits elements writes the same value again without it
BWD_CAP_CASES = (((4, 4, 4), None, 128, 132, False), ((4, 4, 2), 2, 128, 132, False), ((4, 4, 4), None, 128, 132, True))
BWD_CAP_POINTS = 300
BWD_CAP_RADIUS = 0.15  # test_tile_edges'


def bwd_cap_counts(shape, sym_axis, cin, cout):
    """(K of the full kernel, elements of the full gradient, elements of the stored one)."""
    full = list(shape)
    if sym_axis is not None:
        full[sym_axis] *= 2
    K = full[0] * full[1] * full[2]
    return K, K * cin * cout, shape[0] * shape[1] * shape[2] * cin * cout


# ---- G: the forward filter packers -----------------------------------------------------------------------------------------------------

PACK_FILTER_CAP = 2048 * 256
PACK_DIRECT_CAP = 1024 * 256
LAT_BUILD_CAP = 4096 * 256


def lds_cfg(sx, sy, sz, cin, cout):
    """make_cfg of cconv.hip: -> dict(CC, PS, nblocks, NT, nchunks, lds, packed_floats)."""
    TM, waves, threads, stage = 16, 8, 512, 64 * 17
    CC = 4 if cin <= 4 else 8
    PR = sx * sy * CC

    def conflicts(PS, zgroup):
        bad = 0
        for by in range(2):
            for bx in range(2):
                off = []
                for t in range(8):
                    tx, ty, tz = (t & 1) and sx >= 2, ((t >> 1) & 1) and sy >= 2, ((t >> 2) & 1) and sz >= 2
                    off.append(int(bool(tz)) * PS + ((by + int(bool(ty))) * sx + bx + int(bool(tx))) * CC)
                rd = 64 if CC == 8 else 32
                for a in range(8):
                    for b in range(a + 1, 8):
                        if off[a] == off[b]:
                            continue
                        if (off[a] % rd) // CC == (off[b] % rd) // CC:
                            bad += 1
                        ga, gb = ((a >> 1) & 1, (b >> 1) & 1) if zgroup else (a >> 2, b >> 2)
                        if ga == gb and (off[a] % 32) // CC == (off[b] % 32) // CC:
                            bad += 1
        return bad
    has_dead = sx < 2 or sy < 2 or sz < 2

    def lds_bytes(PS):
        kcx = (sz * PS + 15) // 16 * 16
        kcp = kcx + ((4 - kcx % 64) + 64) % 64
        bf = max(TM * kcp, waves * TM * 16 * ((cout + 15) // 16))
        return (bf + TM + waves * stage + (2 * threads if has_dead else 0)) * 4
    PS0 = (PR + 7) // 8 * 8
    step = 80 * 1024 if lds_bytes(PS0) <= 80 * 1024 else 160 * 1024
    best, best_bad = PS0, 1 << 30
    for zgroup in range(2):
        if best_bad <= 0:
            break
        for k in range(12):
            PS = PS0 + 8 * k
            if k > 0 and (sz < 2 or lds_bytes(PS) > step):
                break
            bad = conflicts(PS, zgroup)
            if bad < best_bad:
                best_bad, best = bad, PS
            if bad == 0:
                break
    KC = (sz * best + 15) // 16 * 16
    nblocks, NT, nchunks = KC // 16, (cout + 15) // 16, (cin + CC - 1) // CC
    return dict(CC=CC, PS=best, nblocks=nblocks, NT=NT, nchunks=nchunks, lds=lds_bytes(best),
                packed_floats=nchunks * nblocks * 4 * NT * 16 * 4)


def mfma_packed(K, cin, cout):
    return ((cin + 15) // 16) * (16 * ((K + 15) // 16)) * 4 * ((cout + 15) // 16) * 16 * 4


def blk_packed(cin, cout):
    return ((cin + 15) // 16) * 64 * 4 * ((cout + 15) // 16) * 16 * 4


def cls_packed(cin, cout):
    return ((cin + 15) // 16) * 64 * 4 * ((cout + 15) // 16) * 16 * 4 + 16


def direct_largest_image():
    """The largest LDS image (float4 entries) direct_cfg accepts: at least 8 waves of 2,560 staging bytes must fit beside the
    image and its one zero entry in 160 KiB."""
    return (160 * 1024 - 8 * 64 * 10 * 4) // 16 - 1


def lat_packed(n_offsets, cin, cout):
    return ((n_offsets + 3) // 4) * 4 * ((cin + 3) // 4) * ((cout + 15) // 16) * 64


# the lattice case above lat_build_filters' cap (cconv_forward_ref.lattice_case("over_cap")): the widest filter the form
# accepts per offset (Cin 8, two column tiles) on a lattice of spacing 0.05 with a radius of 10.2 voxels
LAT_OVER_CAP = dict(cin=8, cout=17, voxel=0.05, radius=0.51)


def lattice_offset_count(voxel, radius):
    """The stencil offsets of ops.lattice_offsets on a cubic lattice without a shift: integer d with |d * voxel| <= radius,
    decided in float32 on the un-fused squared distance."""
    v = F(voxel)
    r = int(np.floor(radius / float(v))) + 1
    ax = np.arange(-r, r + 1, dtype=np.int32).astype(F) * v
    z, y, x = np.meshgrid(ax, ax, ax, indexing="ij")
    return int((((x * x + y * y) + z * z) <= F(radius) * F(radius)).sum())


def _smallest_lds_over_cap():
    """The smallest Cin at which the generic form's packed 4x4x4 filter with four column tiles (Cout 49) exceeds the cap."""
    cin = 8
    while lds_cfg(4, 4, 4, cin, 49)["packed_floats"] <= PACK_FILTER_CAP:
        cin += 1
    return cin


LDS_OVER_CAP = (_smallest_lds_over_cap(), 49)
# forced kernel -> [(Cin, Cout)] of the 4x4x4 cases above the cap that tests/cconv_forward_ref.matrix() carries
PACKER_CASES = {"lds": [LDS_OVER_CAP], "mfma": [(129, 49)], "blk": [(132, 49)], "cls": [(116, 49), (132, 49)]}


def packed_count(kernel, cin, cout):
    if kernel == "lds":
        cfg = lds_cfg(4, 4, 4, cin, cout)
        assert cfg["lds"] <= 160 * 1024, "generic_launch refuses the shape"
        return cfg["packed_floats"]
    if kernel == "mfma":
        return mfma_packed(64, cin, cout)
    return blk_packed(cin, cout) if kernel == "blk" else cls_packed(cin, cout)


def packer_table():
    """[(packer, cap, largest reachable count or None when unbounded, smallest accepted count above the cap or None)]."""
    rows = [(f"pack_filter ({k})" if k != "cls" else "pack_filter_cls", PACK_FILTER_CAP, None,
             packed_count(k, *PACKER_CASES[k][0])) for k in ("lds", "mfma", "blk", "cls")]
    rows.append(("pack_direct", PACK_DIRECT_CAP, direct_largest_image(), None))
    n_off = lattice_offset_count(LAT_OVER_CAP["voxel"], LAT_OVER_CAP["radius"])
    rows.append(("lat_build_filters", LAT_BUILD_CAP, None, lat_packed(n_off, LAT_OVER_CAP["cin"], LAT_OVER_CAP["cout"])))
    return rows
