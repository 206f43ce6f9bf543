"""Reference and scenes of the batched neighbour search (points_row_splits / queries_row_splits), shared by
tests/test_batched_search_ref_cpu.py (the reference against the oracle, the scenes against their own conditions) and
tests/test_gpu_batched_search.py (the HIP search and the batched ContinuousConv against the reference).

The reference is the float32 numpy brute force of tests/test_gpu_radius_search.py -- un-fused ((dx*dx + dy*dy) + dz*dz),
inclusive -- run once per batch item; the rows are concatenated and the indices offset by the item's first point.

A scene is a dict: points [n,3], queries [m,3], prs / qrs (int64 row splits of length batch + 1), radius.  Scenes are
deterministic, built once per process and never written to."""
import functools

import numpy as np

from test_gpu_radius_search import brute_force


def splits(counts):
    return np.concatenate([[0], np.cumsum(np.asarray(counts, np.int64))]).astype(np.int64)


def batched_brute_force(points, queries, radii, prs, qrs, ignore_query_point=False):
    """-> (index int32 into the concatenated points, row_splits int64 over all queries, d2 float32).  ``radii``: one radius, or
    one per query."""
    points, queries = np.asarray(points, np.float32), np.asarray(queries, np.float32)
    radii = np.broadcast_to(np.asarray(radii, np.float32), (queries.shape[0],))
    idx, cnt, dist = [], [], []
    for b in range(len(prs) - 1):
        p0, p1, q0, q1 = int(prs[b]), int(prs[b + 1]), int(qrs[b]), int(qrs[b + 1])
        if q1 == q0:
            continue
        if p1 == p0:
            cnt.append(np.zeros(q1 - q0, np.int64))
            continue
        i, rs, d = brute_force(points[p0:p1], queries[q0:q1], radii[q0:q1], ignore_query_point)
        idx.append(i + np.int32(p0))
        dist.append(d)
        cnt.append(np.diff(rs))
    rs = splits(np.concatenate(cnt) if cnt else np.zeros(0, np.int64))
    if not idx:
        return np.zeros(0, np.int32), rs, np.zeros(0, np.float32)
    return np.concatenate(idx).astype(np.int32), rs, np.concatenate(dist).astype(np.float32)


@functools.lru_cache(maxsize=None)
def reference(name, ignore=False, dim=3):
    """The batched brute force of scene ``name`` at its one radius (computed once, shared, read-only)."""
    s = scene(name, dim)
    ref = batched_brute_force(s["points"], s["queries"], s["radius"], s["prs"], s["qrs"], ignore)
    for a in ref:
        a.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def scene(name, dim=3):
    s = SCENES[name](dim) if name in ("overlapping",) else SCENES[name]()
    for v in s.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return s


def item_rows(s, b):
    """(points of item b, queries of item b, first point, first query)."""
    p0, p1, q0, q1 = (int(v) for v in (s["prs"][b], s["prs"][b + 1], s["qrs"][b], s["qrs"][b + 1]))
    return s["points"][p0:p1], s["queries"][q0:q1], p0, q0


def mean_row_lengths(s, ref):
    """{item: mean row length} of the items that have points and queries."""
    rs = ref[1]
    out = {}
    for b in range(len(s["prs"]) - 1):
        p0, p1, q0, q1 = (int(v) for v in (s["prs"][b], s["prs"][b + 1], s["qrs"][b], s["qrs"][b + 1]))
        if p1 > p0 and q1 > q0:
            out[b] = float(rs[q1] - rs[q0]) / (q1 - q0)
    return out


def _blob(rng, n, sigma=0.2):
    """n points of the box [-1, 1]^3: a normal cloud around the origin, clipped to the box (dense enough in the middle for rows
    of tens of neighbours at radius 0.12, with a thin halo that reaches the faces of the box)."""
    return np.clip(rng.normal(0.0, sigma, size=(n, 3)), -1.0, 1.0).astype(np.float32)


OVERLAP_POINTS = (3000, 0, 1, 700, 2500)
OVERLAP_QUERIES = (1000, 40, 0, 900, 1)


def _overlapping(dim=3):
    """Five items drawn from the same box [-1, 1]^3, so that every item lies on top of every other: item 3's points are a copy
    of item 0's first 700 (coincident across items), 600 queries sit on points of their own item (300 of item 0, 299 of
    item 3, the one of item 4), item 1 has queries and no points, item 2 one point and no query."""
    rng = np.random.default_rng(20 + dim)
    pts = [_blob(rng, n) for n in OVERLAP_POINTS]
    pts[3] = pts[0][:700].copy()
    qs = [_blob(rng, m) for m in OVERLAP_QUERIES]
    # a tenth of the queries anywhere in the box, also outside the grid's bulk
    for b in (0, 3):
        k = OVERLAP_QUERIES[b] // 10
        qs[b][-k:] = rng.uniform(-1, 1, size=(k, 3)).astype(np.float32)
    qs[0][:300] = pts[0][100:400]
    qs[3][:299] = pts[3][401:700]
    qs[4][0] = pts[4][int(np.argmin(np.square(pts[4]).sum(1)))]
    points, queries = np.concatenate(pts), np.concatenate(qs)
    if dim == 2:
        points[:, 2] = 0
        queries[:, 2] = 0
    return dict(points=points, queries=queries, prs=splits(OVERLAP_POINTS), qrs=splits(OVERLAP_QUERIES), radius=0.12,
                on_points=600)


EDGE_POINTS = (0, 400, 0, 0, 300, 500, 350, 0)
EDGE_QUERIES = (0, 300, 25, 0, 1, 200, 2, 0)


def _edges():
    """Empty items first, last and twice in a row (item 2 has queries and no points: their rows are empty); items of one and
    of two queries, whose first and last rows are neighbours in the query array."""
    rng = np.random.default_rng(31)
    pts = [_blob(rng, n, 0.15) for n in EDGE_POINTS]
    qs = [_blob(rng, m, 0.12) for m in EDGE_QUERIES]
    # (the lone query of item 4 sits in the middle of its item's cloud, next to a point, not on it)
    qs[4][0] = pts[4][int(np.argmin(np.square(pts[4]).sum(1)))] + np.float32([0.01, 0, 0])
    return dict(points=np.concatenate(pts), queries=np.concatenate(qs), prs=splits(EDGE_POINTS), qrs=splits(EDGE_QUERIES),
                radius=0.1)


STRAYS = np.float32([[1e4, 1e4, 1e4], [-1e4, -1e4, -1e4], [0, 0, 50], [0, 0, -50]])
STRAY_POINTS = (1500, 1200, 1000)
STRAY_QUERIES = (600, 500, 400)


def _strays():
    """Three items far from each other -- offsets (40, 0, 0) and (0, -25, 3) -- so that the one grid of the call is coarse;
    item 0 ends in four stray points far outside everything, each with a query of ITS item next to it (the first four queries
    of item 0) and a query of item 1 at the very same place (the first four of item 1), which must find nothing."""
    rng = np.random.default_rng(32)
    offs = np.float32([[0, 0, 0], [40, 0, 0], [0, -25, 3]])
    pts = [_blob(rng, n, 0.25) + o for n, o in zip(STRAY_POINTS, offs)]
    qs = [_blob(rng, m, 0.25) + o for m, o in zip(STRAY_QUERIES, offs)]
    pts[0][-4:] = STRAYS
    near = STRAYS + np.float32([0.05, -0.03, 0.02])
    qs[0][:4] = near
    qs[1][:4] = near
    return dict(points=np.concatenate(pts).astype(np.float32), queries=np.concatenate(qs).astype(np.float32),
                prs=splits(STRAY_POINTS), qrs=splits(STRAY_QUERIES), radius=0.15, stray_points=np.arange(1496, 1500),
                stray_queries=np.arange(0, 4), foreign_queries=np.arange(600, 604))


def _many():
    """130 items of 50 to 400 points in the unit square (z = 0), 20 to 100 queries each."""
    rng = np.random.default_rng(33)
    np_, nq = rng.integers(50, 401, size=130), rng.integers(20, 101, size=130)
    np_[0], np_[-1] = 50, 400
    points = rng.uniform(0, 1, size=(int(np_.sum()), 3)).astype(np.float32)
    queries = rng.uniform(0, 1, size=(int(nq.sum()), 3)).astype(np.float32)
    points[:, 2] = 0
    queries[:, 2] = 0
    return dict(points=points, queries=queries, prs=splits(np_), qrs=splits(nq), radius=0.3)


TABLE_BATCH, TABLE_N = 16, 2025


def _table_bound():
    """16 x 2,025 points in the unit square (z = 0), in two bands along its lower and upper edge, searched from themselves.
    The cell table of the call has 4 * 32,400 entries, 8,100 per item; cells of edge R / 3 at R = 0.03 would be 100 x 100 per
    item, so the build has to take coarser cells."""
    rng = np.random.default_rng(34)
    pts = rng.uniform(0, 1, size=(TABLE_BATCH * TABLE_N, 3)).astype(np.float32)
    y = pts[:, 1] * np.float32(0.4)
    pts[:, 1] = np.where(y > 0.2, y + np.float32(0.6), y)
    pts[:, 2] = 0
    for b in range(TABLE_BATCH):  # (the corners of the square belong to every item)
        pts[b * TABLE_N:b * TABLE_N + 4, :2] = np.float32([[0, 0], [1, 0], [0, 1], [1, 1]])
    rs = splits([TABLE_N] * TABLE_BATCH)
    return dict(points=pts, queries=pts, prs=rs, qrs=rs, radius=0.03)


SCENES = {"overlapping": _overlapping, "edges": _edges, "strays": _strays, "many": _many, "table_bound": _table_bound}


# ---- the layer's scene ---------------------------------------------------------------------------------------------------------

LAYER_POINTS = (300, 0, 450)
LAYER_OUTPUTS = (200, 50, 0)
LAYER_EXTENT = 2 * 0.23


@functools.lru_cache(maxsize=None)
def layer_scene():
    """B = 3 in [-0.5, 0.5]^3: input points [300, 0, 450], separate output points [200, 50, 0] (item 1's outputs have no input,
    item 2's inputs no output), features [750, 8], filters [4, 4, 4, 8, 16], a gradient for either output set."""
    rng = np.random.default_rng(35)
    n, m = sum(LAYER_POINTS), sum(LAYER_OUTPUTS)
    s = dict(inp=rng.uniform(-0.5, 0.5, size=(n, 3)).astype(np.float32),
             out=rng.uniform(-0.5, 0.5, size=(m, 3)).astype(np.float32),
             feat=rng.normal(size=(n, 8)).astype(np.float32),
             filt=rng.uniform(-1, 1, size=(4, 4, 4, 8, 16)).astype(np.float32),
             grad_same=rng.normal(size=(n, 16)).astype(np.float32),
             grad_sep=rng.normal(size=(m, 16)).astype(np.float32),
             # two extent groups for the rank-1 run, one value per output point
             ext_same=rng.choice(np.float32([LAYER_EXTENT, 0.36]), size=n).astype(np.float32),
             ext_sep=rng.choice(np.float32([LAYER_EXTENT, 0.36]), size=m).astype(np.float32),
             irs=splits(LAYER_POINTS), ors=splits(LAYER_OUTPUTS))
    for v in s.values():
        v.setflags(write=False)
    return s
