"""The grid regimes of the radius search (dmcf_amd/csrc/frs.hip), shared by tests/test_frs_regimes_cpu.py (the scenes against the
host restatement of the sizing, the measurement of C_WIN, the teeth of the checkers) and tests/test_gpu_frs_regimes.py (every
form of the search on each regime, asserted from the header the DEVICE built).

Reading the structure back: ``decode(table)`` copies ``SpatialHashTable.workspace`` to the host and returns the header
(FrsHeader, the first 128 bytes) and the cell sort (cell_start, and the x, y, z, index entries of ``sorted``), by the layout of
frs_layout; it asserts that the layout has not drifted.

Restating the build: ``sizing`` is frs_finish_header_one in numpy (the same float32 / float64 steps), ``cell_coords`` the float32
cell_coord, ``expected_sort`` the stable sort of the point indices by cell.

Scenes (SCENES): deterministic, read-only, at most 4,040 points, so that the brute force is cheap and both builds
(frs_build_small, and the general one under DMCF_FRS_NO_SMALL_BUILD) can run.  Each names the regime that must be asserted from
the device's header (``Scene.regime``); ``decisions`` lists the comparisons of the sizing that put it there, for the CPU test's
"no threshold within 10 %".

References: the float32 un-fused brute force of tests/test_gpu_radius_search.py (L2, also with a radius per query), a max-norm
variant of it, and for the fused window sum a float64 sum over the brute-force pair list with the formulas of
tests/density_grad_ref.py.  (density_grad_ref.WindowSum itself drops the coincident pairs of the sqrt-based windows, which the
gradient needs and the forward sum must not: every fourth point of a scene is a query, so the sum here keeps them.)

The window-sum bar, element by element:

    |gpu - ref64| <= ((ceil(n / 64) + 7) * A_i + C_WIN * k_i) * 2^-24

A_i = sum |w| over the row, k_i the row length.  ceil(n / 64) + 7: no lane adds more than ceil(n / 64) terms before the 6-step
butterfly.  C_WIN covers the rounding of one term -- the float32 un-fused d^2, inv_r2 = 1 / (R * R), q = d^2 * inv_r2 and the
formulas of window_value -- and is MEASURED, by tests/test_frs_regimes_cpu.py::test_c_win_is_the_measured_constant, on a float32
numpy restatement of one term against float64 over every pair of every scene; times 4 (the GPU's sqrt and reciprocal are not
correctly rounded, and its compiler may contract a product and a sum: the margin C_GEO takes), rounded up to a power of two."""
import functools
import math

import numpy as np

import density_grad_ref as dg
from test_gpu_radius_search import brute_force

F = np.float32
EPS = 2.0 ** -24
SPREAD = 3.0          # kFrsSpread
CELL_DIV = 3          # FRS_CELL_DIV
WIN = 4               # kWin: 64-wide candidate windows in flight per iteration of the scan
WINDOWS = ["poly6", "cubic", "linear", "peak", "cubic_grad", "explicit"]

MEASURED_C_WIN = 20.0
C_WIN = 128.0


# ---- layout and decoding ---------------------------------------------------------------------------------------------------

def table_size(n, batch=1):
    return max(min(max(4 * n, 4096), 1 << 26), batch)


def _up(x):
    return (x + 255) // 256 * 256


def layout(n, batch=1):
    """Byte offsets of frs_layout up to the end of ``sorted`` (what does not depend on the number of queries)."""
    t, nn = table_size(n, batch), max(n, 1)
    off, o = {"table": t}, 0
    for name, size in (("header", 128), ("cell_start", (t + 1) * 4), ("cell_fill", (t + 1) * 4), ("point_cell", nn * 4),
                       ("tmp_idx", nn * 4), ("sorted", nn * 16)):
        off[name] = o
        o += _up(size)
    off["end"] = o
    return off


def _ord2f(u):
    """ord2f of frs.hip: the order-preserving uint32 encoding of a float, back to the float."""
    u = np.asarray(u, np.uint32)
    return np.where(u & np.uint32(0x80000000), u & np.uint32(0x7fffffff), ~u).astype(np.uint32).view(F)


def decode_header(buf):
    b = np.ascontiguousarray(np.asarray(buf[:128], np.uint8))
    return dict(origin=b[0:12].view(F).copy(), inv_cell=b[12:24].view(F).copy(), dims=b[24:36].view(np.int32).copy(),
                ncells=int(b[36:40].view(np.int32)[0]), bb_min=_ord2f(b[40:52].view(np.uint32)),
                bb_max=_ord2f(b[52:64].view(np.uint32)), radius=b[64:68].view(F)[0], n_points=int(b[68:72].view(np.int32)[0]),
                sum=b[72:96].view(np.float64).copy(), sumsq=b[96:120].view(np.float64).copy())


def decode_bytes(buf, n, radius, limit, batch=1):
    """The header and the cell sort out of the workspace bytes ``buf`` of a structure over ``n`` points built for ``radius``;
    ``limit``: what dmcf_frs_workspace_bytes(n, 0) (or its batched form) says."""
    L = layout(n, batch)
    assert L["sorted"] + n * 16 <= limit <= len(buf), "the layout restated here reaches beyond the workspace"
    h = decode_header(buf)
    assert int(h["dims"][0]) * int(h["dims"][1]) * int(h["dims"][2]) == h["ncells"], "dims / ncells: the header layout has drifted"
    assert h["radius"] == F(radius) and h["n_points"] == n, "radius / n_points: the header layout has drifted"
    t = L["table"]
    h["table"] = t
    h["cell_start"] = np.ascontiguousarray(buf[L["cell_start"]:L["cell_start"] + (t + 1) * 4]).view(np.uint32).copy()
    s = np.ascontiguousarray(buf[L["sorted"]:L["sorted"] + n * 16]).view(F).reshape(n, 4)
    h["sorted_xyz"] = s[:, :3].copy()
    h["sorted_index"] = s[:, 3].copy().view(np.int32)
    return h


def decode(table):
    """The header and the cell sort of a ``SpatialHashTable`` (batched or not), copied from the device."""
    from dmcf_amd import _lib
    n = int(table.points.shape[0])
    buf = table.workspace.cpu().numpy()
    if table.row_splits is None:
        return decode_bytes(buf, n, table.radius, _lib.lib().dmcf_frs_workspace_bytes(n, 0))
    batch = len(table.row_splits) - 1
    return decode_bytes(buf, n, table.radius, _lib.lib().dmcf_frs_workspace_bytes_batched(n, 0, batch), batch)


# ---- the sizing and the sort, restated -----------------------------------------------------------------------------------------

def box_sums(points):
    """bb_min, bb_max (float32) and the float64 sums of x and of the float32 x * x (the device adds float32 partial sums in an
    order of its own: the last digits differ, which is why no scene may sit near a threshold)."""
    p = np.asarray(points, F)
    return p.min(0), p.max(0), p.astype(np.float64).sum(0), (p * p).astype(np.float64).sum(0)


def sizing(bb_min, bb_max, s1, s2, n, radius, table=None, batch=1):
    """frs_finish_header_one.  -> dict(origin, inv_cell, dims, ncells, cell, div, decisions); ``div``: 3, 2, 1 cells per
    radius, 0 when the grid was coarsened to fit the table.  ``decisions``: the comparisons that chose the regime, as
    (what, value, threshold, taken) with taken = value <= threshold -- the two conditions of every cell edge tried, and the
    first "does it fit" of the coarsening loop.  (The later rounds of that loop aim 2 % below the table on purpose and only
    decide how coarse, not whether.)"""
    table = table_size(n, batch) if table is None else table
    slab, fill = float(table // batch), float(batch)
    radius = F(radius)
    lo, ext = np.zeros(3, F), np.zeros(3, F)
    for a in range(3):
        lo[a], hi = F(bb_min[a]), F(bb_max[a])
        ext[a] = hi - lo[a]
        if not ext[a] >= 0 or not np.isfinite(ext[a]):
            ext[a] = 0
        if not np.isfinite(lo[a]):
            lo[a] = 0
        if n > 0:
            mean = s1[a] / n
            var = s2[a] / n - mean * mean
            sd = math.sqrt(var) if var > 0 else 0.0
            blo, bhi = F(mean - SPREAD * sd), F(mean + SPREAD * sd)
            if np.isfinite(blo) and np.isfinite(bhi) and bhi > blo:
                nlo, nhi = max(lo[a], blo), min(hi, bhi)
                if nhi >= nlo:
                    lo[a], ext[a] = nlo, F(nhi - nlo)
    decisions = []

    def cells(c):
        cnt = [math.floor(float(ext[a]) / float(c)) + 1.0 for a in range(3)]
        return cnt, cnt[0] * cnt[1] * cnt[2]

    cell, div_taken = F(radius * F(1.001)), 1
    for div in range(CELL_DIV, 1, -1):
        c = F(F(radius * F(1.001)) / F(div))
        _, prod = cells(c)
        fits, dense = prod <= slab, n >= 0.5 * prod * fill
        decisions.append((f"R/{div} fits the table", prod, slab, fits))
        decisions.append((f"R/{div} one point per two cells", 0.5 * prod * fill, float(n), dense))
        if fits and dense:
            cell, div_taken = c, div
            break
    d = [1, 1, 1]
    for it in range(64):
        cnt, prod = cells(cell)
        d = [2000000000 if c > 2.0e9 else int(c) for c in cnt]
        if it == 0:
            decisions.append(("the chosen cell fits the table", prod, slab, prod <= slab))
        if prod <= slab:
            break
        div_taken = 0
        grow = F(F(np.cbrt(prod / slab)) * F(1.02))
        cell = F(cell * (grow if grow > F(1.05) else F(1.05)))
    return dict(origin=lo.copy(), inv_cell=np.full(3, F(1) / cell, F), dims=np.array(d, np.int32), ncells=d[0] * d[1] * d[2],
                cell=cell, div=div_taken, decisions=decisions, radius=radius, n_points=n, table=table)


def host_header(points, radius):
    return sizing(*box_sums(points), len(points), radius)


def cell_coords(x, header):
    """The float32 cell_coord of every row of ``x`` [k, 3]: floorf((x - origin) * inv) clamped to [-1, dim] (NaN -> -1)."""
    x = np.asarray(x, F)
    c = np.floor((x - header["origin"].astype(F)) * header["inv_cell"].astype(F))
    c = np.fmin(np.fmax(c, F(-1)), header["dims"].astype(F))
    return c.astype(np.int32)


def binning(points, header):
    """-> (cell of every point, mask of the points binned from beyond the grid, occupancy of every cell)."""
    c = cell_coords(points, header)
    dims = header["dims"].astype(np.int32)
    beyond = np.any((c < 0) | (c > dims - 1), axis=1)
    c = np.minimum(np.maximum(c, 0), dims - 1)
    cell = (c[:, 2] * dims[1] + c[:, 1]) * dims[0] + c[:, 0]
    return cell, beyond, np.bincount(cell, minlength=int(header["ncells"]))


def border_cells(header):
    """Mask over the cells: on the outermost layer of an axis that has more than one cell."""
    d = [int(v) for v in header["dims"]]
    z, y, x = np.meshgrid(np.arange(d[2]), np.arange(d[1]), np.arange(d[0]), indexing="ij")
    m = np.zeros_like(x, bool)
    for c, n in ((x, d[0]), (y, d[1]), (z, d[2])):
        if n > 1:
            m |= (c == 0) | (c == n - 1)
    return m.reshape(-1)


def expected_sort(points, header):
    """The point indices in the order of ``sorted``: by cell, then by index."""
    return np.argsort(binning(points, header)[0], kind="stable").astype(np.int32)


def cells_per_radius(header):
    return float(F(header["radius"]) * header["inv_cell"][0])


# ---- scenes ----------------------------------------------------------------------------------------------------------------------

CORNERS = np.array([[x, y, z] for z in (0, 1) for y in (0, 1) for x in (0, 1)], F)


def _uniform(rng, n):
    return rng.uniform(0, 1, size=(n, 3)).astype(F)


def _clumps(rng, n, k, sigma):
    """n points in k normal clumps of width sigma, clipped to the unit cube whose corners are the first eight points."""
    centres = rng.uniform(0.1, 0.9, size=(k, 3))
    p = np.clip(centres[rng.integers(0, k, size=n)] + rng.normal(0, sigma, size=(n, 3)), 0, 1).astype(F)
    p[:8] = CORNERS
    return p


def _div3(rng, n):
    return _uniform(rng, n)


def _div2(rng, n):
    return _uniform(rng, n)


def _div1(rng, n):
    return _clumps(rng, n, 60, 0.02)


def _coarse(rng, n):
    return _clumps(rng, n, 60, 0.008)


def _plane(rng, n):
    p = _uniform(rng, n)
    p[:, 2] = 0
    return p


def _line(rng, n):
    p = _uniform(rng, n)
    p[:, 0] = 0
    p[:, 2] = 0
    return p


def _same(rng, n):
    return np.zeros((n, 3), F) + F(0.25)


CLUMP_AT = 0.39


def _clump(rng, n):
    """A quarter uniform in the unit cube, three quarters in a cube of edge 0.05: the grid covers mean +- 3 sigma, which the
    clump pulls in, so a share of the uniform points is binned from beyond it; the clump fills one cell of edge R / 2."""
    k = n // 4
    return np.concatenate([_uniform(rng, k), (F(CLUMP_AT) + F(0.05) * _uniform(rng, n - k)).astype(F)])


STRAYS_AT = np.array([30.0, 0.5, 0.5], F)


def _outliers(rng, n):
    """3,700 points uniform in the unit cube, 300 in a cube of edge 0.05 at x = 30 and 40 anywhere in [-40, 40]^3.  The 40
    coarsen the grid and lie beyond it, but spread over its border cells (4,000 uniform points plus these 40: the fullest
    border cell holds 6); the 300 -- 7 % of the points, so that mean + 3 sigma stays at 0.86 of their distance -- are binned
    from beyond the grid into ONE border cell, which a query next to them has to find through the clamps of the scan."""
    k = n * 40 // 4040
    m = n * 300 // 4040
    return np.concatenate([_uniform(rng, n - k - m), (STRAYS_AT + F(0.05) * _uniform(rng, m)).astype(F),
                           rng.uniform(-40, 40, size=(k, 3)).astype(F)])


def _heavy_tail(rng, n):
    return (rng.standard_cauchy(size=(n, 3)) * 0.1).astype(F)


def _far(rng, n):
    p = _uniform(rng, n)
    p[-1] = F([4000.0, -2500.0, 900.0])
    return p


class Scene:
    def __init__(self, name, make, n, radius, seed, regime, box=False):
        self.name, self.make, self.n, self.radius, self.seed, self.regime, self.box = name, make, n, radius, seed, regime, box

    def draw(self, n, seed):
        return self.make(np.random.default_rng(seed), n)


def _regime_div(lo, hi, dims):
    def check(h, occ, beyond):
        cpr = cells_per_radius(h)
        assert lo < cpr <= hi, f"radius * inv_cell = {cpr}"
        assert [int(v) for v in h["dims"]] == list(dims), h["dims"]
    return check


def _regime_coarse(h, occ, beyond):
    assert cells_per_radius(h) < 0.95 and int(h["ncells"]) <= h["table"]


def _regime_plane(h, occ, beyond):
    assert h["dims"][2] == 1 and h["dims"][0] > 1 and h["dims"][1] > 1


def _regime_line(h, occ, beyond):
    assert h["dims"][0] == 1 and h["dims"][2] == 1 and h["dims"][1] > 1


def _regime_same(h, occ, beyond):
    assert [int(v) for v in h["dims"]] == [1, 1, 1]


def _regime_clump(h, occ, beyond):
    assert occ.max() > WIN * 4 * 64, f"largest cell holds {occ.max()}"
    assert beyond.mean() >= 0.03, f"{beyond.mean():.4f} of the points beyond the grid"


def _regime_outliers(h, occ, beyond):
    assert cells_per_radius(h) < 0.95, "not coarsened"
    assert beyond.mean() > 0.005, f"{beyond.mean():.4f} of the points beyond the grid"
    assert occ[border_cells(h)].max() > 256, f"fullest border cell holds {occ[border_cells(h)].max()}"


def _regime_heavy_tail(h, occ, beyond):
    assert cells_per_radius(h) < 0.2, f"radius * inv_cell = {cells_per_radius(h)}"
    assert occ.max() > WIN * 4 * 64, f"largest cell holds {occ.max()}"


SCENES = {s.name: s for s in [
    Scene("div3", _div3, 4000, 0.2, 101, _regime_div(2.9, 3.0, (15, 15, 15)), box=True),
    Scene("div2", _div2, 4000, 0.12, 102, _regime_div(1.9, 2.0, (17, 17, 17)), box=True),
    Scene("div1", _div1, 4000, 0.05, 103, _regime_div(0.99, 1.0, (20, 20, 20)), box=True),
    Scene("coarse", _coarse, 4000, 0.02, 104, _regime_coarse, box=True),
    Scene("plane", _plane, 4000, 0.05, 105, _regime_plane, box=True),
    Scene("line", _line, 4000, 0.01, 106, _regime_line, box=True),
    Scene("same", _same, 300, 0.1, 107, _regime_same),
    Scene("clump", _clump, 4000, 0.11, 108, _regime_clump),
    Scene("outliers", _outliers, 4040, 0.1, 109, _regime_outliers),
    Scene("heavy_tail", _heavy_tail, 4000, 0.1, 110, _regime_heavy_tail),
    Scene("far", _far, 4001, 0.1, 102, None),
]}


@functools.lru_cache(maxsize=None)
def points(name):
    s = SCENES[name]
    p = np.ascontiguousarray(s.draw(s.n, s.seed), F)
    p.setflags(write=False)
    return p


def _rim_queries(pts, radius, want=4):
    """Queries at float32 distance EXACTLY R from a point along x (fl(q.x - p.x) == R, the other coordinates equal): on the rim
    of the inclusive test, so that a radius one ulp smaller loses the pair."""
    r, out = F(radius), []
    for p in pts[:400]:
        for sign in (1, -1):
            q = p.copy()
            q[0] = F(p[0] + F(sign) * r)
            if abs(F(p[0] - q[0])) == r:
                out.append(q)
                break
        if len(out) == want:
            break
    return np.array(out, F).reshape(-1, 3)


def _face_queries(rng, pts, header, radius):
    """Queries a few ulps either side of cell faces of the grid in ``header``, the other coordinates inside the points' box."""
    lo, hi = pts.min(0), pts.max(0)
    out = []
    for a in range(3):
        dim = int(header["dims"][a])
        if dim <= 1:
            continue
        cell = F(1) / header["inv_cell"][a]
        for k in sorted({0, 1, dim // 2, dim - 1, dim}):
            face = F(header["origin"][a] + F(k) * cell)
            for ulps in (-16, -3, -1, 0, 1, 3, 16):
                q = rng.uniform(lo, hi).astype(F)
                x = face
                for _ in range(abs(ulps)):
                    x = np.nextafter(x, F(np.inf) if ulps > 0 else F(-np.inf))
                q[a] = x
                out.append(q)
    return np.array(out, F).reshape(-1, 3)


def _header_key(header):
    return (header["origin"].tobytes(), header["inv_cell"].tobytes(), header["dims"].tobytes())


_QUERIES = {}


def queries(name, header=None):
    """The scene's queries: every fourth point; 500 points of the scene's own distribution; 64 up to 3 R outside the bounding
    box, on every side in turn; a few on the rim of a point's sphere; and, for the box scenes, queries a few ulps either side
    of cell faces of ``header`` (the host restatement's when None).  Read-only, one array per (scene, grid)."""
    s = SCENES[name]
    pts = points(name)
    header = host_header(pts, s.radius) if header is None else header
    key = (name,) + (_header_key(header) if s.box else ())
    if key not in _QUERIES:
        rng = np.random.default_rng(s.seed + 1000)
        parts = [pts[::4], s.draw(max(500, 48), s.seed + 2000)[-500:]]
        lo, hi = pts.min(0), pts.max(0)
        out = rng.uniform(lo, hi, size=(64, 3))
        for i in range(64):
            a, side = i % 3, (i // 3) % 2
            u = rng.uniform(0.02, 3.0) * s.radius
            out[i, a] = hi[a] + u if side else lo[a] - u
            if i >= 48:  # (the last ones beyond an edge or a corner)
                b = (a + 1) % 3
                out[i, b] = hi[b] + 0.5 * u if (i // 6) % 2 else lo[b] - 0.5 * u
        parts.append(out.astype(F))
        parts.append(_rim_queries(pts, s.radius))
        if s.box:
            parts.append(_face_queries(rng, pts, header, s.radius))
        q = np.ascontiguousarray(np.concatenate(parts), F)
        q.setflags(write=False)
        _QUERIES[key] = q
    return _QUERIES[key]


# ---- references ----------------------------------------------------------------------------------------------------------------

def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


_REF = {}


def _cached(key, make):
    if key not in _REF:
        _REF[key] = _frozen(*make())
    return _REF[key]


def reference(name, qs, ignore=False):
    """The float32 un-fused brute force at the scene's radius: (index, row_splits, d2), rows in ascending point index."""
    s = SCENES[name]
    return _cached((name, "l2", qs.tobytes(), ignore),
                   lambda: brute_force(points(name), qs, np.full(len(qs), s.radius, F), ignore))


def radii_for(name, m):
    """A radius per query from {0, R / 50, R / 7, R / 2, R}; every 29th a value just above R (the next float, 1.5 R, 3 R)."""
    r = F(SCENES[name].radius)
    rng = np.random.default_rng(SCENES[name].seed + 3000)
    radii = rng.choice(np.array([0, r / F(50), r / F(7), r / F(2), r], F), size=m).astype(F)
    above = np.array([np.nextafter(r, F(np.inf)), F(1.5) * r, F(3) * r], F)
    radii[::29] = above[np.arange(len(radii[::29])) % 3]
    radii.setflags(write=False)
    return radii


def reference_radii(name, qs, ignore=False):
    """The brute force with ``radii_for``; a radius above the structure's R gives an empty row."""
    r = F(SCENES[name].radius)

    def make():
        radii = radii_for(name, len(qs))
        idx, rs, d2 = brute_force(points(name), qs, np.where(radii <= r, radii, F(0)), ignore)
        keep = np.repeat(radii <= r, np.diff(rs))
        cnt = np.where(radii <= r, np.diff(rs), 0)
        return idx[keep], np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64), d2[keep]
    return _cached((name, "radii", qs.tobytes(), ignore), make)


def brute_force_linf(pts, qs, radius, ignore=False):
    """The max-norm set: |dx|, |dy|, |dz| <= R on float32 differences, inclusive.  -> (index int32, row_splits int64)."""
    pts, qs, r = np.asarray(pts, F), np.asarray(qs, F), F(radius)
    idx, cnt = [], []
    for q0 in range(0, len(qs), 256):
        d = pts[None, :, :] - qs[q0:q0 + 256, None, :]
        hit = np.all(np.abs(d) <= r, axis=2)
        if ignore:
            hit &= ~np.all(d == 0, axis=2)
        idx.append(np.nonzero(hit)[1].astype(np.int32))
        cnt.append(hit.sum(axis=1))
    rs = np.concatenate([[0], np.cumsum(np.concatenate(cnt))]).astype(np.int64) if cnt else np.zeros(1, np.int64)
    return (np.concatenate(idx) if idx else np.zeros(0, np.int32)), rs


def reference_linf(name, qs, ignore=False):
    return _cached((name, "linf", qs.tobytes(), ignore),
                   lambda: brute_force_linf(points(name), qs, SCENES[name].radius, ignore))


# ---- checkers ------------------------------------------------------------------------------------------------------------------

def canonical(idx, rs, *per_pair):
    row = np.repeat(np.arange(len(rs) - 1), np.diff(rs))
    order = np.lexsort((idx, row))
    return (np.asarray(idx)[order],) + tuple(np.asarray(p)[order] for p in per_pair)


def check_rows(tag, got, ref):
    """Row splits equal, index sets equal row by row and -- where both sides carry them -- squared distances bit for bit."""
    idx, rs = np.asarray(got[0]), np.asarray(got[1])
    assert np.array_equal(rs, ref[1]), f"{tag}: row lengths differ from the brute force"
    if len(got) > 2 and got[2] is not None and len(ref) > 2:
        a, da = canonical(idx, rs, np.asarray(got[2], F))
        b, db = canonical(ref[0], ref[1], ref[2])
        assert np.array_equal(a, b), f"{tag}: neighbour sets differ from the brute force"
        assert np.array_equal(da.view(np.uint32), db.view(np.uint32)), f"{tag}: squared distances are not bit-exact"
    else:
        assert np.array_equal(canonical(idx, rs)[0], canonical(ref[0], ref[1])[0]), f"{tag}: neighbour sets differ from the brute force"


def _window64(name, pts, qs, idx, rs, radius):
    """Per pair w in float64 (exact differences of the float32 positions; the radius the library sees, a float32)."""
    import torch
    row = np.repeat(np.arange(len(qs)), np.diff(rs))
    diff = np.asarray(pts, np.float64)[idx] - np.asarray(qs, np.float64)[row]
    d2 = (diff * diff).sum(1)
    r = float(F(radius))
    if name is None:
        return np.ones_like(d2), d2, row
    if name == "explicit":
        return d2, d2, row
    return dg.window(name, torch.from_numpy(d2 / (r * r))).numpy(), d2, row


def window_value32(name, d2, radius):
    """window_value of cconv_common.h as frs_window_sum calls it, in float32 numpy: inv_r2 = 1 / (R * R), q = d2 * inv_r2."""
    d2 = np.asarray(d2, F)
    if name is None:
        return np.ones_like(d2)
    if name == "explicit":
        return d2
    one, r = F(1), F(radius)
    q = d2 * (one / (r * r))
    if name == "poly6":
        t = one - q
        return np.minimum(np.maximum(t * t * t, F(0)), one)
    s = np.sqrt(q)
    u = one - s
    if name == "linear":
        return u
    if name == "peak":
        return one - F(2) * s + q
    k = F(4) / F(3)
    if name == "cubic":
        return k * np.where(q <= one, np.where(s <= F(0.5), F(6) * (s * s * s - q) + one, F(2) * u * u * u), F(0))
    if name == "cubic_grad":
        return k * np.where(q <= one, np.where(s <= F(0.5), F(18) * q - F(12) * s, F(-6) * u * u), F(0))
    raise NotImplementedError(name)


def window_sum_ref(name, window, qs, ignore=False):
    """-> (ref64 [m], A [m] = sum |w|, k [m] row lengths) of the scene's brute-force pair list."""
    def make():
        idx, rs, _ = reference(name, qs, ignore)
        w, _, row = _window64(window, points(name), qs, idx, rs, SCENES[name].radius)
        m = len(qs)
        return (np.bincount(row, weights=w, minlength=m), np.bincount(row, weights=np.abs(w), minlength=m),
                np.diff(rs).astype(np.float64))
    return _cached((name, "wsum", window, qs.tobytes(), ignore), make)


def window_bar(n, A, k, c_win=None):
    return ((math.ceil(n / 64) + 7) * A + (C_WIN if c_win is None else c_win) * k) * EPS


WORST = {}


def check_window_sum(tag, window, got, ref, A, k, n):
    """The element-wise bar of the module docstring; the count (window None) must equal the row length exactly.  Keeps the
    worst err / bar per window in WORST."""
    got = np.asarray(got, np.float64)
    if window is None:
        assert np.array_equal(got, k), f"{tag}: the count is not the row length"
        return
    err, bar = np.abs(got - ref), window_bar(n, A, k)
    assert np.all(np.isfinite(got)), f"{tag}: non-finite sums"
    ratio = np.where(bar > 0, err / np.where(bar > 0, bar, 1), np.where(err > 0, np.inf, 0))
    WORST[window] = max(WORST.get(window, 0.0), float(ratio.max()) if ratio.size else 0.0)
    i = int(np.argmax(ratio)) if ratio.size else 0
    assert ratio.size == 0 or ratio[i] <= 1, f"{tag}: row {i} misses the bar: err {err[i]:.3g}, bar {bar[i]:.3g} (k {k[i]:.0f}, A {A[i]:.3g})"


def measure_c_win(name):
    """The worst |w32 - w64| / 2^-24 of one term over every pair of the scene's list and every window."""
    qs = queries(name)
    idx, rs, d2 = reference(name, qs)
    worst = 0.0
    for window in WINDOWS:
        w64 = _window64(window, points(name), qs, idx, rs, SCENES[name].radius)[0]
        w32 = window_value32(window, d2, SCENES[name].radius).astype(np.float64)
        if w64.size:
            worst = max(worst, float(np.abs(w32 - w64).max()) / EPS)
    return worst
