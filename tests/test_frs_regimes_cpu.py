"""CPU side of the radius search's regime matrix (tests/frs_regimes.py, tests/test_gpu_frs_regimes.py): every scene reaches its
regime under the host restatement of the sizing, with room; the decoder reads back a structure packed by the restated layout
and trips when the layout drifts; C_WIN is the measured constant; and the checkers have teeth -- seeded faults of the reference
must fail them."""
import math

import numpy as np
import pytest

import frs_regimes as fg
from test_gpu_radius_search import brute_force

F = np.float32
REGIME_SCENES = [n for n, s in fg.SCENES.items() if s.regime is not None]


def _state(name):
    s = fg.SCENES[name]
    p = fg.points(name)
    h = fg.host_header(p, s.radius)
    cell, beyond, occ = fg.binning(p, h)
    return s, p, h, cell, beyond, occ


def test_scene_table():
    assert list(fg.SCENES) == ["div3", "div2", "div1", "coarse", "plane", "line", "same", "clump", "outliers", "heavy_tail", "far"]
    for name, s in fg.SCENES.items():
        p = fg.points(name)
        assert p.dtype == F and p.shape == (s.n, 3) and s.n <= 4040 and not p.flags.writeable
        assert fg.points(name) is p and np.array_equal(p, s.draw(s.n, s.seed)), "scenes are deterministic and built once"
    for name in ("div3", "div2", "div1", "coarse", "plane", "line"):
        p = fg.points(name)
        assert p.min() >= 0 and p.max() <= 1
    for name in ("div1", "coarse"):  # (the corners are pinned: the box is exact)
        assert np.array_equal(fg.points(name)[:8], fg.CORNERS)
    assert np.all(fg.points("plane")[:, 2] == 0) and np.all(fg.points("line")[:, [0, 2]] == 0)
    assert len(np.unique(fg.points("same"), axis=0)) == 1
    assert np.array_equal(fg.points("far")[:-1], fg.points("div2")) and fg.points("far")[-1].tolist() == [4000.0, -2500.0, 900.0]


@pytest.mark.parametrize("name", REGIME_SCENES)
def test_scene_reaches_its_regime_with_room(name):
    """The regime under the host restatement of frs_finish_header_one, and no comparison that chose it within 10 % of its
    threshold: a cell edge that was TAKEN passed both of its conditions with room; one that was rejected failed at least one of
    them with room (the other then decides nothing); the first "does the chosen cell fit the table" has room either way."""
    s, p, h, cell, beyond, occ = _state(name)
    s.regime(h, occ, beyond)
    dec = h["decisions"]
    edges, last = dec[:-1], dec[-1]
    assert last[0] == "the chosen cell fits the table" and len(edges) % 2 == 0

    def room(d):
        return d[1] <= 0.9 * d[2] if d[3] else d[1] >= 1.1 * d[2]

    for fits, dense in zip(edges[::2], edges[1::2]):
        if fits[3] and dense[3]:
            assert room(fits) and room(dense), (fits, dense)
        else:
            assert any(not d[3] and room(d) for d in (fits, dense)), (fits, dense)
    assert room(last), last
    assert (h["div"] == 0) == (not last[3])
    # the restated header is self-consistent the way the decoder demands of the device's
    assert int(np.prod(h["dims"].astype(np.int64))) == h["ncells"] <= h["table"] == fg.table_size(s.n)


def test_far_scene_header_is_printed_not_asserted():
    s, p, h, cell, beyond, occ = _state("far")
    print("far (host restatement):", {k: h[k] for k in ("origin", "inv_cell", "dims")}, "largest cell", occ.max())
    assert s.regime is None and h["ncells"] <= h["table"]


@pytest.mark.parametrize("name", [n for n in fg.SCENES if n != "same"])
def test_mean_row_length(name):
    rs = fg.reference(name, fg.queries(name))[1]
    assert np.diff(rs).mean() >= 8, np.diff(rs).mean()


def test_occupancies_and_beyond_grid_shares():
    """The stated cell occupancies and shares of points binned from beyond the grid, each with a tenth of room."""
    _, _, h, cell, beyond, occ = _state("clump")
    assert occ.max() >= 1.1 * 1024 and beyond.mean() >= 1.1 * 0.03, (occ.max(), beyond.mean())
    assert np.diff(fg.reference("clump", fg.queries("clump"))[1]).max() > fg.WIN * 4 * 64  # rows over more than kWin x 4 windows
    _, p, h, cell, beyond, occ = _state("outliers")
    border = fg.border_cells(h)
    full = int(np.argmax(np.where(border, occ, 0)))
    assert fg.cells_per_radius(h) <= 0.9 * 0.95 and beyond.mean() >= 1.1 * 0.005 and occ[full] >= 1.1 * 256
    assert beyond[cell == full].all(), "the fullest border cell holds strays only"
    _, _, h, cell, beyond, occ = _state("heavy_tail")
    assert fg.cells_per_radius(h) <= 0.9 * 0.2 and occ.max() >= 1.1 * 1024


@pytest.mark.parametrize("name", list(fg.SCENES))
def test_queries(name):
    s = fg.SCENES[name]
    p, q = fg.points(name), fg.queries(name)
    assert q.dtype == F and not q.flags.writeable and fg.queries(name) is q
    k = len(p[::4])
    assert np.array_equal(q[:k], p[::4])
    lo, hi = p.min(0), p.max(0)
    outside = q[k + 500:k + 564]
    off = np.maximum(lo - outside, outside - hi).max(1)
    assert np.all(off > 0) and np.all(off <= 3.0 * s.radius * 1.001)
    for a in range(3):  # every side
        assert np.any(outside[:, a] < lo[a]) and np.any(outside[:, a] > hi[a])
    if name != "same":
        rim = q[k + 564:k + 568]
        idx, rs, d2 = brute_force(p, rim, np.full(len(rim), s.radius, F))
        r2 = F(s.radius) * F(s.radius)
        assert len(rim) == 4 and all(np.any(d2[rs[i]:rs[i + 1]] == r2) for i in range(4)), "no pair exactly on the rim"
    if s.box:
        h = fg.host_header(p, s.radius)
        faces = q[k + 568:]
        c = fg.cell_coords(faces, h)
        assert len(faces) >= 25
        for a in range(3):
            if h["dims"][a] > 1:  # both sides of a face, and both ends of the grid
                assert {-1, 0, int(h["dims"][a]) - 1, int(h["dims"][a])} <= set(c[:, a].tolist())
        # another grid gives other face queries, the rest unchanged
        h2 = dict(h, origin=h["origin"] + F(0.01))
        q2 = fg.queries(name, h2)
        assert np.array_equal(q2[:k + 568], q[:k + 568]) and not np.array_equal(q2[k + 568:], faces)


def test_references():
    name = "div2"
    q = fg.queries(name)
    r = F(fg.SCENES[name].radius)
    idx, rs, d2 = fg.reference(name, q)
    assert fg.reference(name, q)[0] is idx and not idx.flags.writeable
    ign = fg.reference(name, q, True)
    self_hits = np.diff(rs) - np.diff(ign[1])
    assert np.all(self_hits[:1000] == 1) and np.all(self_hits >= 0)
    # a radius per query: rows above R are empty, rows at R those of the fixed search, rows at 0 the coincident points
    radii = fg.radii_for(name, len(q))
    ridx, rrs, rd2 = fg.reference_radii(name, q)
    cnt = np.diff(rrs)
    assert set(np.unique(radii[radii <= r]).tolist()) == {0.0, float(r / F(50)), float(r / F(7)), float(r / F(2)), float(r)}
    assert (radii > r).sum() >= 50 and np.nextafter(r, F(np.inf)) in radii and np.all(cnt[radii > r] == 0)
    assert np.array_equal(cnt[radii == r], np.diff(rs)[radii == r]) and np.all(cnt[:1000][radii[:1000] == 0] == 1)
    assert np.all(rd2 <= np.repeat(radii * radii, cnt))
    # the max-norm set holds the L2 set; the difference is what lies in the corners of the box
    lidx, lrs = fg.reference_linf(name, q)
    assert np.all(np.diff(lrs) >= np.diff(rs)) and lrs[-1] > 1.5 * rs[-1]
    row = np.repeat(np.arange(len(q)), np.diff(lrs))
    d = fg.points(name)[lidx] - q[row]
    assert np.all(np.abs(d).max(1) <= r)
    l2 = set(zip(np.repeat(np.arange(len(q)), np.diff(rs)).tolist(), idx.tolist()))
    assert l2 <= set(zip(row.tolist(), lidx.tolist()))


# ---- the decoder ---------------------------------------------------------------------------------------------------------------

def _f2ord(f):
    u = np.asarray(f, F).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def _pack(p, radius, h, extra=0):
    """The workspace of a structure over ``p`` as the restated layout and build lay it out."""
    n = len(p)
    L = fg.layout(n)
    buf = np.zeros(L["end"] + extra, np.uint8)
    head = np.zeros(128, np.uint8)
    head[0:12] = h["origin"].view(np.uint8)
    head[12:24] = h["inv_cell"].view(np.uint8)
    head[24:36] = h["dims"].view(np.uint8)
    head[36:40] = np.array([h["ncells"]], np.int32).view(np.uint8)
    bb_min, bb_max, s1, s2 = fg.box_sums(p)
    head[40:52] = _f2ord(bb_min).view(np.uint8)
    head[52:64] = _f2ord(bb_max).view(np.uint8)
    head[64:68] = np.array([radius], F).view(np.uint8)
    head[68:72] = np.array([n], np.int32).view(np.uint8)
    head[72:96] = s1.view(np.uint8)
    head[96:120] = s2.view(np.uint8)
    buf[:128] = head
    cell, _, occ = fg.binning(p, h)
    start = np.zeros(L["table"] + 1, np.uint32)
    start[1:len(occ) + 1] = np.cumsum(occ)
    start[len(occ) + 1:] = n
    buf[L["cell_start"]:L["cell_start"] + start.nbytes] = start.view(np.uint8)
    order = fg.expected_sort(p, h)
    s = np.zeros((n, 4), F)
    s[:, :3] = p[order]
    s[:, 3] = order.view(F)
    buf[L["sorted"]:L["sorted"] + s.nbytes] = s.reshape(-1).view(np.uint8)
    return buf, L


@pytest.mark.parametrize("name", ["div2", "outliers", "same"])
def test_decoder_round_trip_and_drift(name):
    s, p, h, cell, beyond, occ = _state(name)
    buf, L = _pack(p, s.radius, h)
    d = fg.decode_bytes(buf, s.n, s.radius, L["end"])
    for k in ("origin", "inv_cell", "dims", "sum", "sumsq", "bb_min", "bb_max"):
        ref = dict(zip(("bb_min", "bb_max", "sum", "sumsq"), fg.box_sums(p)))
        assert np.array_equal(d[k], h[k] if k in h else ref[k]), k
    assert d["ncells"] == h["ncells"] and d["table"] == fg.table_size(s.n)
    assert np.array_equal(d["cell_start"][:h["ncells"] + 1], np.concatenate([[0], np.cumsum(occ)]))
    assert np.array_equal(d["sorted_index"], fg.expected_sort(p, h))
    assert np.array_equal(d["sorted_xyz"].view(np.uint32), p[d["sorted_index"]].view(np.uint32))
    assert np.array_equal(np.sort(d["sorted_index"]), np.arange(s.n)) and np.all(np.diff(cell[d["sorted_index"]]) >= 0)
    # drift: a field inserted in front of dims, another radius, another point count, a workspace that ends early
    moved = buf.copy()
    moved[28:128] = buf[24:124]
    for bad in (lambda: fg.decode_bytes(moved, s.n, s.radius, L["end"]),
                lambda: fg.decode_bytes(buf, s.n, s.radius * 1.5, L["end"]),
                lambda: fg.decode_bytes(buf, s.n + 1, s.radius, L["end"] + 4096),
                lambda: fg.decode_bytes(buf, s.n, s.radius, L["sorted"] + 16 * s.n - 16)):
        with pytest.raises(AssertionError):
            bad()


def test_layout_is_frs_layout():
    """The restated layout against the library's own size: dmcf_frs_workspace_bytes(n, 0) is the end of ``sorted`` plus the
    blocks that follow it (one count, the scan scratch, one flag byte: 256 bytes each at these sizes)."""
    from dmcf_amd import _lib
    L = _lib.lib()
    for n in (0, 1, 300, 4000, 4040, 16384, 100000):
        end = fg.layout(n)["end"]
        total = L.dmcf_frs_workspace_bytes(n, 0)
        scan = fg._up((-(-(fg.table_size(n) + 1) // 2048) + 1) * 8)
        assert total == end + 256 + scan + 256, (n, end, total)


# ---- C_WIN ---------------------------------------------------------------------------------------------------------------------

def test_c_win_is_the_measured_constant():
    """C_WIN = 4 x the worst |w32 - w64| / 2^-24 of one term (float32 un-fused d^2, inv_r2 = 1 / (R * R), the formulas of
    window_value, against float64) over every pair of every scene and every window, rounded up to a power of two."""
    per_scene = {name: fg.measure_c_win(name) for name in fg.SCENES}
    worst = max(per_scene.values())
    print("measured c_win per scene", {k: round(v, 2) for k, v in per_scene.items()})
    print(f"measured c_win {worst:.4g}; recorded {fg.MEASURED_C_WIN:.4g}; C_WIN = {fg.C_WIN:.4g} = 2^{math.log2(fg.C_WIN):.0f}")
    assert 0.5 * fg.MEASURED_C_WIN <= worst <= fg.MEASURED_C_WIN, "the recorded measurement is stale"
    assert fg.C_WIN == 2.0 ** math.ceil(math.log2(4 * fg.MEASURED_C_WIN))


def test_float32_window_sum_is_within_the_bar():
    """The float32 restatement of frs_window_sum's terms, added in float32 in ascending point index, passes the checker that
    the GPU has to pass; the count is exact."""
    name = "div2"
    q, n = fg.queries(name), fg.SCENES[name].n
    idx, rs, d2 = fg.reference(name, q)
    for window in fg.WINDOWS + [None]:
        w = fg.window_value32(window, d2, fg.SCENES[name].radius)
        got = np.array([w[rs[i]:rs[i + 1]].sum(dtype=F) for i in range(len(q))], F)
        fg.check_window_sum(f"float32 {window}", window, got, *fg.window_sum_ref(name, window, q), n)


# ---- teeth ---------------------------------------------------------------------------------------------------------------------

def _drop(ref, row, pos):
    idx, rs, d2 = ref
    at = int(rs[row]) + pos
    rs2 = rs.copy()
    rs2[row + 1:] -= 1
    return np.delete(idx, at), rs2, np.delete(d2, at)


def _fails(fn, *a):
    with pytest.raises(AssertionError):
        fn(*a)


def test_row_checker_has_teeth():
    name = "clump"
    q = fg.queries(name)
    ref = fg.reference(name, q)
    fg.check_rows("self", ref, ref)
    # one pair dropped from a long row
    long_row = int(np.argmax(np.diff(ref[1])))
    assert np.diff(ref[1])[long_row] > 1024
    _fails(fg.check_rows, "long row", _drop(ref, long_row, 1500), ref)
    # ... and the same with the row length kept (another point's index in its place): the sets differ
    idx = ref[0].copy()
    idx[ref[1][long_row] + 1500] = idx[ref[1][long_row] + 1499]
    _fails(fg.check_rows, "long row, length kept", (idx, ref[1], ref[2]), ref)
    # one pair of a point binned from beyond the grid (it lives in a border cell) dropped
    _, p, h, cell, beyond, occ = _state(name)
    pair = int(np.nonzero(beyond[ref[0]])[0][0])
    row = int(np.searchsorted(ref[1], pair, side="right") - 1)
    _fails(fg.check_rows, "border cell", _drop(ref, row, pair - int(ref[1][row])), ref)
    # a squared distance one ulp off
    d2 = ref[2].copy()
    d2[pair] = np.nextafter(d2[pair], F(1))
    _fails(fg.check_rows, "distance", (ref[0], ref[1], d2), ref)
    # a radius one ulp smaller: the pairs on the rim (fl(q.x - p.x) == R exactly) are lost
    for scene in ("div3", "clump", "heavy_tail"):
        s, qs = fg.SCENES[scene], fg.queries(scene)
        smaller = brute_force(fg.points(scene), qs, np.full(len(qs), np.nextafter(F(s.radius), F(0)), F))
        _fails(fg.check_rows, "radius", smaller, fg.reference(scene, qs))
    # the max-norm and per-query-radius references go through the same checker
    lin = fg.reference_linf("div2", fg.queries("div2"))
    _fails(fg.check_rows, "linf", (np.delete(lin[0], 7), np.concatenate([lin[1][:1], lin[1][1:] - 1])), lin)


def _one_neighbour_case():
    """300 points in [0, 100]^3, R = 10, queries 9 away from a point: rows of ONE term with d^2 = 81 or so.  n <= 512 makes the
    summation part of the bar (ceil(n / 64) + 7 = 12) smaller than 16, and d^2 > 32 lifts a term of the "explicit" window above
    the absolute part C_WIN * 2^-24: the one place where the bar resolves a relative fault of 2^-20 in one term."""
    rng = np.random.default_rng(7)
    p = rng.uniform(0, 100, size=(300, 3)).astype(F)
    q = (p + F([9, 0, 0])).astype(F)
    idx, rs, d2 = brute_force(p, q, np.full(300, 10, F))
    return p, q, idx, rs, d2


def test_window_sum_checker_has_teeth():
    name = "div2"
    q, n, radius = fg.queries(name), fg.SCENES[name].n, fg.SCENES[name].radius
    idx, rs, d2 = fg.reference(name, q)
    for window in fg.WINDOWS + [None]:
        ref, A, k = fg.window_sum_ref(name, window, q)
        fg.check_window_sum("self", window, ref.astype(F), ref, A, k, n)
    # one row's sum missing its smallest term
    for window in ("linear", "peak", "cubic", None):
        ref, A, k = fg.window_sum_ref(name, window, q)
        w = fg._window64(window, fg.points(name), q, idx, rs, radius)[0]
        bar = fg.window_bar(n, A, k)
        rows = [i for i in range(len(q)) if rs[i + 1] - rs[i] >= 20 and np.abs(w[rs[i]:rs[i + 1]]).min() > 2 * bar[i]]
        assert rows, window
        got = ref.copy()
        got[rows[0]] -= w[rs[rows[0]]:rs[rows[0] + 1]][np.argmin(np.abs(w[rs[rows[0]]:rs[rows[0] + 1]]))]
        _fails(fg.check_window_sum, "smallest term", window, got, ref, A, k, n)
    # a count that is off by one, a NaN
    ref, A, k = fg.window_sum_ref(name, None, q)
    _fails(fg.check_window_sum, "count", None, ref + (np.arange(len(q)) == 5), ref, A, k, n)
    ref, A, k = fg.window_sum_ref(name, "poly6", q)
    _fails(fg.check_window_sum, "nan", "poly6", np.where(np.arange(len(q)) == 5, np.nan, ref), ref, A, k, n)
    # one term's window evaluated at q * (1 + 2^-20)
    p1, q1, idx1, rs1, d21 = _one_neighbour_case()
    w = fg._window64("explicit", p1, q1, idx1, rs1, 10.0)[0]
    row = np.repeat(np.arange(300), np.diff(rs1))
    ref = np.bincount(row, weights=w, minlength=300)
    A, k = np.bincount(row, weights=np.abs(w), minlength=300), np.diff(rs1).astype(np.float64)
    fg.check_window_sum("self", "explicit", ref, ref, A, k, 300)
    single = [i for i in range(300) if k[i] == 1 and ref[i] > 64]
    assert single
    got = ref.copy()
    got[single[0]] = ref[single[0]] * (1 + 2.0 ** -20)
    _fails(fg.check_window_sum, "q * (1 + 2^-20)", "explicit", got, ref, A, k, 300)


def test_what_the_window_bar_cannot_see():
    """The same fault -- one term at q * (1 + 2^-20) -- on the scenes of the matrix (n = 4,000, R <= 0.2) stays INSIDE the bar,
    for every window and every term: it moves a term by at most 16 |q w'(q)| <= 32 units of 2^-24 (cubic_grad at q = 1 / 4), and
    the bar grants every term C_WIN = 128 of them, four times the float32 formula's own measured error.  Written down so that
    nobody reads the tooth above as more than it is; what the bar does see at these sizes are the faults of the other teeth."""
    name = "div3"
    q, n, radius = fg.queries(name), fg.SCENES[name].n, fg.SCENES[name].radius
    idx, rs, d2 = fg.reference(name, q)
    import torch
    r = float(F(radius))
    row = np.repeat(np.arange(len(q)), np.diff(rs))
    for window in fg.WINDOWS:
        ref, A, k = fg.window_sum_ref(name, window, q)
        w, d64, _ = fg._window64(window, fg.points(name), q, idx, rs, radius)
        q64 = d64 / (r * r) * (1 + 2.0 ** -20)
        moved = q64 * r * r if window == "explicit" else fg.dg.window(window, torch.from_numpy(q64)).numpy()
        shift = np.abs(moved - w)
        assert shift.max() <= 33 * fg.EPS
        assert np.all(shift <= fg.window_bar(n, A, k)[row])
