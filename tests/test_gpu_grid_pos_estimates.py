"""grid_pos on the cell tables a rollout sizes from its last step: ops._grid_count_levels with the estimates of ``_GRID_CELLS``
on the device, un-batched and with row splits, the C ABI on tables and outputs smaller than the header says, and both entry-point
families on a workspace of exactly the reported size (they share one layout).

Every comparison is bit for bit against ``oracle.grid_pos`` (numpy) on the positions of that call -- per item and concatenated
for a batch -- never against a second run of the product.  Every step asserts how many count passes it made: the number says
which branch of the table sizing the step took (2 = one per level, no recount).

Scenes: n uniform points in an origin-centred cube of edge E, the second half the mirror image of the first, so the mean is
the centre and a box is as wide as its edge allows: at voxel 0.1, hyst 0.1, pad 0 an edge of 1 / 4 / 4.3 / 6.5 gives
13^3 = 2197 / 43^3 = 79507 / 45^3 = 91125 / 67^3 = 300763 cells.  (10 E + 3 cells per axis, 97336 and 314432 for the two
larger cubes, need a box that straddles a voxel boundary on both sides, which a centred cube of these edges does not; the
transitions are the same: 91125 fits the estimate 131072 that a step of 79507 cells leaves behind, 300763 does not.)  The
second level, voxel 0.2, stays under the smallest size class, 65536 entries, in every dense step.

One stray particle at +4000 on every axis makes BOTH levels sparse (6.4e13 and 8e12 cells against GRID_MIN_CELLS = 2^22): that
step recounts both levels, four count passes."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIZES3 = [[0.1, 0.1, 0.1], [0.2, 0.2, 0.2]]
SIZES2 = [[0.1, 0.1, 0.0], [0.2, 0.2, 0.0]]
PLAIN = dict(centralize=True, pad=0, hyst=0.1, center=None)


def cube(edge, n=3000, seed=0, flat=False, at=(0.0, 0.0, 0.0)):
    """n uniform points of a cube of edge ``edge`` around ``at``, the second half mirrored.  No coordinate is closer than
    2^-10 edges to a centre plane: the double sums of the mean are then exact in any order, and the device's centre is numpy's."""
    u = np.random.RandomState(seed).uniform(-0.5, 0.5, size=(n // 2, 3))
    u = np.where(np.abs(u) < 2.0 ** -10, 2.0 ** -10, u)
    half = (u * edge).astype(np.float32)
    p = np.concatenate([half, -half])
    if flat:
        p[:, 2] = 0.0
    return (p + np.float32(at)).astype(np.float32)


def with_stray(p, flat=False):
    return np.concatenate([p, np.float32([[4000.0, 4000.0, 0.0 if flat else 4000.0]])])


def _cells(points, voxel, origin):
    """Integer cells of lattice points ``float(cell) * voxel + origin`` (collapsed axes: cell 0)."""
    active = voxel >= 1e-5
    g = np.rint((points.astype(np.float64) - origin.astype(np.float64)) / np.where(active, voxel, 1.0).astype(np.float64))
    return np.where(active, g, 0.0).astype(np.int64)


def reference(oracle, p, voxel, o):
    """oracle.grid_pos on ``p`` -> (points, (minp, dims) | None, cells): the box is the one the oracle's points span, which
    is the box of its candidates (every candidate cell is a lattice point).  A given centre c is not an argument of the oracle:
    the cells are the oracle's for p - c without centring, the points float(cell) * voxel + c as losses.py:178 forms them."""
    voxel = np.asarray(voxel, dtype=np.float32)
    if p.shape[0] == 0:
        return np.zeros((0, 3), dtype=np.float32), None, 0
    if o["center"] is not None:
        c = np.float32(o["center"])
        raw = oracle.grid_pos((p - c).astype(np.float32), voxel, centralize=False, pad=o["pad"], hyst=o["hyst"])
        g = _cells(raw, voxel, voxel / np.float32(2))
        ref = (g.astype(np.float32) * voxel + c).astype(np.float32)
    else:
        ref = oracle.grid_pos(p, voxel, centralize=o["centralize"], pad=o["pad"], hyst=o["hyst"])
        origin = p.mean(axis=0, dtype=np.float64).astype(np.float32) if o["centralize"] else voxel / np.float32(2)
        g = _cells(ref, voxel, origin)
    minp = g.min(axis=0)
    dims = g.max(axis=0) - minp + 1
    return ref, (minp.tolist(), dims.tolist()), int(np.prod(dims))


def same_bits(got, ref):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    return got.shape == ref.shape and got.dtype == ref.dtype and np.array_equal(got.view(np.uint32), ref.view(np.uint32))


class _Counting:
    """The library with a counter on every entry point called (as in tests/test_gpu_step_batched.py)."""

    def __init__(self, real):
        self._real, self.calls = real, {}

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("dmcf_"):
            return fn

        def counted(*a):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*a)
        return counted


@pytest.fixture
def grid(monkeypatch):
    from dmcf_amd import ops, _lib
    monkeypatch.setattr(ops, "_GRID_CELLS", {})
    counting = _Counting(_lib.lib())
    monkeypatch.setattr(_lib, "lib", lambda: counting)
    return ops, counting


def _entry(ops):
    assert len(ops._GRID_CELLS) == 1, "every call of a sequence runs under the same key"
    return next(iter(ops._GRID_CELLS.values()))


def call(grid, oracle, p, o, sizes, counts, tag):
    """One grid_pos_many call: every level equals the oracle in points and box, ``counts`` count passes were made, and the
    entry left behind holds the cells of the oracle's boxes (-1: sparse).  -> (cells per level, sparse per level)."""
    ops, counting = grid
    counting.calls.clear()
    center = None if o["center"] is None else torch.tensor(o["center"], dtype=torch.float32, device=DEV)
    res = ops.grid_pos_many(torch.from_numpy(p).to(DEV), [np.float32(v) for v in sizes], centralize=o["centralize"], pad=o["pad"],
                            hyst=o["hyst"], center=center)
    refs = [reference(oracle, p, v, o) for v in sizes]
    assert len(res) == len(sizes)
    for level, ((got, box), (ref, rbox, _)) in enumerate(zip(res, refs)):
        assert same_bits(got, ref), (tag, level, tuple(got.shape), ref.shape)
        assert box == rbox, (tag, level, box, rbox)
    made = counting.calls.get("dmcf_grid_pos_count", 0)
    print(f"{tag}: n {p.shape[0]}, cells {[r[2] for r in refs]}, points {[r[0].shape[0] for r in refs]}, count passes {made}")
    assert made == counts and counting.calls.get("dmcf_grid_pos_count_batched", 0) == 0, (tag, made, counts)
    cells = [r[2] for r in refs]
    sparse = [ops._grid_too_sparse(c, p.shape[0]) for c in cells]
    assert _entry(ops) == [-1 if s else c for c, s in zip(cells, sparse)], (tag, _entry(ops), cells)
    return cells, sparse


def rollout(grid, oracle, o, sizes, edges, flat=False):
    """Steps 1 to 8: grow within the estimate, outgrow it, shrink, lose one particle to infinity, get it back."""
    ops, _ = grid
    e1, e2, e3, small = edges
    est = lambda c: ops._size_class(c + c // 4)  # noqa: E731  (the table a level gets after a call with c cells)
    c1, _ = call(grid, oracle, cube(e1, seed=1, flat=flat), o, sizes, 2, "1 first call")
    c2, _ = call(grid, oracle, cube(e2, seed=2, flat=flat), o, sizes, 2, "2 estimate holds")
    assert c1[0] > 65536 and c1[0] < c2[0] <= est(c1[0]) and c2[1] <= est(c1[1]), "step 2 must fit a table above the smallest class"
    c3, _ = call(grid, oracle, cube(e3, seed=3, flat=flat), o, sizes, 3, "3 outgrown")
    assert c3[0] > est(c2[0]) and c3[1] <= est(c2[1]) == 65536, "step 3 must outgrow level 0's table and only that"
    c4, _ = call(grid, oracle, cube(small, seed=4, flat=flat), o, sizes, 2, "4 table far too big")
    assert 64 * c4[0] < est(c3[0])
    stray = with_stray(cube(small, seed=5, flat=flat), flat)
    c5, s5 = call(grid, oracle, stray, o, sizes, 4, "5 dense -> hashed")
    assert s5 == [True, True] and c5[0] > 100 * ops.GRID_MIN_CELLS and _entry(ops) == [-1, -1]
    call(grid, oracle, stray, o, sizes, 2, "6 hashed from the start")
    assert _entry(ops) == [-1, -1]
    back = cube(small, seed=7, flat=flat)
    c7, s7 = call(grid, oracle, back, o, sizes, 2, "7 runs hashed, is dense")
    assert s7 == [False, False] and _entry(ops) == c7 and c7[0] < 65536
    call(grid, oracle, back, o, sizes, 2, "8 dense again")
    return c1, c7


def test_rollout_sequence(grid, oracle):
    """A1: steps 1 to 8, then another point count under the same key, an empty call and a full one after it."""
    ops, _ = grid
    c1, c7 = rollout(grid, oracle, PLAIN, SIZES3, (4.0, 4.3, 6.5, 1.0))
    assert c1 == [79507, 23 ** 3] and c7 == [2197, 7 ** 3]
    assert ops._size_class(79507 + 79507 // 4) == 131072
    call(grid, oracle, cube(1.0, n=40, seed=9), PLAIN, SIZES3, 2, "9 forty points")
    c10, _ = call(grid, oracle, cube(6.5, n=20000, seed=10), PLAIN, SIZES3, 3, "10 twenty thousand points")
    assert c10[0] == 67 ** 3 and c10[1] <= 65536
    counting = grid[1]
    counting.calls.clear()
    res = ops.grid_pos_many(torch.zeros((0, 3), device=DEV), [np.float32(v) for v in SIZES3], centralize=True)
    assert [tuple(pts.shape) for pts, _ in res] == [(0, 3), (0, 3)] and [box for _, box in res] == [None, None]
    assert counting.calls.get("dmcf_grid_pos_count", 0) == 2 and _entry(ops) == [0, 0]
    c12, _ = call(grid, oracle, cube(4.0, seed=12), PLAIN, SIZES3, 3, "12 full after empty")
    assert c12[0] == 79507 > ops._size_class(0) >= c12[1]


@pytest.mark.parametrize("name", ["not_centralized", "pad1_hyst02", "flat", "given_center"])
def test_rollout_sequence_options(grid, oracle, name):
    """A2: steps 1 to 8 with other options.  The 2-D form needs edges of 26, 27 and 50 to pass 65536 cells and outgrow 131072
    while its second level (at most 253^2 = 64009 cells at edge 50) stays within 65536."""
    o, sizes, edges, flat = {
        "not_centralized": (dict(PLAIN, centralize=False), SIZES3, (4.0, 4.3, 6.5, 1.0), False),
        "pad1_hyst02": (dict(PLAIN, pad=1, hyst=0.2), SIZES3, (4.0, 4.3, 6.5, 1.0), False),
        "flat": (PLAIN, SIZES2, (26.0, 27.0, 50.0, 1.0), True),
        "given_center": (dict(PLAIN, center=[0.013, -0.027, 0.041]), SIZES3, (4.0, 4.3, 6.5, 1.0), False),
    }[name]
    rollout(grid, oracle, o, sizes, edges, flat=flat)


# ---- A3: the batched form -----------------------------------------------------------------------------------------------------------

def call_batched(grid, oracle, items, counts, sparse, tag):
    """One call with row splits over ``items``: points and all three forms of the output row splits equal the oracle per item.
    -> (the device's points per level and item, cells per level and item)."""
    ops, counting = grid
    counting.calls.clear()
    rs = [0]
    for it in items:
        rs.append(rs[-1] + it.shape[0])
    res = ops.grid_pos_many(torch.from_numpy(np.concatenate(items)).to(DEV), [np.float32(v) for v in SIZES3], centralize=True,
                            row_splits=rs)
    out, cells = [], []
    for level, (got, splits) in enumerate(res):
        refs = [reference(oracle, it, SIZES3[level], PLAIN) for it in items]
        host = [0]
        for r in refs:
            host.append(host[-1] + r[0].shape[0])
        assert splits.host == tuple(host), (tag, level, splits.host, host)
        assert splits.dev.dtype == torch.int64 and splits.dev.tolist() == host, (tag, level)
        assert splits.sparse is sparse, (tag, level)
        assert got.shape == (host[-1], 3)
        for b, r in enumerate(refs):
            assert same_bits(got[host[b]:host[b + 1]], r[0]), (tag, level, b)
        out.append([got[host[b]:host[b + 1]].cpu().numpy() for b in range(len(items))])
        cells.append([r[2] for r in refs])
    made = counting.calls.get("dmcf_grid_pos_count_batched", 0)
    print(f"{tag}: cells per item {cells}, count passes {made}")
    assert made == counts and counting.calls.get("dmcf_grid_pos_count", 0) == 0, (tag, made, counts)
    n = sum(it.shape[0] for it in items)
    assert _entry(ops) == [-1 if ops._grid_too_sparse(sum(c), n) else sum(c) for c in cells], (tag, _entry(ops), cells)
    return out, cells


def batch_items(item0):
    """Item 1 has the coordinates item 0 starts with (items share no cell), item 2 is empty, item 3 a small cube elsewhere."""
    return [item0, cube(4.0, seed=1), np.zeros((0, 3), dtype=np.float32), cube(1.0, n=500, seed=8, at=(7.0, -3.0, 2.0))]


def test_batched_sequence(grid, oracle):
    ops, _ = grid
    est = lambda c: ops._size_class(c + c // 4)  # noqa: E731
    o1, c1 = call_batched(grid, oracle, batch_items(cube(4.0, seed=1)), 2, False, "1 first call")
    assert c1[0][0] == c1[0][1] == 79507 and c1[0][2] == 0
    _, c2 = call_batched(grid, oracle, batch_items(cube(4.3, seed=2)), 2, False, "2 estimate holds")
    assert sum(c1[0]) < sum(c2[0]) <= est(sum(c1[0]))
    o3, c3 = call_batched(grid, oracle, batch_items(cube(6.5, seed=3)), 3, False, "3 outgrown")
    # item 0 alone is larger than the table of the first count pass: the cells of items 1 and 3 start past its end
    assert c3[0][0] > est(sum(c2[0])) and sum(c3[1]) <= est(sum(c2[1])) == 65536
    for level in range(2):
        for b in (1, 3):
            assert same_bits(o3[level][b], o1[level][b]), (level, b)
    stray = with_stray(cube(1.0, seed=5))
    call_batched(grid, oracle, batch_items(stray), 4, True, "5 dense -> hashed")
    assert _entry(ops) == [-1, -1]
    call_batched(grid, oracle, batch_items(stray), 2, True, "6 hashed from the start")
    items = batch_items(cube(1.0, seed=7))
    _, c7 = call_batched(grid, oracle, items, 2, True, "7 runs hashed, is dense")
    assert _entry(ops) == [sum(c7[0]), sum(c7[1])]
    # the key holds the batch size only: items 0 and 3 exchange their points, the total stays
    swapped = [items[3], items[1], items[2], items[0]]
    o8, c8 = call_batched(grid, oracle, swapped, 2, False, "8 items 0 and 3 exchanged")
    assert [c8[0][3], c8[0][0]] == [c7[0][0], c7[0][3]] and o8[0][0].shape[0] < o8[0][3].shape[0]


# ---- A4: the C ABI on buffers smaller than the header says, between guard words ----------------------------------------------------

G = 4096
WORD = 0x5A5A5A5A
FSENT = -1.2345e30


class _Abi:
    """The three phases of one level through the library itself, un-batched or over ``items``."""

    def __init__(self, items, batched):
        import ctypes
        from dmcf_amd import ops, _lib
        self.L, self.stream, self.batched = _lib.lib(), ops._stream, batched
        self.items = items
        self.pos = torch.from_numpy(np.concatenate(items)).to(DEV)
        self.n, self.batch = self.pos.shape[0], len(items)
        rs = [0]
        for it in items:
            rs.append(rs[-1] + it.shape[0])
        self.rs = torch.tensor(rs, dtype=torch.int64, device=DEV)
        self.vs = (ctypes.c_float * 3)(0.1, 0.1, 0.1)
        self.nb = (self.L.dmcf_grid_pos_workspace_bytes_batched(self.n, self.batch) if batched
                   else self.L.dmcf_grid_pos_workspace_bytes(self.n))
        self.ws = torch.zeros(self.nb, dtype=torch.uint8, device=DEV)
        assert self.nb > 0 and self.ws.data_ptr() % 256 == 0
        # the output row splits between guards of their own (batched form)
        self.ors = torch.full((G + self.batch + 1 + G,), WORD, dtype=torch.int64, device=DEV)

    def reference(self, oracle):
        refs = [reference(oracle, it, [0.1] * 3, PLAIN) for it in self.items]
        host = [0]
        for r in refs:
            host.append(host[-1] + r[0].shape[0])
        return np.concatenate([r[0] for r in refs]), host, sum(r[2] for r in refs)

    def bounds(self):
        p, w = self.pos.data_ptr(), self.ws.data_ptr()
        if self.batched:
            rc = self.L.dmcf_grid_pos_bounds_batched(p, self.n, self.rs.data_ptr(), self.batch, self.vs, 1, None, 0, 0.1, w, self.nb,
                                                     self.stream())
        else:
            rc = self.L.dmcf_grid_pos_bounds(p, self.n, self.vs, 1, None, 0, 0.1, w, self.nb, self.stream())
        assert rc == 0, rc

    def count(self, table_ptr, table_cells):
        p, w = self.pos.data_ptr(), self.ws.data_ptr()
        if self.batched:
            rc = self.L.dmcf_grid_pos_count_batched(p, self.n, self.rs.data_ptr(), self.batch, self.vs, 1, 0, 0.1, w, self.nb, table_ptr,
                                                    table_cells, self.ors.data_ptr() + 8 * G, self.stream())
        else:
            rc = self.L.dmcf_grid_pos_count(p, self.n, self.vs, 1, 0, 0.1, w, self.nb, table_ptr, table_cells, self.stream())
        torch.cuda.synchronize()
        assert rc == 0, rc  # DMCF_OK

    def write(self, table_ptr, table_cells, out_ptr, out_capacity):
        p, w = self.pos.data_ptr(), self.ws.data_ptr()
        if self.batched:
            rc = self.L.dmcf_grid_pos_write_batched(p, self.n, self.rs.data_ptr(), self.batch, self.vs, 1, 0, 0.1, w, self.nb, table_ptr,
                                                    table_cells, out_ptr, out_capacity, self.stream())
        else:
            rc = self.L.dmcf_grid_pos_write(p, self.n, self.vs, 1, 0, 0.1, w, self.nb, table_ptr, table_cells, out_ptr, out_capacity,
                                            self.stream())
        torch.cuda.synchronize()
        assert rc == 0, rc

    def header(self):
        """-> (cells, total) of the call as the device reports them"""
        h = self.ws[:64 * (self.batch if self.batched else 1)].cpu().view(torch.int64).reshape(-1, 8)
        return int(h[:, 3].sum()), int(h[:, 4].sum())

    def row_splits_ok(self, host=None):
        o = self.ors.cpu()
        guards = bool((o[:G] == WORD).all()) and bool((o[G + self.batch + 1:] == WORD).all())
        return guards and (host is None or o[G:G + self.batch + 1].tolist() == host)


def _abi_forms():
    return {"one": ([cube(6.5, seed=3)], False), "batched": (batch_items(cube(4.0, seed=1)), True)}


def _guarded_out(abi, table_ptr, table_cells, ref, capacity):
    """The write pass into ``capacity`` rows between guards: the first rows of the oracle, and nothing else is touched.  The
    words behind the rows would hold the whole result: a write past the capacity lands in them, not outside the tensor."""
    buf = torch.full((G + 3 * ref.shape[0] + G,), FSENT, dtype=torch.float32, device=DEV)
    abi.write(table_ptr, table_cells, buf.data_ptr() + 4 * G, capacity)
    host = buf.cpu().numpy()
    assert same_bits(host[G:G + 3 * capacity].reshape(-1, 3), ref[:capacity])
    rest = np.concatenate([host[:G], host[G + 3 * capacity:]])
    assert rest.size >= 2 * G and same_bits(rest, np.full(rest.shape, FSENT, dtype=np.float32))


@pytest.mark.parametrize("form", ["one", "batched"])
def test_abi_dense_table_smaller_than_the_header_says(oracle, form, monkeypatch):
    """The second read_headers() of the estimate path relies on this: a count pass on a table of fewer cells than the box has
    returns DMCF_OK, writes no word outside the table and leaves the header's cells alone.  The tensor behind the table is as
    long as the box: EVERY word outside [0, table_cells) is compared, the G words on either side included."""
    from dmcf_amd import ops
    monkeypatch.setattr(ops, "_GRID_CELLS", {})
    items, batched = _abi_forms()[form]
    abi = _Abi(items, batched)
    ref, host, cells = abi.reference(oracle)
    abi.bounds()
    torch.cuda.synchronize()
    assert abi.header()[0] == cells
    big = torch.empty(G + cells + G, dtype=torch.int32, device=DEV)
    for table_cells in (cells // 3, cells - 1):
        big.fill_(WORD)
        abi.ors.fill_(WORD)
        abi.count(big.data_ptr() + 4 * G, table_cells)
        words = big.cpu()
        assert bool((words[:G] == WORD).all()) and bool((words[G + table_cells:] == WORD).all()), table_cells
        assert bool((words[G:G + table_cells] != WORD).all()), "the table itself is initialised"
        got_cells, total = abi.header()
        assert got_cells == cells and 0 < total <= ref.shape[0], (table_cells, got_cells, total)
        assert abi.row_splits_ok()
    big.fill_(WORD)
    abi.count(big.data_ptr() + 4 * G, cells)
    words = big.cpu()
    assert bool((words[:G] == WORD).all()) and bool((words[G + cells:] == WORD).all())
    assert abi.header() == (cells, ref.shape[0])
    assert abi.row_splits_ok(host if batched else None)
    _guarded_out(abi, big.data_ptr() + 4 * G, cells, ref, ref.shape[0])
    _guarded_out(abi, big.data_ptr() + 4 * G, cells, ref, ref.shape[0] // 2)
    words = big.cpu()
    assert bool((words[:G] == WORD).all()) and bool((words[G + cells:] == WORD).all())


@pytest.mark.parametrize("form", ["one", "batched"])
def test_abi_hashed_table_of_the_right_size(oracle, form, monkeypatch):
    """table_cells = -slots: 12 bytes per slot (a rank and a 64-bit key), guards behind them."""
    from dmcf_amd import ops
    monkeypatch.setattr(ops, "_GRID_CELLS", {})
    items, batched = _abi_forms()[form]
    abi = _Abi(items, batched)
    ref, host, cells = abi.reference(oracle)
    slots = ops._grid_hash_slots(abi.n, [0.1] * 3, 0)
    assert slots >= 2 * 2 * abi.n * 8 and slots & (slots - 1) == 0
    abi.bounds()
    big = torch.full((G + 3 * slots + G,), WORD, dtype=torch.int32, device=DEV)
    abi.count(big.data_ptr() + 4 * G, -slots)
    assert abi.header() == (cells, ref.shape[0])
    assert abi.row_splits_ok(host if batched else None)
    _guarded_out(abi, big.data_ptr() + 4 * G, -slots, ref, ref.shape[0])
    _guarded_out(abi, big.data_ptr() + 4 * G, -slots, ref, ref.shape[0] // 2)
    words = big.cpu()
    assert bool((words[:G] == WORD).all()) and bool((words[G + 3 * slots:] == WORD).all())


# ---- A4b: both families share one workspace layout: a workspace of EXACTLY the reported size, between guard bytes --------------------

HDR = np.dtype([("minp", "<i4", 3), ("dims", "<i4", 3), ("cells", "<i8"), ("total", "<i8"), ("center", "<u4", 3), ("pad_", "<i4", 3)])
EXACT_N = [0, 1, 255, 256, 257, 513]  # the block-count edges of the two reductions (256 points per block) and the empty call
BYTE = 0x5A


def raster_points(n, seed):
    """n points of [-1, 1]^3 on a raster of 2^-12: a double sum of them is exact in any order, so the device's mean is numpy's."""
    return (np.round(np.random.RandomState(seed).uniform(-1.0, 1.0, size=(n, 3)) * 4096.0) / 4096.0).astype(np.float32)


def _fenced(inner, dtype, fill):
    return torch.full((G + inner + G,), fill, dtype=dtype, device=DEV)


def _fences_whole(t, inner, fill):
    """Every element of ``t`` outside [G, G + inner) still holds ``fill``."""
    host = t.cpu().numpy()
    rest = np.concatenate([host[:G], host[G + inner:]])
    return rest.size >= 2 * G and rest.tobytes() == np.full(rest.shape, fill, dtype=rest.dtype).tobytes()


def _phases_exact(pos, rs, centralize, pad, slots):
    """bounds, count and write of one family (``rs`` None: the un-batched one) at voxel 0.1, every buffer between guards and the
    workspace as long as the size function says, not a byte more.  ``slots``: the hashed table, None: a dense one of exactly the
    headers' cells.  -> (points, the item headers, the output row splits | None)."""
    import ctypes
    from dmcf_amd import ops, _lib
    L, stream = _lib.lib(), ops._stream
    n, batch, sfx = pos.shape[0], 1 if rs is None else len(rs) - 1, "" if rs is None else "_batched"
    rs_dev = None if rs is None else torch.tensor(rs, dtype=torch.int64, device=DEV)
    nb = L.dmcf_grid_pos_workspace_bytes(n) if rs is None else L.dmcf_grid_pos_workspace_bytes_batched(n, batch)
    assert nb >= 64 * batch
    ws = _fenced(nb, torch.uint8, BYTE)
    w = ws.data_ptr() + G
    assert w % 256 == 0
    head = (pos.data_ptr(), n) + (() if rs is None else (rs_dev.data_ptr(), batch)) + ((ctypes.c_float * 3)(0.1, 0.1, 0.1), centralize)
    assert getattr(L, "dmcf_grid_pos_bounds" + sfx)(*head, None, pad, 0.1, w, nb, stream()) == 0

    def headers():
        return np.frombuffer(ws[G:G + 64 * batch].cpu().numpy().tobytes(), dtype=HDR)

    cells = int(np.maximum(headers()["cells"], 0).sum())
    words, table_cells = (cells, cells) if slots is None else (3 * slots, -slots)
    table = _fenced(words, torch.int32, WORD)
    ors = _fenced(batch + 1, torch.int64, WORD)
    assert getattr(L, "dmcf_grid_pos_count" + sfx)(*head, pad, 0.1, w, nb, table.data_ptr() + 4 * G, table_cells,
                                                   *(() if rs is None else (ors.data_ptr() + 8 * G,)), stream()) == 0
    total = int(headers()["total"].sum())
    out = _fenced(3 * total, torch.float32, FSENT)
    assert getattr(L, "dmcf_grid_pos_write" + sfx)(*head, pad, 0.1, w, nb, table.data_ptr() + 4 * G, table_cells,
                                                   out.data_ptr() + 4 * G, total, stream()) == 0
    torch.cuda.synchronize()
    assert _fences_whole(ws, nb, BYTE), "workspace"
    assert _fences_whole(table, words, WORD), "cell table"
    assert _fences_whole(out, 3 * total, FSENT), "points"
    assert _fences_whole(ors, 0 if rs is None else batch + 1, WORD), "output row splits"
    return (out[G:G + 3 * total].cpu().numpy().reshape(-1, 3), headers(),
            None if rs is None else ors[G:G + batch + 1].tolist())


@pytest.mark.parametrize("n", EXACT_N)
def test_abi_both_families_on_a_workspace_of_exactly_the_reported_size(oracle, n):
    """The un-batched and the batched entry points carve one workspace layout.  Every phase of both, on ``n`` points as one
    item, behind an empty item and as three items with an empty one in the middle, with a dense table of exactly the headers'
    cells and with a hashed one: no byte outside any buffer changes, every item's points and header are the oracle's for its
    slice, and the un-batched call and the call with row splits [0, n] leave the same bytes in points and header."""
    from dmcf_amd import ops
    p = raster_points(n, seed=100 + n)
    pos = torch.from_numpy(p).to(DEV)
    forms = [None, [0, n], [0, 0, n], [0, n // 3, n // 3, n]]
    for centralize in (0, 1):
        for pad in (0, 1):
            o = dict(centralize=bool(centralize), pad=pad, hyst=0.1, center=None)
            refs = {}
            for slots in (None, ops._grid_hash_slots(n, [0.1] * 3, pad)):
                got = []
                for rs in forms:
                    tag = (n, centralize, pad, slots, rs)
                    pts, hdr, ors = _phases_exact(pos, rs, centralize, pad, slots)
                    splits = [0, n] if rs is None else rs
                    host = [0]
                    for b, (lo, hi) in enumerate(zip(splits[:-1], splits[1:])):
                        if (lo, hi) not in refs:
                            refs[(lo, hi)] = reference(oracle, p[lo:hi], [0.1] * 3, o)
                        ref, box, cells = refs[(lo, hi)]
                        assert same_bits(pts[host[b]:host[b] + ref.shape[0]], ref), (tag, b)
                        assert (int(hdr["cells"][b]), int(hdr["total"][b])) == (cells, ref.shape[0]), (tag, b)
                        assert box is None or (hdr["minp"][b].tolist(), hdr["dims"][b].tolist()) == box, (tag, b)
                        host.append(host[b] + ref.shape[0])
                    assert pts.shape[0] == host[-1] and (ors is None or ors == host), (tag, ors, host)
                    got.append((pts, hdr))
                (one, one_hdr), (many, many_hdr) = got[0], got[1]
                assert one.tobytes() == many.tobytes(), (n, centralize, pad, slots)
                for field in ("minp", "dims", "cells", "total", "center"):
                    assert one_hdr[field].tobytes() == many_hdr[field].tobytes(), (n, centralize, pad, slots, field)


# ---- A5: levels with different numbers of active axes share one call, hashed ---------------------------------------------------------

def isolated_plane(seed, n=250):
    """n points on z = 0 on a jittered 16 x 16 grid of pitch 1.0: ten voxels apart, no two points share a candidate cell."""
    rng = np.random.RandomState(seed)
    ij = np.stack(np.meshgrid(np.arange(16), np.arange(16), indexing="ij"), axis=-1).reshape(-1, 2)[:n]
    p = np.zeros((n, 3), dtype=np.float32)
    p[:, :2] = ij + rng.uniform(-0.3, 0.3, size=(n, 2))
    return p


MIXED = [[0.1, 0.1, 0.0], [0.1, 0.1, 0.1]]


@pytest.mark.parametrize("order", ["flat_first", "flat_last"])
def test_hashed_levels_with_different_active_axes(grid, oracle, monkeypatch, order):
    """The 3-D level offers 64 candidates per row where the 2-D level offers 16, and on z = 0 the +h row never equals the -h row:
    80 distinct cells per point and more (where the hysteresis also crosses a voxel in x or y).  A hashed table sized from the
    2-D level alone has fewer slots than the 3-D level has cells:
    with that sizing the 3-D level came back with one row per slot, 16384 of 21095 rows (32768 of 42292 with row splits), the rest
    dropped without a report.  Both wrappers now size the table from the level with the most offsets."""
    ops, _ = grid
    monkeypatch.setattr(ops, "GRID_MAX_CELLS", 0)  # every level hashed
    o = dict(PLAIN, centralize=False, pad=1)
    sizes = MIXED if order == "flat_first" else MIXED[::-1]
    items = [isolated_plane(21), isolated_plane(22)]
    refs = [[reference(oracle, it, v, o)[0] for v in sizes] for it in items]
    flat, full = (0, 1) if order == "flat_first" else (1, 0)
    # the premise: the 3-D level has more lattice points than a table sized from the 2-D level has slots
    assert ops._grid_hash_slots(250, MIXED[0], 1) == 16384 < refs[0][full].shape[0]
    assert ops._grid_hash_slots(500, MIXED[0], 1) == 32768 < refs[0][full].shape[0] + refs[1][full].shape[0]
    assert refs[0][full].shape[0] >= 78 * 250 and refs[0][flat].shape[0] <= 25 * 250
    res = ops.grid_pos_many(torch.from_numpy(items[0]).to(DEV), [np.float32(v) for v in sizes], pad=1)
    for level, (got, _) in enumerate(res):
        print(f"{order} level {level}: {got.shape[0]} points, oracle {refs[0][level].shape[0]}")
    for level, (got, _) in enumerate(res):
        assert same_bits(got, refs[0][level]), (level, got.shape[0], refs[0][level].shape[0])
    rs = [0, 250, 500]
    res = ops.grid_pos_many(torch.from_numpy(np.concatenate(items)).to(DEV), [np.float32(v) for v in sizes], pad=1, row_splits=rs)
    for level, (got, splits) in enumerate(res):
        want = np.concatenate([refs[0][level], refs[1][level]])
        print(f"{order} batched level {level}: {got.shape[0]} points, oracle {want.shape[0]}")
        assert splits.sparse
        assert splits.host == (0, refs[0][level].shape[0], want.shape[0]) and splits.dev.tolist() == list(splits.host)
        assert same_bits(got, want), (level, got.shape[0], want.shape[0])
