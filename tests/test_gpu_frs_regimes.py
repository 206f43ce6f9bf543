"""Every form of the radius search on each grid regime it can build (dmcf_amd/csrc/frs.hip), scene x build.

One table per case, built by ops.build_spatial_hash_table -- by the single-workgroup build (frs_build_small) or, under
DMCF_FRS_NO_SMALL_BUILD, by the general ten-launch one -- and read back with frs_regimes.decode.  The case then
  1. asserts the scene's regime from the header the DEVICE built (tests/frs_regimes.py holds the scenes and what each must reach;
     tests/test_frs_regimes_cpu.py holds them to it under the host restatement, with room);
  2. asserts the build product: cell_start is the histogram of the restated float32 cell coordinates, the index column of
     ``sorted`` their stable sort, every entry's xyz its point, bit for bit;
  3. runs every form on THAT table (``hash_table=``; the radius-per-query search, which ops always builds a table of its own
     for, through its C entry points): the CSR search with and without ignore_query_point and under the two open3d readings, the
     padded single pass with a stride that holds every row and with one that cuts the long ones, the radius-per-query search,
     the max-norm search, and the fused window sum for every window under the element-wise bar of frs_regimes.
test_report_worst_ratio prints the worst err / bar per window (run with -s).  One more case drives the scan of the row counts
(scan_counts_to_row_splits, misc.hip) through three rounds of its block-sum loop."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import frs_regimes as fg  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
BUILDS = ["small", "general"]
SETS = {"open3d": "own+corners", "open3d_corners": "corners"}  # DMCF_FRS_SET -> the oracle's statement of it (oracle.BINS)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but torch.cuda.is_available() is False")
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)  # (a copy: the scenes are read-only)


class _Case:
    """The table of (scene, build) on the device, its decoded header, the queries for that grid, and a guard that fails the
    test if any form builds a table of its own."""

    def __init__(self, dev, monkeypatch, name, build):
        from dmcf_amd import ops
        self.name, self.scene, self.dev = name, fg.SCENES[name], dev
        self.radius = float(self.scene.radius)
        self.pts = fg.points(name)
        self.P = _t(self.pts, dev)
        if build == "small":
            monkeypatch.delenv("DMCF_FRS_NO_SMALL_BUILD", raising=False)
        else:
            monkeypatch.setenv("DMCF_FRS_NO_SMALL_BUILD", "1")
        monkeypatch.delenv("DMCF_FRS_SET", raising=False)
        # (room for the face queries, whose number depends on the grid that is about to be built)
        self.table = ops.build_spatial_hash_table(self.P, self.radius, n_queries=len(self.pts) // 4 + 1024)
        self.header = fg.decode(self.table)
        self.qs = fg.queries(name, self.header)
        assert len(self.qs) <= self.table.n_queries_capacity
        self.Q = _t(self.qs, dev)

        def no_rebuild(*a, **kw):
            raise AssertionError("a form of the search built a table of its own instead of using hash_table=")
        monkeypatch.setattr(ops, "build_spatial_hash_table", no_rebuild)

    def tag(self, what):
        return f"{self.name} {what}"


def _np(res):
    return tuple(x.cpu().numpy() for x in res)


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("name", list(fg.SCENES))
def test_regime_and_build_product(dev, monkeypatch, name, build):
    c = _Case(dev, monkeypatch, name, build)
    h, pts = c.header, c.pts
    cell, beyond, occ = fg.binning(pts, h)
    print(f"{name} / {build}: origin {h['origin']}, cells per radius {fg.cells_per_radius(h):.4f}, dims {h['dims']}, "
          f"ncells {h['ncells']} of {h['table']}, beyond the grid {beyond.mean():.4f}, largest cell {occ.max()}")
    # 1. the regime, from the device's header
    assert h["ncells"] <= h["table"] == fg.table_size(len(pts))
    assert np.all(h["inv_cell"] == h["inv_cell"][0]) and np.isfinite(h["origin"]).all() and h["inv_cell"][0] > 0
    assert np.array_equal(h["bb_min"], pts.min(0)) and np.array_equal(h["bb_max"], pts.max(0))
    if c.scene.regime is not None:
        c.scene.regime(h, occ, beyond)
        # the restatement of the sizing, fed the device's own box and sums, lands on the device's grid
        want = fg.sizing(h["bb_min"], h["bb_max"], h["sum"], h["sumsq"], len(pts), c.radius)
        assert np.array_equal(want["dims"], h["dims"]), (want["dims"], h["dims"])
        assert np.allclose(want["inv_cell"], h["inv_cell"], rtol=1e-6, atol=0) and np.allclose(want["origin"], h["origin"], rtol=1e-6, atol=1e-9)
    # 2. the build product
    start = h["cell_start"]
    assert np.array_equal(start[:h["ncells"] + 1], np.concatenate([[0], np.cumsum(occ)])), "cell_start is not the histogram's scan"
    assert np.all(start[h["ncells"]:] == len(pts)), "the table's unused tail does not end the last cell"
    assert np.array_equal(h["sorted_index"], fg.expected_sort(pts, h)), "sorted is not the stable sort by cell"
    assert np.array_equal(h["sorted_xyz"].view(np.uint32), pts[h["sorted_index"]].view(np.uint32)), "an entry's xyz is not its point"


def _padded_abi(c, ignore, stride, flags=0):
    """dmcf_frs_search_padded on the case's table into buffers filled with a sentinel.  -> (index [m, stride], d2 [m, stride],
    counts, max_count, row_begin, the sentinel-filled tail behind the last row)."""
    from dmcf_amd import _lib, ops
    L = _lib.lib()
    n, m = len(c.pts), len(c.qs)
    nbytes = L.dmcf_frs_workspace_bytes(n, c.table.n_queries_capacity)
    tail = 512
    index = torch.full((m * stride + tail,), -7, dtype=torch.int32, device=c.dev)
    dist = torch.full((m * stride + tail,), -7.0, dtype=torch.float32, device=c.dev)
    begin = torch.empty(m + 1, dtype=torch.int64, device=c.dev)
    counts = torch.empty(m, dtype=torch.int32, device=c.dev)
    max_count = torch.zeros(1, dtype=torch.int32, device=c.dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    _lib.check(L.dmcf_frs_search_padded(p(c.Q), m, n, c.radius, (1 if ignore else 0) | flags, p(c.table.workspace), nbytes, stride,
                                        p(begin), p(counts), p(index), p(dist), p(max_count), ops._stream()), "dmcf_frs_search_padded")
    torch.cuda.synchronize()
    index, dist = index.cpu().numpy(), dist.cpu().numpy()
    return (index[:m * stride].reshape(m, stride), dist[:m * stride].reshape(m, stride), counts.cpu().numpy(), int(max_count.item()),
            begin.cpu().numpy(), (index[m * stride:], dist[m * stride:]))


def _check_padded(c, ignore, stride):
    ref = fg.reference(c.name, c.qs, ignore)
    want = np.diff(ref[1])
    index, dist, counts, max_count, begin, (ti, td) = _padded_abi(c, ignore, stride)
    tag = c.tag(f"padded stride {stride} ignore {ignore}")
    assert np.array_equal(begin, np.arange(len(c.qs) + 1) * stride), tag
    assert max_count == want.max(), f"{tag}: max_count {max_count}, longest row {want.max()}"
    assert np.array_equal(counts, np.minimum(want, stride)), f"{tag}: counts"
    col = np.arange(stride)[None, :]
    written = col < counts[:, None]
    assert np.all(index[~written] == -7) and np.all(dist[~written] == -7) and np.all(ti == -7) and np.all(td == -7), \
        f"{tag}: something was written beyond a row's count or stride"
    # the written prefix: the whole row where it fits; distinct members of the row, each with its own distance, where it is cut
    rows = np.repeat(np.arange(len(c.qs)), counts)
    got = (index[written], np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), dist[written])
    if stride >= want.max():
        fg.check_rows(tag, got, ref)
        return
    key_ref = np.repeat(np.arange(len(c.qs), dtype=np.int64), want) * len(c.pts) + ref[0]
    key_got = rows.astype(np.int64) * len(c.pts) + got[0]
    assert len(np.unique(key_got)) == len(key_got), f"{tag}: a neighbour twice in a cut row"
    order = np.argsort(key_ref)
    at = np.searchsorted(key_ref[order], key_got)
    assert np.all(at < len(key_ref)) and np.array_equal(key_ref[order][np.minimum(at, len(key_ref) - 1)], key_got), \
        f"{tag}: a cut row holds an index that is not a neighbour"
    assert np.array_equal(ref[2][order][at].view(np.uint32), got[2].view(np.uint32)), f"{tag}: distances of a cut row"


def _radius_search_abi(c, radii, ignore):
    """dmcf_radius_search_count / _write on the case's table, with the table's radius as max_radius."""
    from dmcf_amd import _lib, ops
    L = _lib.lib()
    n, m = len(c.pts), len(c.qs)
    nbytes = L.dmcf_frs_workspace_bytes(n, c.table.n_queries_capacity)
    R = _t(radii, c.dev)
    rs = torch.empty(m + 1, dtype=torch.int64, device=c.dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    flags = 1 if ignore else 0
    _lib.check(L.dmcf_radius_search_count(p(c.Q), m, n, p(R), c.radius, flags, p(c.table.workspace), nbytes, p(rs), ops._stream()),
               "dmcf_radius_search_count")
    total = int(rs[-1].item())
    index = torch.full((total + 64,), -7, dtype=torch.int32, device=c.dev)
    dist = torch.full((total + 64,), -7.0, dtype=torch.float32, device=c.dev)
    _lib.check(L.dmcf_radius_search_write(p(c.Q), m, n, p(R), c.radius, flags, p(c.table.workspace), nbytes, p(rs), p(index), p(dist),
                                          total, ops._stream()), "dmcf_radius_search_write")
    torch.cuda.synchronize()
    assert torch.all(index[total:] == -7) and torch.all(dist[total:] == -7), "written beyond the last row"
    return index[:total].cpu().numpy(), rs.cpu().numpy(), dist[:total].cpu().numpy()


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("name", list(fg.SCENES))
def test_every_list_form(oracle, dev, monkeypatch, name, build):
    from dmcf_amd import ops
    c = _Case(dev, monkeypatch, name, build)
    kw = dict(hash_table=c.table)
    longest = 0
    for ignore in (False, True):
        # CSR: row splits, index sets and squared distances bit for bit
        ref = fg.reference(name, c.qs, ignore)
        longest = max(longest, int(np.diff(ref[1]).max()))
        res = ops.fixed_radius_search(c.P, c.Q, c.radius, ignore_query_point=ignore, return_distances=True, **kw)
        assert res.neighbors_index.dtype == torch.int32 and res.neighbors_row_splits.dtype == torch.int64
        fg.check_rows(c.tag(f"csr ignore {ignore}"), _np(res), ref)
        res = ops.fixed_radius_search(c.P, c.Q, c.radius, ignore_query_point=ignore, return_distances=False, **kw)
        fg.check_rows(c.tag(f"csr index only ignore {ignore}"), _np(res)[:2], ref[:2])
        # the same under the two open3d readings, against the oracle's statement of each set
        if name != "far":
            for env, bins in SETS.items():
                monkeypatch.setenv("DMCF_FRS_SET", env)
                res = ops.fixed_radius_search(c.P, c.Q, c.radius, ignore_query_point=ignore, return_distances=True, **kw)
                monkeypatch.delenv("DMCF_FRS_SET")
                want = oracle.fixed_radius_search(c.pts, c.qs, c.radius, ignore, bins=bins)
                fg.check_rows(c.tag(f"{env} ignore {ignore}"), _np(res), want)
                assert np.all(np.diff(want[1]) <= np.diff(ref[1])), "the walk's set is a subset of the distance set"
        # padded rows through ops: counts, max_count and every row's prefix
        stride = int(np.diff(ref[1]).max()) + 3
        pad = ops.fixed_radius_search(c.P, c.Q, c.radius, ignore_query_point=ignore, return_distances=True, row_stride=stride, **kw)
        assert isinstance(pad, ops.PaddedNeighborList) and pad.stride == stride
        assert int(pad.max_count.item()) == int(np.diff(ref[1]).max())
        assert np.array_equal(pad.row_count.cpu().numpy(), np.diff(ref[1]))
        assert np.array_equal(pad.neighbors_row_splits.cpu().numpy(), np.arange(len(c.qs) + 1) * stride)
        fg.check_rows(c.tag(f"padded, compacted, ignore {ignore}"), _np(tuple(pad)), ref)
        # ... and through the entry point into sentinel-filled buffers: a stride that holds every row, one that cuts the long ones
        _check_padded(c, ignore, stride)
        cut = max(1, int(np.sort(np.diff(ref[1]))[len(c.qs) * 3 // 4]) // 2)
        assert cut < np.diff(ref[1]).max()
        _check_padded(c, ignore, cut)
        # a radius per query
        radii = fg.radii_for(name, len(c.qs))
        fg.check_rows(c.tag(f"radii ignore {ignore}"), _radius_search_abi(c, radii, ignore), fg.reference_radii(name, c.qs, ignore))
        # the max-norm set
        res = ops.fixed_radius_search(c.P, c.Q, c.radius, ignore_query_point=ignore, return_distances=False, metric="Linf", **kw)
        fg.check_rows(c.tag(f"linf ignore {ignore}"), _np(res)[:2], fg.reference_linf(name, c.qs, ignore))
    if name == "clump":  # (heavy_tail's full cell is a long run of CANDIDATES; here the hits themselves span the windows)
        assert longest > fg.WIN * 4 * 64


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("name", list(fg.SCENES))
def test_window_sums(dev, monkeypatch, name, build):
    from dmcf_amd import ops
    c = _Case(dev, monkeypatch, name, build)
    n = len(c.pts)
    for window in fg.WINDOWS + [None]:
        for ignore in ((False, True) if window in ("poly6", "cubic_grad", None) else (False,)):
            got = ops.window_sum(c.P, c.Q, c.radius, window=window, ignore_query_point=ignore, hash_table=c.table)
            assert got.dtype == torch.float32 and got.shape == (len(c.qs),)
            ref, A, k = fg.window_sum_ref(name, window, c.qs, ignore)
            fg.check_window_sum(c.tag(f"{build} {window} ignore {ignore}"), window, got.cpu().numpy(), ref, A, k, n)


def test_report_worst_ratio():
    """Prints the worst err / bar of every window over the cases of this file (run with -s)."""
    print("worst err/bar", {k: round(v, 4) for k, v in fg.WORST.items()})


def test_row_count_scan_runs_three_rounds(dev):
    """64 points, 1,050,629 queries: ceil(m / 2048) = 514 block sums, so the loop of scan_sums_inplace runs three times in the
    int64 instantiation that turns every search's counts into row splits."""
    from dmcf_amd import ops
    rng = np.random.default_rng(77)
    n, m, radius = 64, 1_050_629, 0.3
    assert 2 * 256 < -(-m // 2048) <= 3 * 256
    pts = rng.uniform(0, 1, size=(n, 3)).astype(F)
    qs = rng.uniform(0, 1, size=(m, 3)).astype(F)
    res = ops.fixed_radius_search(_t(pts, dev), _t(qs, dev), radius, return_distances=True)
    idx, rs, d2 = _np(res)
    r2 = F(radius) * F(radius)
    cnt = np.empty(m, np.int64)
    keys, dist = [], []
    for q0 in range(0, m, 1 << 16):
        q = qs[q0:q0 + (1 << 16)]
        dx, dy, dz = (pts[None, :, a] - q[:, None, a] for a in range(3))
        d = (dx * dx + dy * dy) + dz * dz
        hit = d <= r2
        cnt[q0:q0 + len(q)] = hit.sum(1)
        rows, cols = np.nonzero(hit)
        keys.append((rows + q0).astype(np.int64) * n + cols)
        dist.append(d[rows, cols])
    want_rs = np.concatenate([[0], np.cumsum(cnt)])
    assert np.array_equal(rs, want_rs), "row splits differ from the brute force"
    assert 5_000_000 < rs[-1] == len(idx)
    key = np.repeat(np.arange(m, dtype=np.int64), np.diff(rs)) * n + idx
    order = np.argsort(key, kind="stable")
    assert np.array_equal(key[order], np.concatenate(keys)), "neighbour sets differ from the brute force"
    assert np.array_equal(d2[order].view(np.uint32), np.concatenate(dist).view(np.uint32)), "squared distances are not bit-exact"
