"""CPU side of the primitive edge cases (tests/primitive_edges_ref.py, tests/test_gpu_primitive_edges.py): every condition a
case must meet is asserted here without a GPU -- the thresholds the list lengths sit around, the key widths and sentinels of
the inversion's lists, min |v| > 2 * bar for the row sums, the brute-force counts of the scan scene, the ties of the sampling
cases, K * Cin * Cout above the cap for the backward cases, and the packed-filter counts either side of the packers' caps.  The
references pass their own checkers, and seeded faults of the references fail them."""
import math

import numpy as np
import pytest

import cconv_backward_ref as bref
import cconv_forward_ref as fr
import primitive_edges_ref as pe

F = np.float32


def _fails(fn, *a):
    with pytest.raises(AssertionError):
        fn(*a)


# ---- A ---------------------------------------------------------------------------------------------------------------------------

def test_thresholds_are_the_constants_the_lengths_sit_around():
    """1024 = 256 x 4 (rocPRIM's single-block sort) and 1 << 20 (its merge-sort limit, and the 4096 blocks x 256 threads of
    grid_for) are the numbers the list lengths of INVERT_CASES straddle."""
    assert pe.SORT_BLOCK_ITEMS == pe.SORT_BLOCK_SIZE * pe.SORT_ITEMS_PER_THREAD == 256 * 4 == 1024
    assert pe.SORT_MERGE_LIMIT == 1024 * 1024 == 1 << 20 == pe.GRID_FOR_CAP == 4096 * 256
    lengths = {c[0] for c in pe.INVERT_CASES.values()}
    assert lengths >= {1, 2, 1023, 1024, 1025, 4097, 1_048_575, 1_048_576, 1_048_577, 1_300_003, 0}
    for t in (pe.SORT_BLOCK_ITEMS, pe.SORT_MERGE_LIMIT):
        assert {t - 1, t, t + 1} <= lengths


def test_invert_cases_cover_what_they_are_named_for():
    cases = {n: pe.invert_case(n) for n in pe.INVERT_CASES}
    assert len(cases) >= 16
    widths = {c["n_inp"] for c in cases.values()}
    assert widths >= {1, 2, 3, 255, 256, 257, 65535, 65536, 65537}
    for name, c in cases.items():
        P, n_inp, kind, opt = pe.INVERT_CASES[name]
        idx, rs = c["index"], c["row_splits"]
        assert idx.dtype == np.int32 and idx.shape == (P,) and rs.dtype == np.int64 and not idx.flags.writeable
        assert pe.invert_case(name) is c
        if c["m"] and not opt.get("one_key"):  # every list references input 0 and input n_inp - 1
            assert c["valid_j"].min() == 0 and c["valid_j"].max() == n_inp - 1, name
        if opt.get("one_key"):
            assert n_inp == 1 and np.all(c["valid_j"] == 0) and np.array_equal(c["pair_index"], np.arange(P)), name
        # the expected result is a permutation of the valid pairs, sorted by input, ascending in pair position inside a row
        j_sorted = c["index"][c["pair_index"]]
        assert np.all(np.diff(j_sorted) >= 0) and np.all((np.diff(c["pair_index"]) > 0) | (np.diff(j_sorted) > 0)), name
        assert c["neighbors_row_splits"].shape == (n_inp + 1,) and c["neighbors_row_splits"][-1] == c["m"] <= P
    # 256 and 65536 with a length above the merge-sort limit and the grid cap
    for n_inp in (256, 65536):
        assert any(c["n_inp"] == n_inp and c["index"].shape[0] > pe.SORT_MERGE_LIMIT for c in cases.values())
    # the sentinel at a power of two needs one bit more than the largest valid key: such lists must carry sentinels
    for n_inp in (256, 65536):
        assert n_inp & (n_inp - 1) == 0 and (n_inp - 1).bit_length() + 1 == n_inp.bit_length()
        with_bad = [c for n, c in cases.items() if c["n_inp"] == n_inp and pe.INVERT_CASES[n][3].get("invalid")]
        assert with_bad
        for c in with_bad:
            inside = c["index"][:c["row_splits"][-1]]
            for bad in (-1, n_inp, pe.INT32_MAX):
                assert (inside == bad).sum() >= 10, (c["name"], bad)
            assert c["m"] == ((inside >= 0) & (inside < n_inp)).sum() < inside.size
    # a buffer longer than its rows: the slack holds 0, and input 0's row does not grow
    for name in ("slack_p1025_k256", "slack_p1048577_k65536"):
        c = cases[name]
        covered = int(c["row_splits"][-1])
        assert covered < c["index"].shape[0] and np.all(c["index"][covered:] == 0) and c["m"] == covered
        assert c["neighbors_row_splits"][1] == (c["index"][:covered] == 0).sum() < (c["index"] == 0).sum()
    # the padded form: three rows with pairs reach past the buffer, one of them beginning inside it; padding slots hold 0
    c = cases["padded_p1025"]
    P, begin, cnt = c["index"].shape[0], c["row_splits"], c["row_count"]
    past = (begin[:-1] + cnt > P) & (cnt > 0)
    assert P >= 1025 and past.sum() == 3 and (begin[:-1][past] < P).sum() == 1 and cnt.dtype == np.int32
    assert not np.isin(np.flatnonzero(past), c["valid_row"]).any() and c["m"] == cnt[~past & (begin[:-1] + cnt <= P)].sum()
    slots = np.ones(P, bool)
    slots[c["valid_pos"]] = False
    assert np.all(c["index"][slots] == 0) and slots.sum() > 100
    # strictly descending, no rows, no pairs
    d = cases["descending_p1025"]
    assert np.all(np.diff(d["index"].astype(np.int64)) == -1) and np.array_equal(d["pair_index"], np.arange(1024, -1, -1))
    assert cases["n_out_0"]["row_splits"].shape == (1,) and cases["n_out_0"]["m"] == 0 and cases["n_out_0"]["index"].size > 0
    z = cases["p0_k257"]
    assert z["index"].size == 0 and z["n_inp"] == 257 and np.all(z["neighbors_row_splits"] == 0)


def test_invert_checker_has_teeth():
    c = pe.invert_case("p1025_k256_invalid")
    m, P = c["m"], c["index"].shape[0]

    def full(a, fill, dtype):
        out = np.full(P, fill, dtype)
        out[:m] = a
        return out
    good = [full(c["neighbors_index"], -1, np.int32), c["neighbors_row_splits"].copy(), full(c["neighbors_attributes"], 0, F),
            full(c["pair_index"], -1, np.int32)]
    pe.check_invert(c, *good)
    # two pairs of one row swapped (an unstable sort); a sentinel sorted as key 0 (end_bit one short); a tail entry not -1
    row = int(np.argmax(np.diff(c["neighbors_row_splits"]) >= 2))
    at = int(c["neighbors_row_splits"][row])
    swapped = [a.copy() for a in good]
    for a in (swapped[0], swapped[2], swapped[3]):
        a[[at, at + 1]] = a[[at + 1, at]]
    _fails(pe.check_invert, c, *swapped)
    grown = [a.copy() for a in good]
    grown[1][1:] += 1
    _fails(pe.check_invert, c, *grown)
    tail = [a.copy() for a in good]
    tail[3][m] = 0
    _fails(pe.check_invert, c, *tail)


# ---- B ---------------------------------------------------------------------------------------------------------------------------

def test_reduce_cases_resolve_a_single_element():
    assert set(pe.ROW_LENGTHS) == {0, 1, 15, 16, 17, 31, 32, 33, 255, 256, 257, 4101}
    assert {n for n, _ in pe.REDUCE_CASES} == {1, 15, 16, 17, 4097}
    seen = set()
    for n_rows, start in pe.REDUCE_CASES:
        v, rs, ref, bar, lengths = pe.reduce_case(n_rows, start)
        assert v.dtype == F and rs.dtype == np.int64 and rs[-1] == v.size and not v.flags.writeable
        seen |= set(lengths.tolist())
        assert np.all((np.abs(v) >= 0.5) & (np.abs(v) <= 1.0)) and (v < 0).any() == (v > 0).any()
        row = np.repeat(np.arange(n_rows), lengths)
        # the bar as derived: (ceil(len / 16) + 5) 2^-24 sum |v|, and min |v| > 2 * bar in every row
        absum = np.bincount(row, weights=np.abs(v).astype(np.float64), minlength=n_rows)
        assert np.array_equal(bar, (np.ceil(lengths / 16) + 5) * 2.0 ** -24 * absum)
        assert np.all(np.abs(v) > 2 * bar[row]), (n_rows, start)
        assert np.all(bar[lengths == 0] == 0)
        if n_rows >= 15:  # empty rows sit between long ones
            assert (lengths == 0).any() and lengths[np.flatnonzero(lengths == 0)[0] - 1 if lengths[0] else 1] > 0
        # the float32 sum in list order passes; one element dropped, or counted twice, fails in every non-empty row tried
        got = np.array([v[rs[i]:rs[i + 1]].sum(dtype=F) for i in range(n_rows)], F)
        pe.check_reduce(got, ref, bar, lengths)
        for i in np.flatnonzero(lengths)[[0, -1]]:
            k = int(np.argmin(np.abs(v[rs[i]:rs[i + 1]])))
            for sign in (-1, 1):
                bad = got.copy()
                bad[i] = F(np.float64(got[i]) + sign * np.float64(v[rs[i] + k]))
                _fails(pe.check_reduce, bad, ref, bar, lengths)
        if (lengths == 0).any():
            bad = got.copy()
            bad[np.flatnonzero(lengths == 0)[0]] = F(1e-30)
            _fails(pe.check_reduce, bad, ref, bar, lengths)
    assert seen == set(pe.ROW_LENGTHS)
    pe.WORST.pop("reduce", None)


# ---- C ---------------------------------------------------------------------------------------------------------------------------

def test_scan_sizes_sit_on_the_tile_and_round_edges():
    assert pe.SCAN_TILE == 256 * 8 and pe.SCAN_ROUND == 256 * pe.SCAN_TILE == 524_288
    assert set(pe.SCAN_SIZES) >= {pe.SCAN_TILE - 1, pe.SCAN_TILE, pe.SCAN_TILE + 1, 2 * pe.SCAN_TILE, pe.SCAN_ROUND - 1,
                                  pe.SCAN_ROUND, pe.SCAN_ROUND + 1}
    # the total is written by the thread that holds element n - 1: the last thread of the last block iff n % 2048 == 0
    assert sum(m % pe.SCAN_TILE == 0 for m in pe.SCAN_SIZES) >= 3
    p = pe.scan_points()
    assert p.shape == (10, 3) and np.array_equal(np.bincount(pe.POINT_SITE, minlength=5), pe.SITE_COUNTS)
    assert np.abs(p[:, 1:]).max() <= 0.04 * pe.SCAN_RADIUS and np.array_equal(p[:, 0], pe.POINT_SITE.astype(F))
    m = pe.SCAN_SIZES[-1]
    sites = pe.scan_sites(m)
    i = np.arange(m)
    assert np.array_equal(sites, (7 * i + i // 2048) % 5) and set(sites[:5].tolist()) == {0, 1, 2, 3, 4}
    # the count pattern is not periodic in the tile: consecutive tiles begin at different sites
    assert len({int(sites[t * 2048]) for t in range(5)}) == 5
    counts, rs = pe.scan_expected(m)
    assert rs.dtype == np.int64 and rs.shape == (m + 1,) and rs[-1] == counts.sum() and counts.max() == 4 and counts.min() == 0


@pytest.mark.parametrize("m", pe.SCAN_SIZES)
def test_scan_scene_counts_under_a_float64_brute_force(m):
    """The constructed counts are those of a float64 brute force on a sample of 4,096 queries (both ends, the tile edge, an
    even spread), every row's neighbours are its site's cluster, and no pair distance lies within 1 % of the radius."""
    p, q = pe.scan_points().astype(np.float64), pe.scan_queries(m)
    assert q.dtype == F and q.shape == (m, 3)
    sample = pe.scan_sample(m)
    assert sample.size == min(m, 4096) and sample[0] == 0 and sample[-1] == m - 1 and np.all(np.diff(sample) > 0)
    assert {min(2047, m - 1), min(2048, m - 1)} <= set(sample.tolist())
    d = np.sqrt(((q[sample].astype(np.float64)[:, None, :] - p[None, :, :]) ** 2).sum(-1))
    hit = d <= float(F(pe.SCAN_RADIUS))
    counts, _ = pe.scan_expected(m)
    assert np.array_equal(hit.sum(1), counts[sample])
    assert np.array_equal(hit, pe.POINT_SITE[None, :] == pe.scan_sites(m)[sample][:, None])
    assert not np.any(np.abs(d - pe.SCAN_RADIUS) <= 0.01 * pe.SCAN_RADIUS)
    assert d[hit].max() < 0.05 * pe.SCAN_RADIUS and d[~hit].min() > 9 * pe.SCAN_RADIUS


# ---- D ---------------------------------------------------------------------------------------------------------------------------

def test_dense_sizes_take_the_row_loop_a_second_and_a_third_time():
    assert pe.DENSE_ROWS_PER_PASS == 2048 * 4 * 16 == 131_072
    assert set(pe.DENSE_N) == {15, 16, 17, 63, 64, 65, 131_072, 131_073, 262_147}
    passes = {n: math.ceil(math.ceil(n / 16) / (2048 * 4)) for n in pe.DENSE_N}
    assert passes[131_072] == 1 and passes[131_073] == 2 and passes[262_147] == 3
    assert set(pe.DENSE_KM) == {(32, 32), (64, 64), (12, 4), (20, 40)} and pe.DENSE_BAR == 4e-7
    for k, m in pe.DENSE_KM:
        assert k % 4 == 0 and k <= 64 and m <= 64  # dense_supported
    x, W, b, r, ref, scale = pe.dense_case(65, 20, 40)
    y = (x @ W).astype(F)
    yb = (x.astype(np.float64) @ W.astype(np.float64) + b + r).astype(F)
    pe.check_dense(y, yb, b, r, ref, scale)
    bad = y.copy()
    bad[64] = y[48]  # the last row written from another tile
    _fails(pe.check_dense, bad, yb, b, r, ref, scale)
    _fails(pe.check_dense, y, (yb - b).astype(F), b, r, ref, scale)
    pe.WORST.pop("dense", None)


# ---- E ---------------------------------------------------------------------------------------------------------------------------

def test_fps_sizes_sit_on_the_thread_and_register_edges():
    assert pe.FPS_REG_POINTS == 8 * 1024 == 8192
    assert set(pe.FPS_SIZES) == {1023, 1024, 1025, 8191, 8192, 8193} and pe.FPS_SAMPLES == 40
    assert {n for _, n in pe.FPS_TIES} == {8193, 9000} and 8192 % 512 == 0


@pytest.mark.parametrize("kind,n", pe.FPS_TIES)
def test_fps_ties_straddle_registers_and_workspace(oracle, kind, n):
    """The replay equals the oracle, and the ties the case is named for occur among the first 40 samples."""
    p = pe.fps_tie_points(kind, n)
    assert p.shape == (n, 3) and p.dtype == F
    idx, ties = pe.fps_replay(p, pe.FPS_SAMPLES)
    assert np.array_equal(idx, oracle.farthest_point_sample(pe.FPS_SAMPLES, p))
    R = pe.FPS_REG_POINTS
    won = [(int(idx[j + 1]), t) for j, t in enumerate(ties)]
    if kind == "copies":
        copies = [k for k in pe.COPIES_OF if k + R < n]
        for k in copies:
            assert np.array_equal(p[k], p[k + R]) and (k & 511) == ((k + R) & 511)
            assert any(w == k and set(t.tolist()) == {k, k + R} for w, t in won), f"no tie between {k} and its copy"
            assert k + R not in idx
        if not copies:  # n = 8193: the one workspace point is the copy of sample 0, at distance 0 from the first step on
            assert np.array_equal(p[R], p[0]) and R not in idx
    elif kind == "mirror":
        assert any(w >= R and (t < R).any() for w, t in won), "no tie that the workspace point wins by i & 511"
        assert idx[1] == R and set(ties[0].tolist()) == {1, R}
    else:
        # equal i & 511 on both sides of 8192: the lower index wins
        hits = [(w, t) for w, t in won if w < R and ((t >= R) & ((t & 511) == (w & 511))).any()]
        assert hits, "no tie with equal i & 511 on both sides of 8192"
        assert len(ties[0]) == 8 and (ties[0] >= R).any() and (ties[0] < R).any()
        # ... and the lattice is one: 21^3 points at multiples of 1 / 8, no two alike
        assert np.all(p * 8 == np.round(p * 8)) and len(np.unique(p, axis=0)) == n


def test_gather_cases():
    assert {ch for _, ch in pe.GATHER_CASES} == {1, 3, 5, 64}
    assert {m * ch for m, ch in pe.GATHER_CASES} >= {255, 256, 257}
    for m, ch in pe.GATHER_CASES:
        feats, idx = pe.gather_case(m, ch)
        assert feats.shape == (pe.GATHER_N, ch) and idx.dtype == np.int32 and idx.min() >= 0 and idx.max() < pe.GATHER_N
        assert len(np.unique(idx)) < m, "no repeated index"


# ---- F ---------------------------------------------------------------------------------------------------------------------------

def test_backward_cases_exceed_the_grid_cap_and_are_the_smallest_that_do():
    assert [(c[1] is not None, c[4]) for c in pe.BWD_CAP_CASES] == [(False, False), (True, False), (False, True)]
    for shape, axis, cin, cout, _ in pe.BWD_CAP_CASES:
        K, n_full, n_stored = pe.bwd_cap_counts(shape, axis, cin, cout)
        assert K == 64 and bref.bwd_supported(K, cin, cout)
        assert K * cin == 8192 and K * cout == 8448 and n_full == K * cin * cout == 1_081_344 > 4096 * 256
        # symmetric: the expanded filter and the full gradient are above the cap, the stored half below it
        assert (n_stored == n_full) if axis is None else (n_stored == n_full // 2 < 4096 * 256)
    # one quad of output channels fewer is exactly the cap, and still accepted: the cases are the first above it
    assert 64 * 128 * 128 == 4096 * 256 and bref.bwd_supported(64, 128, 128) and bref.BWD_LDS_FLOATS == 16384


# ---- G ---------------------------------------------------------------------------------------------------------------------------

def test_packer_caps_and_the_cases_above_them():
    assert pe.PACK_FILTER_CAP == 2048 * 256 and pe.PACK_DIRECT_CAP == 1024 * 256 and pe.LAT_BUILD_CAP == 4096 * 256
    for kernel, shapes in pe.PACKER_CASES.items():
        for cin, cout in shapes:
            assert pe.packed_count(kernel, cin, cout) > pe.PACK_FILTER_CAP, (kernel, cin, cout)
            assert cout == 49  # the fewest output channels with four column tiles
    # the smallest: one input channel (lds, mfma) or one quad (blk, cls: Cin % 4 == 0) fewer stays at or below the cap
    cin, cout = pe.LDS_OVER_CAP
    assert pe.packed_count("lds", cin - 1, cout) <= pe.PACK_FILTER_CAP
    assert pe.mfma_packed(64, 128, 49) == pe.PACK_FILTER_CAP and pe.blk_packed(128, 49) == pe.PACK_FILTER_CAP
    assert pe.cls_packed(112, 49) <= pe.PACK_FILTER_CAP < pe.cls_packed(116, 49) == pe.PACK_FILTER_CAP + 16
    # fewer column tiles need more input channels still
    assert pe.mfma_packed(64, 129, 48) <= pe.PACK_FILTER_CAP and pe.cls_packed(116, 48) <= pe.PACK_FILTER_CAP
    # the matrix carries every one of them, forced to its kernel
    matrix = fr.matrix()
    for kernel, shapes in pe.PACKER_CASES.items():
        for cin, cout in shapes:
            assert any(kn == kernel and s["cin"] == cin and s["cout"] == cout and tuple(s["shape"]) == (4, 4, 4)
                       for _, kn, _, s in matrix), (kernel, cin, cout)
    # pack_direct: unreachable
    assert pe.direct_largest_image() == 8959 < pe.PACK_DIRECT_CAP // 29
    # lat_build_filters: 256 floats per offset at most
    assert pe.lat_packed(4096, 8, 32) == pe.LAT_BUILD_CAP < pe.lat_packed(4097, 8, 17)
    c = pe.LAT_OVER_CAP
    n_off = pe.lattice_offset_count(c["voxel"], c["radius"])
    assert n_off > 4096 and pe.lat_packed(n_off, c["cin"], c["cout"]) > pe.LAT_BUILD_CAP and c["cin"] in (4, 8) and c["cout"] <= 32
    assert pe.lattice_offset_count(0.1, 0.4) == 257  # (the models' stencil, for scale)
    L = fr.lattice_case("over_cap")
    assert "over_cap" in fr.LATTICE_CASES and (L["cin"], L["cout"], L["radius"], L["ivox"]) == (c["cin"], c["cout"], c["radius"], c["voxel"])
    print("lattice over_cap:", n_off, "offsets,", pe.lat_packed(n_off, c["cin"], c["cout"]), "packed floats")
    table = pe.packer_table()
    assert [r[0] for r in table] == ["pack_filter (lds)", "pack_filter (mfma)", "pack_filter (blk)", "pack_filter_cls", "pack_direct",
                                     "lat_build_filters"]


def test_generic_form_restatement_against_the_library():
    """The restated packed-filter counts against the library: dmcf_cconv_workspace_bytes reserves the largest packed filter of
    any form (rounded up to 256 bytes).  At Cin 65, 81, 113 and 132 that is the generic form's (lds_cfg = make_cfg: 36 blocks
    per 8-channel chunk against 64 per 16-channel chunk of the others), at Cin 4 and 24 the class-sorted form's."""
    import ctypes
    import os
    from dmcf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = _lib.lib()
    for cin, cout in ((113, 49), (65, 17), (81, 64), (4, 3), (24, 17), (132, 49)):
        a = _lib.CconvArgs()
        for d, v in enumerate((4, 4, 4, cin, cout)):
            a.filter_dims[d] = v
        a.n_out, a.n_inp, a.n_pairs, a.extent = 100, 100, 1000, 0.5
        # (no launch: the pointers are only tested for NULL and alignment)
        a.filters = a.out_positions = a.inp_positions = a.inp_features = a.neighbors_index = a.neighbors_row_splits = a.out = 1 << 20
        floats = (L.dmcf_cconv_workspace_bytes(ctypes.byref(a)) - 256) // 4
        every = [pe.lds_cfg(4, 4, 4, cin, cout)["packed_floats"], pe.mfma_packed(64, cin, cout), pe.blk_packed(cin, cout),
                 pe.cls_packed(cin, cout)]
        assert max(every) <= floats < max(every) + 64, (cin, cout, every, floats)
        assert (every[0] == max(every)) == (cin in (113, 65, 81, 132))
