"""CPU side of the voxel convolution's edge cases (tests/sparse_conv_edges_ref.py, tests/test_gpu_sparse_conv_edges.py): the
cases are what they are named for, the float64 reference agrees with tests/sparse_conv_ref.py on that module's small cases, the
float32 emulation of the kernels' order of operations lies inside every bar and obeys every exact rule, seeded faults of the
emulation fail them, and the restated slab plan is the library's (through its host-only workspace query).  No device is
touched."""
import ctypes
import os

import numpy as np
import pytest

import sparse_conv_edges_ref as se
import sparse_conv_ref as sr

F = np.float32
ALL = se.all_cases()


# ---- the cases ------------------------------------------------------------------------------------------------------------------

def test_case_lists():
    assert len(se.case_names("channels")) == 32 and len(se.case_names("cells")) == 18 and len(se.case_names("rows")) == 10
    assert len(se.case_names("slabs")) == 32 and len(se.case_names("accumulate")) == 6
    assert len(set(ALL)) == len(ALL) == 98
    for g, n in ALL:
        c = se.case(g, n)
        assert se.case(g, n) is c and c["name"] == n and c["group"] == g
        c3, c4 = (c["cout"], c["cin"]) if c["flags"] & se.W_TRANSPOSED else (c["cin"], c["cout"])
        assert c["W"].shape == (*c["kernel"], c3, c4) and c["x"].shape == (len(c["col_pos"]), c["cin"])
        assert c["G"].shape == (len(c["row_pos"]), c["cout"]) and c["idx"].dtype == np.int32 and c["row_splits"].dtype == np.int64
        assert c["row_splits"][0] == 0 and c["row_splits"][-1] == len(c["idx"]) and np.all(np.diff(c["row_splits"]) >= 0)
        assert (c["out0"] is not None) == bool(c["flags"] & se.ACCUMULATE)
        for k in ("W", "x", "G", "row_pos", "col_pos", "row_scale", "col_scale", "bias", "out0", "idx", "row_splits"):
            a = c[k]
            if a is None:
                continue
            assert not a.flags.writeable, (n, k)
            if a.dtype == F:
                assert np.all(np.isfinite(a))
                nz = np.abs(a[a != 0])
                assert nz.size == 0 or nz.min() > 1e-30, (n, k)  # no denormals
        assert len(c["idx"]) <= 1600 and c["W"].size <= 130000 and len(c["row_pos"]) <= 129 and len(c["col_pos"]) <= 200
        if c["out0"] is not None:
            assert np.all(c["out0"] != 0)


@pytest.mark.parametrize("group,name", ALL + [("layers", c["name"]) for pair in se.layer_cases() for c in pair])
def test_margins_and_planned_cells(group, name):
    """Every filter coordinate is at least 0.2 from a half-integer, and the cells sparse_conv_ref.cells finds from the float32
    positions are the ones the builder planned in integers."""
    c = {c["name"]: c for pair in se.layer_cases() for c in pair}[name] if group == "layers" else se.case(group, name)
    half, lo, hi = se.margins(c)
    assert half >= 0.2
    pr = se.pairs_of(c)
    if group != "layers":
        assert np.array_equal(pr.cell, c["pair_cells"]) and c["hits"] == set(pr.cell.tolist())
    # the float32 operations of the kernel find the same cells
    P = se._params(c)
    if len(pr.i):
        assert np.array_equal(se.emulate_cells(P, pr.i, pr.j), pr.cell)


CHANNEL_PLANS = {  # (Cin, Cout): (cpc, ncc, 16-column tiles, passes over the list, dW chunks, batch)
    (1, 1): (60, 1, 1, 1, 1, 256), (3, 5): (60, 1, 1, 1, 1, 256), (4, 16): (60, 1, 1, 1, 1, 204), (5, 17): (30, 1, 2, 1, 1, 186),
    (16, 15): (15, 1, 1, 1, 1, 132), (33, 64): (6, 1, 4, 1, 3, 42), (60, 65): (4, 1, 5, 2, 4, 32), (61, 3): (3, 1, 1, 1, 1, 64),
    (120, 7): (2, 1, 1, 1, 1, 32), (121, 4): (1, 1, 1, 1, 1, 32), (240, 16): (1, 1, 1, 1, 4, 16), (241, 9): (1, 2, 1, 1, 3, 16),
    (243, 5): (1, 2, 1, 1, 2, 16), (481, 6): (1, 3, 1, 1, 3, 8), (7, 129): (30, 1, 9, 3, 1, 30), (65, 241): (3, 1, 16, 4, 16, 13),
}


def test_channel_cases():
    assert set(CHANNEL_PLANS) == set(se.CHANNELS)
    for name in se.case_names("channels"):
        c = se.case("channels", name)
        p = se.fwd_plan(c["cin"], c["cout"], c["K"])
        _, nslabs, batch, chunks, _ = se.slab_plan(len(c["idx"]), c["W"].shape)
        assert (p["cpc"], p["ncc"], p["col_tiles"], p["passes"], chunks, batch) == CHANNEL_PLANS[(c["cin"], c["cout"])], name
        assert nslabs == 1 and c["kernel"] == (2, 2, 2) and c["flags"] in (0, se.W_TRANSPOSED)
        assert len(c["row_pos"]) == 40 and len(c["col_pos"]) == 40 and c["bias"] is not None
        assert c["row_scale"] is not None and c["col_scale"] is not None
        cnt = np.diff(c["row_splits"])
        assert cnt.min() == 0 and cnt.max() == 12 and cnt[0] > 0 and cnt[-1] > 0 and c["hits"] == set(range(8))
        # the feature gradient's plan is the forward's with the channels swapped: it too meets more than 64 on either side
        q = se.fwd_plan(c["cout"], c["cin"], c["K"])
        assert q["col_tiles"] == -(-c["cin"] // 16)
    c = se.case("channels", "65x241_cpc3_ncc1_nt16_f0")
    assert c["W"].size == 125320 and 65 * 241 == 15665 and all((cell * 15665) % 8192 for cell in range(1, 8))
    # a last channel chunk with one real channel
    assert 241 - 240 == 1 and 481 - 2 * 240 == 1 and se.fwd_plan(481, 6, 8)["CW"] == 240
    # the same list under both flags; the filter is stored the other way round
    a, b = se.case("channels", "5x17_cpc30_ncc1_nt2_f0"), se.case("channels", "5x17_cpc30_ncc1_nt2_f2")
    assert np.array_equal(a["idx"], b["idx"]) and a["W"].shape[3:] == (5, 17) and b["W"].shape[3:] == (17, 5)


CELL_PLANS = {  # (Cin, kernel): (K, cpc, cell chunks)
    (32, (1, 1, 7)): (7, 7, 1), (32, (2, 2, 2)): (8, 7, 2), (32, (1, 2, 7)): (14, 7, 2), (32, (1, 3, 5)): (15, 7, 3),
    (5, (3, 3, 3)): (27, 30, 1), (5, (2, 3, 5)): (30, 30, 1), (5, (1, 1, 31)): (31, 30, 2), (5, (4, 4, 4)): (64, 30, 3),
    (1, (3, 4, 5)): (60, 60, 1), (1, (4, 4, 4)): (64, 60, 2), (1, (5, 5, 5)): (125, 60, 3),
}


def test_cell_cases():
    assert set(CELL_PLANS) == set(se.CELLS)
    seen_flags = set()
    for name in se.case_names("cells"):
        c = se.case("cells", name)
        p = se.fwd_plan(c["cin"], c["cout"], c["K"])
        K, cpc, chunks = CELL_PLANS[(c["cin"], c["kernel"])]
        assert (c["K"], p["cpc"], p["cell_chunks"]) == (K, cpc, chunks) and p["ncc"] == 1, name
        assert c["hits"] == set(range(K)), name  # every cell
        pr = se.pairs_of(c)
        for e in range(cpc, K, cpc):  # the two cells at every chunk edge, from one row
            rows = set(pr.i[pr.cell == e - 1]) & set(pr.i[pr.cell == e])
            assert rows, (name, e)
        _, lo, hi = se.margins(c)
        many = np.asarray(c["kernel"][::-1]) > 1
        assert np.array_equal(lo, many) and np.array_equal(hi, many), name  # the clamp, at both ends of every axis with cells
        assert (np.diff(c["row_splits"]) == 0).sum() >= 2
        if c["kernel"] in ((2, 3, 5), (3, 4, 5)):
            assert len(set(c["offset"])) == 3 and not np.any(c["offset"] == 0)
        if c["kernel"] == (2, 3, 5):
            seen_flags.add(c["flags"])
    assert seen_flags == set(range(8))


def test_row_cases():
    for n in se.ROWS_N:
        c = se.case("rows", f"n{n}")
        cnt = np.diff(c["row_splits"])
        assert len(cnt) == n and cnt[0] > 0 and cnt[-1] > 0 and (c["cin"], c["cout"], c["kernel"]) == (5, 7, (2, 3, 5))
    assert se.ROWS_N == (1, 15, 16, 17, 63, 64, 65, 129)
    a, b = se.case("rows", "lengths"), se.case("rows", "lengths_oob")
    assert tuple(np.diff(a["row_splits"])) == tuple(np.diff(b["row_splits"])) == se.ROW_LENGTHS
    assert se.ROW_LENGTHS[:13] == (0, 1, 2, 3, 4, 5, 63, 64, 65, 300, 0, 0, 7) and len(se.ROW_LENGTHS) == 20
    n_cols = len(a["col_pos"])
    assert ((a["idx"] >= 0) & (a["idx"] < n_cols)).all()
    for c in (a, b):
        rs, n_cols = c["row_splits"], len(c["col_pos"])
        ok = (c["idx"] >= 0) & (c["idx"] < n_cols)
        pr = se.pairs_of(c)
        assert len(set(pr.cell[pr.i == se.ROW_300])) == 1 and len(set(pr.j[pr.i == se.ROW_300])) == 6  # one cell, six columns
        r40 = c["idx"][rs[se.ROW_40]:rs[se.ROW_40 + 1]]
        assert len(r40) == 40 and len(set(r40[(r40 >= 0) & (r40 < n_cols)])) == 1
        for r in np.flatnonzero(np.diff(rs) > 0):
            assert ok[rs[r + 1] - 1] or r == se.ROW_ALL_BAD  # the last entry of a row is in range: dropping it must show
    rs, n_cols = b["row_splits"], len(b["col_pos"])
    ok = (b["idx"] >= 0) & (b["idx"] < n_cols)
    assert set(np.unique(b["idx"][~ok])) == {-1, n_cols, n_cols + 7}
    free = np.ones(len(ok), bool)
    for r in (se.ROW_ALL_BAD, se.ROW_LAST_ONLY):
        free[rs[r]:rs[r + 1]] = False
    assert 0.05 < (~ok[free]).mean() < 0.15
    assert not ok[rs[se.ROW_ALL_BAD]:rs[se.ROW_ALL_BAD + 1]].any() and rs[se.ROW_ALL_BAD + 1] - rs[se.ROW_ALL_BAD] == 5
    last = ok[rs[se.ROW_LAST_ONLY]:rs[se.ROW_LAST_ONLY + 1]]
    assert len(last) == 7 and not last[:-1].any() and last[-1]
    # the first tile holds rows of 0 to 300 pairs; the list has a second tile
    assert max(se.ROW_LENGTHS[:16]) == 300 and max(se.ROW_LENGTHS[16:]) == 7
    # the plans: one image chunk of 30 cells of 8 channels, one column tile; the 579 entries of the lengths make two slabs
    for name in se.case_names("rows"):
        c = se.case("rows", name)
        p = se.fwd_plan(5, 7, 30)
        assert (p["cpc"], p["ncc"], p["cell_chunks"], p["col_tiles"]) == (30, 1, 1, 1)
        assert se.slab_plan(len(c["idx"]), c["W"].shape)[1:4] == (2 if name.startswith("lengths") else 1, 256, 1), name
    assert len(a["idx"]) == 579


SLAB_COUNTS = {1: 1, 255: 1, 256: 1, 257: 1, 511: 1, 512: 1, 513: 2, 1024: 2, 1025: 3, 1537: 4}
SLAB_BATCH = {(5, 7): 256, (4, 13): 240, (65, 241): 13}
SLAB_CHUNKS = {(5, 7): 1, (4, 13): 1, (65, 241): 16}


def test_slab_cases():
    assert tuple(SLAB_COUNTS) == se.SLAB_PAIRS and tuple(SLAB_BATCH) == se.SLAB_WIDTHS
    for name in se.case_names("slabs"):
        c = se.case("slabs", name)
        slab_pairs, nslabs, batch, chunks, _ = se.slab_plan(len(c["idx"]), c["W"].shape)
        w = (c["cin"], c["cout"])
        assert slab_pairs == 512 and nslabs == SLAB_COUNTS[len(c["idx"])] and batch == SLAB_BATCH[w] and chunks == SLAB_CHUNKS[w], name
        assert c["only"] == ("dW",) and int(name.split("_")[0][1:]) == len(c["idx"])
    c = se.case("slabs", "p1537_5x7_dead_slab")
    ok = (c["idx"] >= 0) & (c["idx"] < 40)
    assert not ok[512:1024].any() and ok[:512].all() and ok[1024:].all()
    c = se.case("slabs", "p1025_5x7_cell_in_second_slab")
    _, _, pos = se._in_range(c)
    at7 = pos[c["pair_cells"] == 7]
    assert len(at7) > 20 and at7.min() >= 512 and at7.max() < 1024 and 7 in c["hits"]
    # batches: 255, 256 and 257 pairs either side of one batch of 256; 240 and 13 divide none of the slab sizes
    assert 512 % 240 and 512 % 13 and 257 - 256 == 1


def test_accumulate_cases():
    for name in se.case_names("accumulate"):
        c = se.case("accumulate", name)
        assert (c["bias"] is None) == ("nobias" in name)
        if name.startswith("no_pairs"):
            assert len(c["idx"]) == 0 and not c["row_splits"].any() and len(c["row_pos"]) == 40
        else:
            assert (np.diff(c["row_splits"]) == 0).any()


def test_transpose_is_an_involution_up_to_the_order_inside_a_row():
    c = se.case("rows", "lengths_oob")
    n_rows, n_cols = len(c["row_pos"]), len(c["col_pos"])
    t_idx, t_rs = se.transpose(c["idx"], c["row_splits"], n_cols)
    assert t_rs.shape == (n_cols + 1,) and t_idx.max() < n_rows and t_idx.dtype == np.int32 and t_rs.dtype == np.int64
    b_idx, b_rs = se.transpose(t_idx, t_rs, n_rows)
    for r in range(n_rows):
        e = c["idx"][c["row_splits"][r]:c["row_splits"][r + 1]]
        assert np.array_equal(b_idx[b_rs[r]:b_rs[r + 1]], np.sort(e[(e >= 0) & (e < n_cols)]))
    for j in range(n_cols):
        assert np.all(np.diff(t_idx[t_rs[j]:t_rs[j + 1]]) >= 0)
    assert t_rs[-1] == ((c["idx"] >= 0) & (c["idx"] < n_cols)).sum()


# ---- the reference ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("transpose", [False, True], ids=["conv", "transpose"])
@pytest.mark.parametrize("name", [c.name for c in sr.small_cases()])
def test_reference_agrees_with_sparse_conv_ref(name, transpose):
    old = {c.name: c for c in sr.small_cases()}[name]
    c = se.from_sparse_conv_ref(old, transpose)
    R = se.reference(c)
    ref, A = old.forward(transpose)
    assert np.allclose(R["out"][0], ref, rtol=1e-10, atol=1e-10) and np.allclose(R["out"][1], A, rtol=1e-10, atol=1e-10)
    (dW, aW), (dF, aF), _, _ = old.grads(transpose)
    for got, want in ((R["dW"], (dW, aW)), (R["dF"], (dF, aF))):
        assert np.allclose(got[0], want[0], rtol=1e-10, atol=1e-10) and np.allclose(got[1], want[1], rtol=1e-10, atol=1e-10)
    # the new bars never exceed the old one
    k_out, k_dF, k_dW = se.bar_factors(c)
    assert k_out.max() <= old.kbar(transpose) and k_dW.max() <= old.kbar(transpose)
    assert k_dF.max() <= old.kbar(transpose, chain_channels=old.cout, columns=True)
    # and the emulation, on the layers' own shapes, lies inside them
    if name in ("k2_c1", "k122_planar_offset_xy_c5x7"):
        se.check_case(c, se.emulate(c), group="emulation sparse_conv_ref")


def test_w_transposed_and_negate_in_the_reference():
    """W_TRANSPOSED with the filter stored the other way round is the plain call; NEGATE with the columns mirrored through
    their rows' common point is the plain call."""
    c = se.case("cells", "c5_k2x3x5_K30_cpc30_f0")
    R = se.reference(c)
    t = se.derive(c, "t", flags=se.W_TRANSPOSED, W=np.ascontiguousarray(c["W"].swapaxes(3, 4)))
    T = se.reference(t)
    same = lambda a, b: np.allclose(a, b, rtol=1e-12, atol=1e-12)  # noqa: E731
    assert same(T["out"][0], R["out"][0]) and same(T["dF"][0], R["dF"][0]) and same(T["dW"][0], R["dW"][0].swapaxes(3, 4))
    one = se.derive(c, "one", row_pos=np.zeros_like(c["row_pos"]))
    neg = se.derive(one, "neg", flags=se.NEGATE, col_pos=-c["col_pos"])
    assert same(se.reference(neg)["out"][0], se.reference(one)["out"][0])
    assert not np.allclose(se.reference(se.derive(c, "n", flags=se.NEGATE))["out"][0], R["out"][0], rtol=1e-3, atol=1e-3)


def test_bars_never_exceed_the_old_one():
    for g, n in ALL:
        c = se.case(g, n)
        pr = se.pairs_of(c)
        k_out, k_dF, k_dW = se.bar_factors(c)
        old_rows = max(256, pr.longest_row() + c["K"] * c["cin"] + 64)
        assert k_out.max() <= old_rows and k_dW.max() <= old_rows and k_dF.max() <= max(256, pr.longest_col() + c["K"] * c["cout"] + 64)
        assert k_out.min() >= 4 and k_dW.min() >= 4
    c = se.case("channels", "1x1_cpc60_ncc1_nt1_f0")
    k_out, _, k_dW = se.bar_factors(c)
    L = np.diff(c["row_splits"])
    assert np.array_equal(k_out, L + np.minimum(8, L) * 4 + 4) and k_out.max() == 12 + 8 * 4 + 4
    assert np.array_equal(k_dW, np.bincount(c["pair_cells"], minlength=8) + 1 + 3)


# ---- the bars hold for the emulation, and are sensitive ------------------------------------------------------------------------------

@pytest.mark.parametrize("group,name", ALL)
def test_emulation_lies_inside_the_bars(group, name):
    c = se.case(group, name)
    se.check_case(c, se.emulate(c), group="emulation " + group)


def test_emulation_worst_ratio_is_well_below_one():
    """A kernel that rounds as the emulation does has room: a ratio near 1 would mean a bar counts too few roundings."""
    for group, name in ALL:  # (whatever ran before: every group is measured here too)
        if not any(k[0] == "emulation " + group for k in se.WORST):
            se.check_case(se.case(group, name), se.emulate(se.case(group, name)), group="emulation " + group)
    worst = {k: v for k, v in se.WORST.items() if k[0].startswith("emulation") and k[0] != "emulation sparse_conv_ref"}
    print("emulation worst err/bar", {f"{k[0][10:]} {k[1]}": round(v, 4) for k, v in worst.items()})
    assert {k[0][10:] for k in worst} == set(se.GROUPS) and all(v < 0.6 for v in worst.values())


SENSITIVE = {
    "drop_second_channel_chunk": [("channels", "241x9_cpc1_ncc2_nt1_f0"), ("channels", "481x6_cpc1_ncc3_nt1_f2")],
    "drop_last_cell_chunk": [("cells", "c32_k2x2x2_K8_cpc7_f0"), ("cells", "c1_k5x5x5_K125_cpc60_f0")],
    "carry_acc_across_column_passes": [("channels", "7x129_cpc30_ncc1_nt9_f0"), ("channels", "60x65_cpc4_ncc1_nt5_f2")],
    "stop_at_cout_64": [("channels", "60x65_cpc4_ncc1_nt5_f0"), ("channels", "65x241_cpc3_ncc1_nt16_f2")],
    "read_past_cin": [("channels", "241x9_cpc1_ncc2_nt1_f0"), ("channels", "5x17_cpc30_ncc1_nt2_f2")],
    "swap_ky_kx": [("cells", "c5_k2x3x5_K30_cpc30_f0"), ("cells", "c1_k3x4x5_K60_cpc60_f0")],
    "ignore_negate": [("cells", "c5_k2x3x5_K30_cpc30_f1"), ("accumulate", "bias_negate_transposed_f7")],
    "filter_grad_ignores_transposed": [("channels", "3x5_cpc60_ncc1_nt1_f2"), ("cells", "c5_k2x3x5_K30_cpc30_f2")],
    "drop_cell_part_across_dw_chunk": [("channels", "65x241_cpc3_ncc1_nt16_f0"), ("slabs", "p513_65x241_batch13")],
    "drop_last_batch": [("slabs", "p257_5x7_batch256"), ("slabs", "p255_4x13_batch240")],
    "drop_last_slab": [("slabs", "p513_5x7_batch256"), ("slabs", "p1025_65x241_batch13")],
    "keep_out_of_range_pairs": [("rows", "lengths_oob"), ("slabs", "p1537_5x7_dead_slab")],
    "accumulate_overwrites": [("accumulate", "bias_f4"), ("cells", "c5_k2x3x5_K30_cpc30_f4")],
}


@pytest.mark.parametrize("mutation", se.MUTATIONS)
def test_seeded_faults_fail_the_bars(mutation):
    for group, name in SENSITIVE[mutation]:
        c = se.case(group, name)
        se.check_case(c, se.emulate(c), group="emulation " + group)
        with pytest.raises(AssertionError):
            se.check_case(c, se.emulate(c, mutate=mutation), group="mutated")
    assert set(SENSITIVE) == set(se.MUTATIONS)


def test_exact_rules_catch_what_they_name():
    c = se.case("accumulate", "bias_f4")
    got = se.emulate(c)
    se.check_exact(c, got)
    empty = int(np.flatnonzero(np.diff(c["row_splits"]) == 0)[0])
    full = int(np.flatnonzero(np.diff(c["row_splits"]) > 0)[0])
    for r in (empty, full):  # one ulp off: out0 + bias in the empty row, float32(plain + out0) in the other
        bad = dict(got, out=got["out"].copy())
        bad["out"][r, 0] = np.nextafter(bad["out"][r, 0], F(np.inf))
        with pytest.raises(AssertionError):
            se.check_exact(c, bad)
    c = se.case("slabs", "p1_5x7_batch256")
    got = se.emulate(c)
    se.check_exact(c, got)
    bad = dict(dW=got["dW"].copy())
    cell = min(set(range(8)) - c["hits"])
    bad["dW"].reshape(8, -1)[cell, 3] = F(1e-30)
    with pytest.raises(AssertionError):
        se.check_exact(c, bad)
    c = se.case("channels", "3x5_cpc60_ncc1_nt1_f0")
    got = se.emulate(c)
    lonely = np.flatnonzero(np.bincount(se.pairs_of(c).j, minlength=40) == 0)
    assert 39 in lonely
    bad = dict(got, dF=got["dF"].copy())
    bad["dF"][39, 0] = F(1e-30)
    with pytest.raises(AssertionError):
        se.check_exact(c, bad)


# ---- the slab plan ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def hip_lib():
    from dmcf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


FAKE = 1 << 20  # a non-NULL device address: the plan is made on the host and dereferences nothing


def _args(dims, n_pairs, n_rows=40, n_cols=40):
    from dmcf_amd._lib import SparseConvArgs
    a = SparseConvArgs()
    a.struct_size = ctypes.sizeof(SparseConvArgs)
    for k in range(5):
        a.filter_dims[k] = dims[k]
    a.extent = 1.0
    a.filters, a.row_positions, a.col_positions, a.col_features = FAKE, FAKE, FAKE, FAKE
    a.neighbors_index, a.neighbors_row_splits = FAKE, FAKE
    a.n_rows, a.n_cols, a.n_pairs = n_rows, n_cols, n_pairs
    return a


def test_restated_slab_plan():
    d = (2, 2, 2, 5, 7)
    assert se.slab_plan(0, d)[:4] == (512, 1, 256, 1) and se.slab_plan(1, d)[:2] == (512, 1)
    assert se.slab_plan(512, d)[:2] == (512, 1) and se.slab_plan(513, d)[:2] == (512, 2)
    assert se.slab_plan(262144, d)[:2] == (512, 512) and se.slab_plan(262145, d)[:2] == (513, 512)
    assert se.slab_plan(1000000, d)[:2] == (1954, 512)
    assert se.slab_plan(513, (2, 2, 2, 65, 241))[2:] == (13, 16, 3 * 2304 + se._up(2 * 125320 * 4, 256))
    assert se.slab_plan(1, (2, 2, 2, 4, 13))[2] == 240


@pytest.mark.parametrize("dims", [(2, 3, 5, 5, 7), (2, 2, 2, 65, 241)])
@pytest.mark.parametrize("n_pairs", [0, 1, 512, 513, 262144, 262145, 1000000])
def test_workspace_is_the_restated_plan(hip_lib, dims, n_pairs):
    got = hip_lib.dmcf_sparse_conv_backward_workspace_bytes(ctypes.byref(_args(dims, n_pairs)), 1)
    slab_pairs, nslabs, _, _, nbytes = se.slab_plan(n_pairs, dims)
    per = -(-max(n_pairs, 1) * 4 // 256) * 256
    assert got == nbytes and nbytes >= 3 * per + nslabs * int(np.prod(dims)) * 4 and nslabs * slab_pairs >= n_pairs
    assert hip_lib.dmcf_sparse_conv_backward_workspace_bytes(ctypes.byref(_args(dims, n_pairs)), 0) == 0


def test_filter_gradient_refuses_more_than_4096_staged_channels(hip_lib):
    """Cin + Cout above 4096: DMCF_EUNSUPPORTED for the filter gradient, decided on the host after the argument checks and
    before the workspace is looked at or anything is launched (nothing is dereferenced: every address here is fake); the
    feature gradient alone is not refused for it."""
    b = hip_lib.dmcf_sparse_conv_backward
    a = _args((1, 1, 1, 4000, 97), 8)
    assert b(ctypes.byref(a), FAKE, None, None, 0, FAKE, None, None, 0, None) == -4
    a = _args((1, 1, 1, 97, 4000), 8)
    assert b(ctypes.byref(a), FAKE, FAKE, FAKE, 8, FAKE, FAKE, None, 0, None) == -4
    a = _args((1, 1, 1, 4000, 96), 8)
    assert b(ctypes.byref(a), FAKE, None, None, 0, FAKE, None, None, 0, None) == -2  # supported: the missing workspace is next
