"""CPU side of the PointNet edge cases (tests/neighbor_dense_edges_ref.py, tests/test_gpu_neighbor_dense_edges.py): the cases
are what they are named for, the float32 emulation of the kernels' order of operations lies inside every bar and obeys every
exact rule, seeded faults of the emulation fail them, the restated slab plan is the library's (through its host-only
workspace query), and the float64 reference agrees with tests/pointnet_ref.py.  No device is touched."""
import ctypes
import os

import numpy as np
import pytest

import neighbor_dense_edges_ref as nd
import pointnet_ref as R

F = np.float32
ALL_SMALL = [(g, n) for g in nd.SMALL_GROUPS for n in nd.case_names(g)]


# ---- the cases ------------------------------------------------------------------------------------------------------------------

def test_edge_rows_are_what_the_issue_lists():
    idx, begin, count, rs = nd.edge_rows(True)
    n = nd.EDGE_N_IN
    assert tuple(count) == nd.EDGE_LENGTHS == (0, 1, 2, 63, 64, 65, 127, 128, 129, 640, 0, 3, 5, 0, 64, 1, 130, 0, 0, 7)
    assert len(count) == 20 and n == 300 and nd.EDGE_X_ROWS == 320
    ok = (idx >= 0) & (idx < n)
    assert set(np.unique(idx[~ok])) == {-1, n, n + 7} and n + 7 < nd.EDGE_X_ROWS
    # about a tenth out of range, the two rows made out of range on purpose apart
    free = np.ones(idx.size, bool)
    free[rs[nd.ROW_130]:rs[nd.ROW_130] + 64] = False
    free[rs[nd.ROW_65]:rs[nd.ROW_65 + 1]] = False
    assert 0.05 < (~ok[free]).mean() < 0.15
    b = rs[nd.ROW_130]
    assert count[nd.ROW_130] == 130 and not ok[b:b + 64].any() and ok[b + 64:b + 130].all()
    b = rs[nd.ROW_65]
    assert count[nd.ROW_65] == 65 and not ok[b:b + 64].any() and ok[b + 64]
    # the first tile of 16 rows holds lengths 0 to 640: its rows end in every chunk from none to the tenth
    chunks = {-(-int(c) // 64) for c in count[:16]}
    assert chunks == {0, 1, 2, 3, 10}
    # the last pair of every row longer than 64 is in range (dropping it must show)
    for r in np.flatnonzero(count > 64):
        assert ok[rs[r + 1] - 1], r
    assert not idx.flags.writeable
    ia, _, ca, _ = nd.edge_rows(False)
    assert np.array_equal(ca, count) and ((ia >= 0) & (ia < n)).all()


def test_padded_rows_differ_past_their_counts_only():
    idx, begin, count, rs = nd.edge_rows(True)
    pidx, pbegin, pcount = nd.edge_rows_padded()
    assert np.array_equal(pbegin, np.arange(20) * 656) and np.array_equal(pcount, count) and pidx.shape == (20 * 656,)
    used = np.zeros(pidx.size, bool)
    for r in range(20):
        assert np.array_equal(pidx[pbegin[r]:pbegin[r] + count[r]], idx[begin[r]:begin[r] + count[r]])
        used[pbegin[r]:pbegin[r] + count[r]] = True
    assert ((pidx[~used] >= 0) & (pidx[~used] < nd.EDGE_N_IN)).all()  # one entry past a count is a valid row of x
    ra, ja = nd.pairs(idx, begin, count, nd.EDGE_N_IN)
    rb, jb = nd.pairs(pidx, pbegin, pcount, nd.EDGE_N_IN)
    assert np.array_equal(ra, rb) and np.array_equal(ja, jb)
    rc, _ = nd.pairs(pidx, pbegin, pcount, nd.EDGE_N_IN, extra=1)
    assert len(rc) == len(rb) + 20


def test_case_lists():
    assert len(nd.case_names("widths")) == 22 and len(nd.case_names("tiles")) == 14 and len(nd.case_names("slabs")) == 55
    assert len(nd.case_names("dx_rows")) == 12 and len(nd.case_names("one_hot_G")) == 5
    have_res = {w: nd.case("widths", f"{w[0]}x{w[1]}_relu")["residual"] is not None for w in nd.WIDTHS}
    have_b = {w: nd.case("widths", f"{w[0]}x{w[1]}_relu")["b"] is not None for w in nd.WIDTHS}
    assert [have_res[w] for w in nd.WIDTHS] == [i % 2 == 0 for i in range(11)]
    assert [have_b[w] for w in nd.WIDTHS] == [i % 3 != 0 for i in range(11)]
    for g, n in ALL_SMALL:
        c = nd.case(g, n)
        assert c["x"].dtype == F and c["W"].dtype == F and c["G"].dtype == F and c["idx"].dtype == np.int32
        assert c["begin"].dtype == np.int64 and c["count"].dtype == np.int32
        for a in (c["x"], c["W"], c["G"]):
            assert np.all(np.isfinite(a)) and not a.flags.writeable
            nz = np.abs(a[a != 0])
            assert nz.size == 0 or nz.min() > 1e-30  # no denormals
        assert c["n_in"] <= len(c["x"]) and nd.case(g, n) is c
    c = nd.case("widths", "64x64_relu")
    assert np.any((c["x"] == 0) & ~np.signbit(c["x"])) and np.any((c["x"] == 0) & np.signbit(c["x"]))
    assert c["n_in"] < len(c["x"])
    for n in nd.case_names("one_hot_G"):
        c = nd.case("one_hot_G", n)
        assert list(np.flatnonzero(np.any(c["G"] != 0, axis=1))) == [c["hot"]]
    for n in nd.case_names("slabs"):
        c = nd.case("slabs", n)
        assert np.all(np.any(c["G"] != 0, axis=1)) and c["count"].max() <= 5
    # the count channel: the last channel of a 64-block at cin 63, alone in a block of its own at 64 and 128
    assert {w[0] for w in nd.SLAB_WIDTHS} >= {63, 64, 128}


def test_dx_rows_walk_the_controlled_lengths():
    """The inversion of transpose(EDGE_ROWS) is EDGE_ROWS with every row sorted: the backward's gather walks rows of exactly
    the controlled lengths (their in-range pairs for the list with out-of-range entries)."""
    for kind, oob in (("inrange", False), ("oob", True)):
        c = nd.case("dx_rows", f"65x33_relu_{kind}")
        eidx, ebegin, ecount, ers = nd.edge_rows(oob)
        assert len(c["count"]) == nd.EDGE_N_IN and c["n_in"] == 20 < len(c["x"])
        back_idx, back_rs = nd.transpose(c["idx"], c["row_splits"], c["n_in"])
        _, cr = nd.aggregate(np.zeros((nd.EDGE_X_ROWS, 1)), eidx, ebegin, ecount, nd.EDGE_N_IN, False)
        assert np.array_equal(np.diff(back_rs), cr.astype(np.int64))
        if not oob:
            assert tuple(np.diff(back_rs)) == nd.EDGE_LENGTHS
        for r in range(20):
            e = eidx[ers[r]:ers[r + 1]]
            assert np.array_equal(back_idx[back_rs[r]:back_rs[r + 1]], np.sort(e[(e >= 0) & (e < nd.EDGE_N_IN)]))
        assert np.diff(back_rs).max() > 512  # ten chunks of 64


def test_transpose_is_an_involution_up_to_the_order_inside_a_row():
    rng = np.random.default_rng(4)
    idx, begin, count, rs = nd.random_rows(rng, 37, 23, 9)
    t_idx, t_rs = nd.transpose(idx, rs, 23)
    assert t_rs.shape == (24,) and t_idx.max() < 37
    b_idx, b_rs = nd.transpose(t_idx, t_rs, 37)
    tt_idx, tt_rs = nd.transpose(b_idx, b_rs, 23)
    assert np.array_equal(tt_idx, t_idx) and np.array_equal(tt_rs, t_rs)  # transposing three times is transposing once
    for r in range(37):
        e = idx[rs[r]:rs[r + 1]]
        assert np.array_equal(b_idx[b_rs[r]:b_rs[r + 1]], np.sort(e[(e >= 0) & (e < 23)]))
    # stable: inside a row of the transpose the given list's rows ascend
    for j in range(23):
        assert np.all(np.diff(t_idx[t_rs[j]:t_rs[j + 1]]) >= 0)


# ---- the reference ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("group,name", ALL_SMALL)
def test_reference_agrees_with_pointnet_ref(group, name):
    c = nd.case(group, name)
    a = (c["x"], c["W"], c["b"], c["idx"], c["row_splits"])
    ref, _ = nd.forward(c["x"], c["W"], c["b"], c["idx"], c["begin"], c["count"], c["n_in"], c["relu"], c["residual"])
    want = R.layer_reference_order(*a, n_in=c["n_in"], relu=c["relu"], residual=c["residual"])
    assert np.allclose(ref, want, rtol=1e-10, atol=1e-10)
    A, _ = nd.forward(c["x"], c["W"], c["b"], c["idx"], c["begin"], c["count"], c["n_in"], c["relu"], c["residual"], absolute=True)
    assert np.allclose(A, R.layer_abs(*a, n_in=c["n_in"], relu=c["relu"], residual=c["residual"]), rtol=1e-10, atol=1e-10)
    got = nd.backward(c["x"], c["W"], c["G"], c["idx"], c["begin"], c["count"], c["n_in"], c["relu"])
    for g, w in zip(got[:3], R.layer_backward(c["x"], c["W"], c["G"], c["idx"], c["row_splits"], n_in=c["n_in"], relu=c["relu"])):
        assert np.allclose(g, w, rtol=1e-10, atol=1e-10)
    got = nd.backward(c["x"], c["W"], c["G"], c["idx"], c["begin"], c["count"], c["n_in"], c["relu"], absolute=True)
    for g, w in zip(got[:3], R.layer_backward(c["x"], c["W"], c["G"], c["idx"], c["row_splits"], n_in=c["n_in"], relu=c["relu"],
                                              absolute=True)):
        assert np.allclose(g, w, rtol=1e-10, atol=1e-10)


def test_padded_reference_equals_the_csr_one():
    c = nd.case("widths", "65x33_relu")
    pidx, pbegin, pcount = c["padded"]
    a, _ = nd.forward(c["x"], c["W"], c["b"], c["idx"], c["begin"], c["count"], c["n_in"], True, c["residual"])
    b, _ = nd.forward(c["x"], c["W"], c["b"], pidx, pbegin, pcount, c["n_in"], True, c["residual"])
    assert np.array_equal(a, b)


# ---- the bars hold for the emulation, and are sensitive ------------------------------------------------------------------------------

@pytest.mark.parametrize("group,name", ALL_SMALL)
def test_emulation_lies_inside_the_bars(group, name):
    c = nd.case(group, name)
    got = nd.emulate(c)
    nd.check_case(c, got, group="emulation " + group)
    if group == "widths":
        pad = nd.emulate(c, padded=True)
        for k in got:
            assert np.array_equal(got[k], pad[k]), k


def test_emulation_worst_ratio_is_well_below_one():
    """A kernel that rounds as the emulation does has room: a ratio near 1 would mean a bar
    counts too few roundings."""
    for group, name in ALL_SMALL:  # (whatever ran before: every group is measured here too)
        if "emulation " + group not in nd.WORST:
            nd.check_case(nd.case(group, name), nd.emulate(nd.case(group, name)), group="emulation " + group)
    worst = {k: v for k, v in nd.WORST.items() if k.startswith("emulation")}
    print("emulation worst err/bar", {k: round(v, 4) for k, v in worst.items()})
    assert len(worst) == len(nd.SMALL_GROUPS) and all(v < 0.6 for v in worst.values())


def test_emulation_of_a_wave_that_takes_three_tiles():
    """The persistent case's builder for a device of one CU and of two (8 resident waves at 128 x 128, 32 and 64 at 8 x 16):
    2 * resident + 4 tiles, rows of 65 and 130 pairs among the short ones.  The emulation lies inside the bars; tiles whose
    sums start from those of an earlier tile do not."""
    for cin, cout, n_cu in ((8, 16, 1), (8, 16, 2), (128, 128, 1)):
        c = nd.persistent_case(cin, cout, n_cu)
        resident = nd.launch_plan(cin, cout, n_cu)[2]
        assert -(-len(c["count"]) // 16) == 2 * resident + 4
        nd.check_case(c, nd.emulate(c), group="emulation persistent")
        with pytest.raises(AssertionError):
            nd.check_case(c, nd.emulate(c, mutate="carry_S"), group="mutated")


SENSITIVE = {
    "drop_last_long": [("widths", "64x64_relu"), ("dx_rows", "65x33_lin_inrange")],
    "stop_at_64": [("widths", "5x15_lin"), ("dx_rows", "7x64_relu_inrange")],
    "bias_oob": [("widths", "2x17_relu")],
    "read_past_count": [("widths", "65x33_relu")],
    "carry_S": [("widths", "127x48_relu"), ("tiles", "n17_7x64")],
    "drop_count_channel": [("slabs", "n129_64x16"), ("slabs", "n5_128x128")],
    "drop_tail_rows": [("slabs", "n5_7x64"), ("slabs", "n133_63x17")],
}


@pytest.mark.parametrize("mutation", nd.MUTATIONS)
def test_seeded_faults_fail_the_bars(mutation):
    for group, name in SENSITIVE[mutation]:
        c = nd.case(group, name)
        nd.check_case(c, nd.emulate(c), group="emulation " + group)
        with pytest.raises(AssertionError):
            nd.check_case(c, nd.emulate(c, mutate=mutation, padded=mutation == "read_past_count"), group="mutated")
    assert set(SENSITIVE) == set(nd.MUTATIONS)


def test_exact_rules_catch_what_they_name():
    c = nd.case("widths", "64x64_relu")
    got = nd.emulate(c)
    out, dx = got["out"].copy(), got["dx"].copy()
    nd.check_exact(c, out, dx)
    bad = out.copy()
    bad[0, 0] = np.nextafter(bad[0, 0], F(np.inf))  # row 0 is empty: one ulp off the residual
    with pytest.raises(AssertionError):
        nd.check_exact(c, bad, dx)
    bad = dx.copy()
    bad[c["n_in"] + 1, 0] = F(1e-30)
    with pytest.raises(AssertionError):
        nd.check_exact(c, out, bad)
    i, k = np.argwhere(c["x"][:c["n_in"]] == 0)[0]
    bad = dx.copy()
    bad[i, k] = F(1e-30)
    with pytest.raises(AssertionError):
        nd.check_exact(c, out, bad)


# ---- the slab plan and the launch plan --------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def hip_lib():
    from dmcf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


FAKE = 1 << 20  # a non-NULL device address: the plan is made on the host and dereferences nothing


def _bwd_args(cin, cout, n_in, n_out):
    from dmcf_amd._lib import NeighborDenseBackwardArgs
    b = NeighborDenseBackwardArgs()
    b.struct_size = ctypes.sizeof(NeighborDenseBackwardArgs)
    b.flags = 1
    b.x, b.n_in, b.cin, b.cout, b.kernel = FAKE, n_in, cin, cout, FAKE
    b.grad_out, b.n_out, b.s, b.count = FAKE, n_out, FAKE, FAKE
    b.grad_kernel, b.grad_bias = FAKE, FAKE
    return b


def test_restated_slab_plan():
    assert nd.bwd_plan(1) == (4, 1) and nd.bwd_plan(4) == (4, 1) and nd.bwd_plan(5) == (8, 1)
    assert nd.bwd_plan(128) == (128, 1) and nd.bwd_plan(129) == (68, 2) and nd.bwd_plan(133) == (68, 2)
    assert nd.bwd_plan(257) == (88, 3) and nd.bwd_plan(2048 * 128) == (128, 2048)
    assert nd.bwd_plan(nd.SLAB_CAP_N_OUT) == (132, 1986)  # the cap: rows_per_slab above 128


@pytest.mark.parametrize("n_out,cin,cout", [(nd.SLAB_CAP_N_OUT, 5, 3), (129, 63, 17), (257, 128, 128), (4, 64, 16)])
def test_workspace_is_the_restated_plan(hip_lib, n_out, cin, cout):
    got = hip_lib.dmcf_neighbor_dense_backward_workspace_bytes(ctypes.byref(_bwd_args(cin, cout, 50, n_out)))
    assert got == nd.workspace_bytes(n_out, cin, cout) == 4 * nd.bwd_plan(n_out)[1] * (cin + 1) * cout
    if n_out == nd.SLAB_CAP_N_OUT:
        assert got == 4 * 1986 * 6 * 3


def test_kernel_names_switch_at_64(hip_lib):
    from dmcf_amd._lib import NeighborDenseArgs
    for cin, cout in nd.WIDTHS:
        a = NeighborDenseArgs()
        a.struct_size = ctypes.sizeof(NeighborDenseArgs)
        a.x, a.n_in, a.cin, a.cout, a.kernel = FAKE, 300, cin, cout, FAKE
        a.neighbors_index, a.neighbors_row_splits, a.n_out, a.n_pairs, a.out = FAKE, FAKE, 20, 100, FAKE
        buf = ctypes.create_string_buffer(256)
        assert hip_lib.dmcf_neighbor_dense_kernel_names(ctypes.byref(a), None, buf, 256) == 0
        assert buf.value.decode() == nd.gather_name(cin) == ("nd_gather_mfma<2>" if cin > 64 else "nd_gather_mfma<1>")


def test_restated_launch_plan():
    """256 CUs: 4 workgroups per CU at 8 x 16 (8192 resident waves), one at 128 x 128 (2048); every wave takes two tiles."""
    assert nd.launch_plan(8, 16, 256) == (6656, 4, 8192)
    assert nd.launch_plan(128, 128, 256) == (140800, 1, 2048)
    assert nd.launch_plan(16, 8, 256)[2] == 8192  # the backward's gather of the 8 x 16 layer: the roles swap
    for cin, cout in nd.PERSISTENT_WIDTHS:
        n_out, resident = nd.persistent_n_out(cin, cout, 256), nd.launch_plan(cin, cout, 256)[2]
        assert -(-n_out // 16) == 2 * resident + 4 and n_out % 16 == 5
    c = nd.persistent_case(8, 16, 2)  # (a device of two CUs: the same builder, small)
    assert len(c["count"]) == nd.persistent_n_out(8, 16, 2) and c["count"][0] == 130 and c["count"][97] == 65
    assert set(np.unique(c["count"])) == {0, 1, 2, 3, 65, 130}


def test_slab_cap_case():
    c = nd.case("slab_cap", "cap")
    n_out = nd.SLAB_CAP_N_OUT
    assert len(c["count"]) == n_out == 2048 * 128 + 5 and c["W"].shape == (5, 3) and c["count"].max() == 2
    hot = np.flatnonzero(np.any(c["G"] != 0, axis=1))
    assert {0, 131, 132, n_out - 1} <= set(hot) and 20 <= len(hot) <= 24 and np.array_equal(hot, c["hot"])
    rps, nslabs = nd.bwd_plan(n_out)
    assert (131 // rps, 132 // rps) == (0, 1) and (n_out - 1) // rps == nslabs - 1  # either side of the first slab edge; the last slab
