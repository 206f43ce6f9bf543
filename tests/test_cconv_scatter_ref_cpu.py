"""The scatter form's error bar of tests/cconv_scatter_ref.py on the CPU: it is sound (the float32 oracle is within its float part
on every case tests/test_gpu_cconv_scatter_bar.py runs, a numpy emulation of the kernel's fixed-point sum within the whole), its
conditions hold, the cases hold what they claim, and it has teeth (the 2^30 scale the kernel first had fails the outlier case;
seeded faults break it).  The library's reach (dmcf_cconv_scatter_reach, and ops.scatter_reach over it) agrees with the plan's
expression as cconv_scatter_ref restates it, and its table of instantiations and box limits (dmcf_cconv_scatter_kernel_name)
with expected_kernel / two_workgroups."""
import ctypes
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import cconv_scatter_ref as sr  # noqa: E402

MATRIX = sr.matrix()
_CASES = {}
OK, EINVAL, EUNSUPPORTED = 0, -1, -4  # DMCF_* of include/dmcf_hip.h


@pytest.fixture(scope="module")
def hip_lib():
    from dmcf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def _case(spec):
    key = tuple(sorted(spec.items()))
    if key not in _CASES:
        _CASES[key] = sr.Case(**spec)
    return _CASES[key]


@pytest.mark.parametrize("cid,spec", MATRIX, ids=[m[0] for m in MATRIX])
def test_float32_oracle_is_within_the_float_part_of_the_bar(oracle, cid, spec):
    c = _case(spec)
    sr.check("oracle32", c.oracle32(), c, fixed_term=False)


@pytest.mark.parametrize("cid,spec", MATRIX, ids=[m[0] for m in MATRIX])
def test_conditions_on_the_case(oracle, cid, spec):
    """The fixed-point term is at most 1 / 16 of the float part (with its floor) on every element; every n_i < 2^16; every row
    is compared; the lists hold the same pairs; a cut list cuts a row that is not empty; the exact rows exist."""
    from dmcf_amd import ops
    c = _case(spec)
    want, bound, fixed = c.bar()
    assert want.shape == bound.shape == fixed.shape == (c.out_pos.shape[0], c.cout)  # (no row left out: check() takes them all)
    assert np.all(fixed <= sr.MAX_SHARE * c.float_bar())
    assert c.n_pairs.max() < 2 ** 16 and c.n_pairs.max() < 1000
    assert c.t_rs[-1] == c.full_rs[-1] == c.t_idx.shape[0]
    i = np.repeat(np.arange(c.out_pos.shape[0]), np.diff(c.full_rs))
    j = np.repeat(np.arange(c.inp_pos.shape[0]), c.t_counts)
    assert np.array_equal(np.sort(i * 10 ** 6 + c.full_idx), np.sort(c.t_idx.astype(np.int64) * 10 ** 6 + j))
    if c.form == "cut":
        assert c.cut >= 2 and c.cut_rows.sum() >= 1 and c.idx.shape[0] < c.full_idx.shape[0]
        assert np.all(c.p_begin[:-1][c.cut_rows] + c.p_cnt[c.cut_rows] > c.p_idx.shape[0])
        assert not np.isin(c.idx, np.flatnonzero(c.cut_rows)).any()
        # one cut row begins inside the buffer and reaches past its end; the others begin at or past the end
        inside = c.p_begin[:-1][c.cut_rows] < c.p_idx.shape[0]
        assert inside.sum() == 1 and (~inside).sum() >= 1
    else:
        assert c.idx.shape[0] == c.full_idx.shape[0]
        # the probes' transposed rows, the lone pair at R / 2 and the pair at the window's edge
        assert {L: int(c.t_counts[p]) for L, p in c.scene.probes.items()} == {L: L for L in c.scene.probes}
        assert set(c.scene.probes) == set(L for L in sr.ROW_LENGTHS if L <= {2: 2, 3: 65, 4: 257}[c.reach])
        for (p, cell), at in ((c.scene.single, 0.5), (c.scene.edge, 0.9995)):
            row = int(np.flatnonzero(np.all(c.scene.cells == cell, axis=1))[0])
            assert c.n_pairs[row] == 1 and c.idx[c.rs[row]] == p
            d = np.linalg.norm(c.inp_pos[p].astype(np.float64) - c.out_pos[row]) / c.radius
            assert abs(d - at) < 2e-4 * (60 if c.offset else 1), d
    # rows no particle reaches (out[0], the plan's origin, among them); the blocks' populations
    assert 0 in c.scene.empty_rows and np.all(c.n_pairs[c.scene.empty_rows] == 0)
    u = c.scene.parts / c.m
    for n, anchor in c.scene.populations.items():
        inside = np.all((u >= anchor / c.m) & (u < anchor / c.m + 1), axis=1)
        around = np.all((u >= anchor / c.m - 1) & (u < anchor / c.m + 2), axis=1)
        assert inside.sum() == n == around.sum()
    assert set(c.scene.populations) == set(sr.POPULATIONS)
    if c.interior:
        assert np.all(np.floor(u).min(axis=0) < -1) and np.all(np.floor(u).max(axis=0) >= 0)  # block coordinates of both signs
    if c.strays:
        assert len(c.scene.strays) == 6 and np.all(np.abs(c.scene.parts[c.scene.strays]).max(axis=1) > 64 * 4 + 64)
        assert np.all(c.t_counts[c.scene.strays] > 0)
    if c.outlier:
        p = c.scene.outlier
        assert 0 < c.t_counts[p] <= 3 and np.abs(c.feat[p]).max() == np.abs(c.feat).max() > 2 ** 8 * np.abs(np.delete(c.feat, p, 0)).max()
    assert c.reach == sr.expected_reach(c.radius, c.voxel) == ops.scatter_reach(c.radius, c.voxel)
    assert c.kernel == ops.scatter_kernel_name(c.cout, c.m, c.reach) and ops.cconv_scatter_supported(c.filt, c.m, c.reach)


def test_matrix_covers_what_the_bar_file_claims():
    specs = [dict(sr.Case.DEFAULTS, **s) for _, s in MATRIX]
    assert 36 <= len(specs) <= 44
    names = {sr.expected_kernel(s["cout"], s["m"], sr.KINDS[s["kind"]][2]) for s in specs}
    assert names == {"cconv_sct_kernel<4, 8>", "cconv_sct_kernel<4, 16>", "cconv_sct_kernel<8, 8>"}
    two = {sr.two_workgroups(8, s["m"], sr.KINDS[s["kind"]][2]) for s in specs if s["cout"] == 8}
    assert two == {True, False}
    assert {s["cin"] for s in specs} == set(sr.CINS) and {s["m"] for s in specs} == {1, 2, 4}
    assert {s["kind"] for s in specs} == set(sr.KINDS) and {s["form"] for s in specs} == {"csr", "padded", "cut"}
    for name in names:  # every instantiation with every list form, window, option
        mine = [s for s in specs if sr.expected_kernel(s["cout"], s["m"], sr.KINDS[s["kind"]][2]) == name]
        assert {s["form"] for s in mine} == {"csr", "padded", "cut"} and {s["window"] for s in mine} == {None, "poly6"}
        assert {s["bias"] for s in mine} == {s["accumulate"] for s in mine} == {True, False}
        assert any(s["window"] == "poly6" and s["window_fac"] == 0.5 for s in mine)
    for key in ("strays", "outlier"):
        assert sum(1 for s in specs if s[key]) >= 2
    assert any(s["offset"] == 60.0 for s in specs) and any(not s["interior"] for s in specs) and any(s["interior"] for s in specs)
    assert any(s["zero_channel"] is not None and s["bias"] for s in specs)
    assert not sr.Case.DEFAULTS["accumulate"] and not sr.IDENTITY.get("accumulate")


@pytest.mark.parametrize("cid,spec", MATRIX, ids=[m[0] for m in MATRIX])
def test_fixed_point_emulation_is_within_the_bar(oracle, cid, spec):
    """Per-pair float64 terms rounded to 2^-s and added as integers, 2^s b <= 2^46: inside the bar on every case; exact rows
    exact."""
    c = _case(spec)
    y = c.fixed_point_emulation()
    sr.check("emulation", y, c)
    empty = c.n_pairs == 0
    assert empty.sum() >= len(sr.EMPTY_CELLS) and np.array_equal(y[empty], c.exact_rows_value()[empty])


def test_a_scale_of_2_to_the_30_fails_the_outlier_case(oracle):
    """What the kernel first had: one particle with features 2^10 times the rest sets a bound whose 2^-30 is more than the bar of
    the rows that hold a small term (the pair at the window's edge)."""
    c = _case(sr.OUTLIER)
    assert sr.within_bar(c.fixed_point_emulation(46), c)
    assert not sr.within_bar(c.fixed_point_emulation(30), c)
    plain = _case(sr.IDENTITY)
    assert sr.within_bar(plain.fixed_point_emulation(30), plain), "without the outlier 2^30 was enough: the case is what finds it"


def test_dropping_the_single_pair_breaks_the_bar(oracle):
    c = _case(sr.IDENTITY)
    p, cell = c.scene.single
    row = int(np.flatnonzero(np.all(c.scene.cells == cell, axis=1))[0])
    assert c.t_counts[p] == 1 and c.n_pairs[row] == 1
    rs = c.rs.copy()
    rs[row + 1:] -= 1
    assert sr.within_bar(c.oracle32(), c, fixed_term=False)
    assert not sr.within_bar(c.oracle32(np.delete(c.idx, c.rs[row]), rs), c)


def test_bias_missing_on_the_rows_without_pairs_breaks_the_bar(oracle):
    c = _case(sr.IDENTITY)
    assert c.bias_v is not None and (c.n_pairs == 0).any()
    assert not sr.within_bar(c.oracle32(bias_rows=c.n_pairs > 0), c)


def test_reach_agrees_with_the_plan(hip_lib):
    """dmcf_cconv_scatter_reach, called directly and through ops.scatter_reach, against ceilf(0.5f * extent / voxel - 1e-4f) of
    dmcf_cconv_scatter_plan as cconv_scatter_ref restates it, +-400 ulp around the radii at which the ceiling steps."""
    from dmcf_amd import ops
    n = 0
    for voxel in (0.05, 0.1, 0.125, 0.2, 0.3):
        for k in range(1, 6):
            r = np.float32(k * voxel * (1 + 1e-4 / k))
            for _ in range(400):
                r = np.nextafter(r, np.float32(0))
            seen = set()
            for _ in range(801):
                a, b = ops.scatter_reach(float(r), voxel), sr.expected_reach(float(r), voxel)
                assert a == b, (float(r), voxel, a, b)
                direct = hip_lib.dmcf_cconv_scatter_reach(2.0 * float(r), voxel)
                assert direct == b, (float(r), voxel, direct, b)
                seen.add(a)
                r = np.nextafter(r, np.float32(np.inf))
                n += 1
            assert seen == {k, k + 1}, "the sweep does not straddle the step of the ceiling"
    assert n == 5 * 5 * 801


def test_reach_refuses_what_is_not_a_length(hip_lib):
    """0 for an extent or a voxel that is not positive and finite."""
    from dmcf_amd import ops
    nan, inf = float("nan"), float("inf")
    for extent, voxel in ((0.0, 0.1), (-0.8, 0.1), (0.8, 0.0), (0.8, -0.1), (-0.8, -0.1), (nan, 0.1), (0.8, nan), (nan, nan),
                          (inf, 0.1), (0.8, inf), (inf, inf)):
        assert hip_lib.dmcf_cconv_scatter_reach(extent, voxel) == 0, (extent, voxel)
        assert ops.scatter_reach(extent / 2, voxel) == 0, (extent, voxel)
    assert hip_lib.dmcf_cconv_scatter_reach(0.8, 0.1) == 4 and ops.scatter_reach(0.4, 0.1) == 4


def test_reach_where_a_float64_subtraction_steps_early():
    """The radius at which the wrapper's former expression parted from the plan's when numpy subtracted the 1e-4 in float64 (its
    scalar arithmetic before 2.0): 0.40001002 / 0.1 - 1e-4 is 4 + 1.4e-7 in float64, which the ceiling takes to 5, and exactly 4
    in float32, the plan's arithmetic.  A call with the 5 sized its box for a plan whose header said 4."""
    from dmcf_amd import ops
    radius, voxel = float(np.float32(0.40001002)), 0.1
    q = np.float32(radius) / np.float32(voxel)
    assert int(np.ceil(np.float64(q) - 1e-4)) == 5 and int(np.ceil(np.float32(q - np.float32(1e-4)))) == 4
    assert ops.scatter_reach(radius, voxel) == sr.expected_reach(radius, voxel) == 4


def _kernel_name(hip_lib, dims, block_cells, reach, size=64):
    name = ctypes.create_string_buffer(size) if size else None
    rc = hip_lib.dmcf_cconv_scatter_kernel_name((ctypes.c_int32 * 5)(*dims), block_cells, reach, name, size)
    return rc, (name.value.decode() if size else None)


def test_kernel_name_and_box_limits(hip_lib):
    """dmcf_cconv_scatter_kernel_name over cout 4 / 8, block_cells 1 .. 6, reach 1 .. 5 (D = 4 .. 17, both sides of every limit):
    the instantiation of expected_kernel where the box fits (D <= 13 at cout 4, 11 at cout 8), DMCF_EUNSUPPORTED beyond; the name
    buffer is optional; the wrappers say the same; scatter_block_cells is the closed form the dispatch had."""
    from dmcf_amd import _lib, ops
    seen_d = set()
    for cout, limit in ((4, 13), (8, 11)):
        for reach in range(1, 6):
            for m in range(1, 7):
                D = m + 2 * reach + 1
                seen_d.add(D)
                dims = (4, 4, 4, 24, cout)
                rc, name = _kernel_name(hip_lib, dims, m, reach)
                filt = np.empty(dims, dtype=np.float32)
                if D <= limit:
                    assert (rc, name) == (OK, sr.expected_kernel(cout, m, reach)), (cout, m, reach, rc, name)
                    assert ops.scatter_kernel_name(cout, m, reach) == name and ops.cconv_scatter_supported(filt, m, reach)
                    if cout == 8:  # 8 waves are chosen first, while two workgroups fit: the instantiation does not tell
                        assert name == "cconv_sct_kernel<8, 8>" and sr.two_workgroups(8, m, reach) == (D <= 6)
                    else:
                        assert sr.two_workgroups(4, m, reach) == (name == "cconv_sct_kernel<4, 8>")
                else:
                    assert rc == EUNSUPPORTED, (cout, m, reach, rc, name)
                    assert not ops.cconv_scatter_supported(filt, m, reach)
                    with pytest.raises(_lib.DmcfError):
                        ops.scatter_kernel_name(cout, m, reach)
                assert _kernel_name(hip_lib, dims, m, reach, size=0) == (rc, None)  # the query without a name
            assert ops.scatter_block_cells(cout, reach) == max(0, min(4, limit - 1 - 2 * reach))
            assert ops.scatter_block_cells(cout, reach, most=6) == max(0, min(6, limit - 1 - 2 * reach))
    assert seen_d == set(range(4, 18))


def test_kernel_name_refusals(hip_lib):
    for dims in ((3, 4, 4, 24, 4), (4, 3, 4, 24, 4), (4, 4, 3, 24, 4), (4, 4, 4, 33, 4), (4, 4, 4, 24, 6), (4, 4, 4, 24, 16)):
        assert _kernel_name(hip_lib, dims, 2, 2)[0] == EUNSUPPORTED, dims
        assert _kernel_name(hip_lib, dims, 2, 2, size=0)[0] == EUNSUPPORTED, dims
    ok = (4, 4, 4, 32, 8)
    assert _kernel_name(hip_lib, ok, 2, 2) == (OK, "cconv_sct_kernel<8, 8>")
    for m, reach in ((2, 0), (0, 2), (2, -1), (-3, 2)):
        assert _kernel_name(hip_lib, ok, m, reach)[0] == EINVAL, (m, reach)
    assert _kernel_name(hip_lib, ok, 2, 2, size=4)[0] == EINVAL  # a buffer too short for the name
    assert _kernel_name(hip_lib, (4, 4, 4, 0, 8), 2, 2)[0] == EINVAL
    # a buffer without a length, a length without a buffer
    dims = (ctypes.c_int32 * 5)(*ok)
    assert hip_lib.dmcf_cconv_scatter_kernel_name(dims, 2, 2, ctypes.create_string_buffer(64), 0) == EINVAL
    assert hip_lib.dmcf_cconv_scatter_kernel_name(dims, 2, 2, None, 64) == EINVAL
