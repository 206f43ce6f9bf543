"""The forward error bar of tests/cconv_forward_ref.py on the CPU: it is sound (the float32 oracle is within it on every case
tests/test_gpu_cconv_forward_bar.py runs; C_GEO is the constant measured here), it has teeth (seeded faults break it), the case
matrix covers what it claims, and every case dispatches to the kernel it names."""
import copy
import ctypes
import math
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import cconv_forward_ref as fr  # noqa: E402

MATRIX = fr.matrix()


@pytest.fixture(scope="module")
def hip_lib():
    from dmcf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()
_MEASURED = {}  # case id -> (what the A part leaves of the float32 oracle's error, share of rows left out)


def _measure(cid, spec):
    if cid not in _MEASURED:
        c = fr.Case(**spec)
        want, A, A1, kbar, keep = c.bar()
        y = c.oracle32()
        fr.check_forward("oracle32", y, want, A, A1, kbar, keep)
        _MEASURED[cid] = (fr.geo_ratio(y, want, A, A1, kbar, keep), float((~keep).mean()), c.interp)
    return _MEASURED[cid]


@pytest.mark.parametrize("cid,kernel,name,spec", MATRIX, ids=[m[0] for m in MATRIX])
def test_float32_oracle_is_within_the_bar(oracle, cid, kernel, name, spec):
    _, left_out, interp = _measure(cid, spec)
    if interp == "nearest_neighbor":
        assert left_out < fr.NN_MAX_SHARE, f"{left_out:.3%} of the rows marked fragile by the reference alone"
    else:
        assert left_out == 0.0


def _lattice_measure(case):
    if case not in _MEASURED:
        import oracle as orc
        L = fr.lattice_case(case)
        idx, rs, d2 = orc.fixed_radius_search(L["ipos"], L["opos"], L["radius"], False, bruteforce=True)
        want, A, A1, kbar = fr.lattice_bar(L, idx, rs)
        r = np.float32(0.5) * np.float32(2 * L["radius"])
        y = orc.continuous_conv(L["filt"], L["opos"], 2 * L["radius"], L["ipos"], L["feat"], idx, rs,
                                orc.window("poly6", d2 / (r * r))) + L["bias"]
        fr.check_forward("oracle32", y, want, A, A1, kbar)
        _MEASURED[case] = (fr.geo_ratio(y, want, A, A1, kbar), 0.0, "linear")
    return _MEASURED[case]


@pytest.mark.parametrize("case", fr.LATTICE_CASES)
def test_float32_oracle_is_within_the_bar_on_the_lattice_cases(oracle, case):
    _lattice_measure(case)


def test_c_geo_is_the_measured_constant(oracle):
    """C_GEO = 4 x the worst (err - kbar A 2^-24) / (A1 2^-24) of the float32 oracle over the matrix and the lattice cases,
    rounded up to a power of two.  Prints the measured value (run with -s)."""
    worst = max([_measure(cid, spec)[0] for cid, _, _, spec in MATRIX] + [_lattice_measure(c)[0] for c in fr.LATTICE_CASES])
    print(f"measured c_geo {worst:.4g}; recorded {fr.MEASURED_C_GEO:.4g}; C_GEO = {fr.C_GEO:.4g} = 2^{math.log2(fr.C_GEO):.0f}")
    assert 0.5 * fr.MEASURED_C_GEO <= worst <= fr.MEASURED_C_GEO, "the recorded measurement is stale"
    assert fr.C_GEO == 2.0 ** math.ceil(math.log2(4 * fr.MEASURED_C_GEO))


def test_row_lengths_and_empty_rows(oracle):
    import oracle as orc
    for dim in (3, 2, 1):
        inp, out = fr.controlled_cloud(1, dim)
        _, rs, _ = orc.fixed_radius_search(inp, out, fr.RADIUS, False, bruteforce=True)
        cnt = np.diff(rs)
        assert [int(c) for c in cnt[:14]] == [0, 1, 2, 63, 64, 0, 65, 127, 128, 129, 640, 1, 1, 0]
        for n in fr.N_OUT_EDGES[1:]:
            inp, o = fr.controlled_cloud(1, dim, n)
            _, rs, _ = orc.fixed_radius_search(inp, o, fr.RADIUS, False, bruteforce=True)
            c = np.diff(rs)
            assert o.shape[0] == n and c[0] == 0 and c[-1] == 0 and c[5] == 0 and c[13] == 0
            assert set(fr.ROW_LENGTHS) <= set(int(x) for x in c)
        for off in (6.0, 60.0):
            inp, o = fr.controlled_cloud(1, dim, None, off)
            _, rs, _ = orc.fixed_radius_search(inp, o, fr.RADIUS, False, bruteforce=True)
            assert set(fr.ROW_LENGTHS) <= set(int(x) for x in np.diff(rs)) and abs(float(o[20, 1])) > off / 2


def test_padded_rows_past_the_buffer_are_empty(oracle):
    c = fr.Case(shape=(4, 4, 4), cin=4, cout=3, padded=True, n_out=33)
    assert c.cut >= 2 and c.count[-c.cut] > 0 and c.idx.shape[0] == (33 - c.cut) * (int(c.count.max()) + 3)
    assert c.pw.i.max() < 33 - c.cut and c.rs[-1 - c.cut] + c.count[-c.cut] > c.idx.shape[0]


def _options(spec):
    s = dict(fr.Case.DEFAULTS)
    s.update(spec)
    o = {("window", s["window"], s["dist"] and s["window"] not in (None, "explicit"))}
    o |= {(k,) for k in ("imp", "normalize", "bias", "accumulate", "mask") if s[k]}
    if s["sym_axis"] is not None:
        o.add(("sym", tuple(s["shape"]), s["sym_axis"]))
    return o


@pytest.mark.parametrize("kernel", list(fr.KERNELS))
def test_matrix_covers_every_option(kernel):
    """Every option the kernel accepts: with a CSR list, with a padded one, and at an n_out edge; every channel count and
    filter shape of its lists at least once."""
    k = fr.KERNELS[kernel]
    cases = [spec for _, kn, _, spec in MATRIX if kn == kernel]
    want = {("window", w, d) for w, d in fr.WINDOW_FORMS} | {("imp",), ("bias",), ("accumulate",)}
    if k.get("normalize"):
        want.add(("normalize",))
    if k.get("mask"):
        want.add(("mask",))
    want |= {("sym", tuple(sh), ax) for sh, ax in k.get("sym", ())}
    for opt in sorted(want, key=str):
        having = [s for s in cases if opt in _options(s)]
        assert any(not s.get("padded") for s in having), f"{opt}: no CSR case"
        assert any(s.get("padded") for s in having), f"{opt}: no padded case"
        assert any(s.get("n_out") in fr.N_OUT_EDGES for s in having), f"{opt}: no n_out edge"
    assert {s["cin"] for s in cases} >= set(k["cins"]) and {s["cout"] for s in cases} >= set(k["couts"])
    assert {tuple(s["shape"]) for s in cases} >= set(k["shapes"])
    assert {s.get("n_out") for s in cases} >= set(fr.N_OUT_EDGES)
    if not k.get("normalize"):
        assert not any(s.get("normalize") for s in cases)


@pytest.mark.parametrize("cid,kernel,name,spec", MATRIX, ids=[m[0] for m in MATRIX])
def test_case_dispatches_to_its_kernel(hip_lib, monkeypatch, cid, kernel, name, spec):
    """dmcf_cconv_kernel_name on the case's arguments (no launch, no device: the pointers are only tested for NULL and
    alignment): a forced name that fell through the eligibility chain would test another kernel."""
    from dmcf_amd import _lib, ops
    if kernel is None:
        monkeypatch.delenv("DMCF_CCONV_KERNEL", raising=False)
    else:
        monkeypatch.setenv("DMCF_CCONV_KERNEL", kernel)
    s = dict(fr.Case.DEFAULTS)
    s.update(spec)
    a = _lib.CconvArgs()
    for d, v in enumerate((*s["shape"], s["cin"], s["cout"])):
        a.filter_dims[d] = v
    a.sym_axis = s["sym_axis"] or 0
    a.n_out, a.n_inp, a.n_pairs = s["n_out"] or fr.N_OUT_FULL, 2420, 10000
    fake = 1 << 20
    a.filters = a.out_positions = a.inp_positions = a.inp_features = a.neighbors_index = a.neighbors_row_splits = a.out = fake
    a.inp_importance = fake if s["imp"] else None
    a.neighbors_value = fake if s["window"] == "explicit" or (s["window"] and s["dist"]) else None
    a.neighbors_row_count = fake if s["padded"] else None
    a.bias = fake if s["bias"] else None
    a.extent, a.window_fac = 0.46, 1.0
    a.window = ops.WINDOWS[s["window"]]
    a.coordinate_mapping, a.interpolation = ops.MAPPINGS[s["mapping"]], ops.INTERPOLATIONS[s["interp"]]
    a.flags = ((ops.FLAG_ALIGN_CORNERS if s["align"] else 0) | (ops.FLAG_NORMALIZE if s["normalize"] else 0) |
               (ops.FLAG_SYMMETRIC if s["sym_axis"] is not None else 0) | (ops.FLAG_ACCUMULATE if s["accumulate"] else 0))
    if s["mask"]:  # (the hint names fewer blocks than the whole filter has)
        ca = max(4, s["cin"] // 2 // 4 * 4)
        mask = ops.block_diagonal_tile_mask([(0, ca, 0, 16), (ca, s["cin"], 16, s["cout"])])
        assert mask not in (0, ops.block_diagonal_tile_mask([(0, s["cin"], 0, s["cout"])]))
        a.filter_tile_mask = mask
    buf = ctypes.create_string_buffer(96)
    fn = hip_lib.dmcf_cconv_extents_kernel_name if s["extents"] else hip_lib.dmcf_cconv_kernel_name
    _lib.check(fn(ctypes.byref(a), buf, 96), "dmcf_cconv_kernel_name")
    assert buf.value.decode().startswith(name), f"{cid} dispatches to {buf.value.decode()}"


# ---- teeth ----------------------------------------------------------------------------------------------------------------------

def _plain():
    # 257 rows: the last tile of 16 holds one row, the empty one; rows 1 / 6: the single-pair and the 65-pair row
    return fr.Case(shape=(4, 4, 4), cin=8, cout=17, window="poly6", dist=True, bias=True, imp=True, n_out=257)


def _drop_last_pair_of_65(c):
    idx, rs, val = c.effective_csr()
    assert rs[7] - rs[6] == 65
    p = rs[7] - 1
    rs = rs.copy()
    rs[7:] -= 1
    return c.oracle32(np.delete(idx, p), rs, np.delete(val, p))


def _pair_64_twice(c):
    idx, rs, val = c.effective_csr()
    p = rs[6] + 64
    rs = rs.copy()
    rs[7:] += 1
    return c.oracle32(np.insert(idx, p, idx[p]), rs, np.insert(val, p, val[p]))


def _one_channel_scaled(c):
    y = c.oracle32()
    y[:, 5] *= np.float32(1 + 2.0 ** -12)
    return y


def _two_corners_swapped(c):
    pw = copy.copy(c.pw)
    pw.wts = pw.wts.copy()
    p = int(np.flatnonzero(pw.i == 3)[10])
    pw.wts[p, [0, 7]] = pw.wts[p, [7, 0]]
    assert abs(c.pw.wts[p, 0] - c.pw.wts[p, 7]) > 1e-3
    W, F = torch.from_numpy(c.filt).double(), torch.from_numpy(c.feat).double()
    return (c.oracle32() + (fr.conv(pw, W, F) - fr.conv(c.pw, W, F)).numpy()).astype(np.float32)


def _bias_missing_on_last_tile(c):
    y = c.oracle32()
    y[256:] -= c.bias_v
    return y


def _importance_ignored_for_one_point(c):
    imp = c.imp_v.copy()
    imp[c.pw.j[c.pw.i == 1][0]] = 1.0
    return c.oracle32(imp=imp)


def _single_pair_row_zeroed(c):
    y = c.oracle32()
    assert c.csr_counts[1] == 1
    y[1] = c.bias_v
    return y


def _ascc():
    return fr.Case(shape=(4, 4, 2), sym_axis=2, cin=8, cout=3, window="peak", dist=True, n_out=257)


def _mirror_without_sign_on_one_cell(c):
    import oracle as orc
    full = orc.mirror_kernel(c.filt, 2).copy()
    full[1, 2, 0] = -full[1, 2, 0]  # (x cells 0, 1 are the mirrored half)
    return c.oracle32(full=full)


def _small_weight():
    # 17 rows, no window, the filter zero but for its last y plane: row "Y" is a corner weight of 2^-13 times one feature row,
    # far below the 640-pair row's output and above the floor of the bar
    return fr.Case(shape=(4, 4, 4), cin=4, cout=3, window=None, far_plane=True, n_out=17)


def _small_row_scaled(c):
    y = c.oracle32()
    y[fr.ROW_Y] *= np.float32(1 + 2.0 ** -8)
    return y


FAULTS = {
    "last_pair_of_a_65_pair_row_dropped": (_plain, _drop_last_pair_of_65),
    "pair_64_of_a_row_counted_twice": (_plain, _pair_64_twice),
    "one_output_channel_scaled_by_1_plus_2^-12": (_plain, _one_channel_scaled),
    "two_corner_weights_of_one_pair_swapped": (_plain, _two_corners_swapped),
    "bias_missing_on_the_last_partial_tile": (_plain, _bias_missing_on_last_tile),
    "ascc_mirror_without_its_sign_on_one_cell": (_ascc, _mirror_without_sign_on_one_cell),
    "inp_importance_ignored_for_one_point": (_plain, _importance_ignored_for_one_point),
    "single_pair_row_zeroed": (_plain, _single_pair_row_zeroed),
    "row_of_one_small_weight_scaled_by_1_plus_2^-8": (_small_weight, _small_row_scaled),
}
SMALL_ELEMENT_FAULTS = ("row_of_one_small_weight_scaled_by_1_plus_2^-8",)
_CASES = {}


def _fault(name):
    make, fault = FAULTS[name]
    if make not in _CASES:
        _CASES[make] = make()
    c = _CASES[make]
    return c, fault(c)


@pytest.mark.parametrize("fault", list(FAULTS))
def test_seeded_fault_breaks_the_bar(oracle, fault):
    c, y = _fault(fault)
    want, A, A1, kbar, keep = c.bar()
    assert fr.within_bar(c.oracle32(), want, A, A1, kbar, keep), "the float32 oracle itself is outside the bar"
    assert not fr.within_bar(y, want, A, A1, kbar, keep), "the fault is within the bar"


@pytest.mark.parametrize("fault", list(FAULTS))
def test_what_the_whole_tensor_criterion_makes_of_the_faults(oracle, fault):
    """_close(..., 1e-5) of tests/test_gpu_ops.py (max error over the tensor's largest element) on the same faults: printed,
    not
    asserted for the eight faults of the issue (run with -s).  Observed: it rejects all eight (the smallest, the channel scaled
    by 1 + 2^-12, is 1.6e-4 of the output scale).  What it cannot see is an error of that relative size in an element far below
    the tensor's largest: the ninth fault, which it is asserted to let through."""
    c, y = _fault(fault)
    want = c.bar()[0]
    err = np.abs(y.astype(np.float64) - want).max() / np.abs(want).max()
    print(f"{fault}: max error {err:.3g} of the output scale -> _close(1e-5) {'passes' if err <= 1e-5 else 'rejects'} it")
    if fault in SMALL_ELEMENT_FAULTS:
        assert err <= 1e-5, "the fault confined to a small element was meant to pass the whole-tensor criterion"
