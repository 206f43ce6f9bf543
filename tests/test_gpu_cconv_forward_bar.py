"""Every forward CConv / ASCC kernel that walks a neighbour list or a lattice stencil against the float64 reference, element by
element (tests/cconv_forward_ref.py; the scatter form, dmcf_cconv_scatter_forward, has the same bar plus the term of its
fixed-point sums in tests/test_gpu_cconv_scatter_bar.py):

    |gpu - ref| <= (kbar * A + C_GEO * A1) * 2^-24

on deterministic clouds with controlled row lengths (0, 1, 2, 63 .. 65, 127 .. 129, 640), n_out at the tile edges, CSR and cut
padded lists, positions far from the origin, the options each kernel's eligibility function accepts, per-row extents (dmcf_cconv_forward_extents) and the lattice form.  Every case first
asserts the kernel it dispatches to.  The same cases run on the float32 CPU oracle in tests/test_cconv_forward_ref_cpu.py, where
C_GEO is measured.  The worst err / bar per kernel is printed by test_report_worst_ratio (run with -s)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import cconv_forward_ref as fr  # noqa: E402

pytestmark = pytest.mark.gpu

MATRIX = fr.matrix()


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but torch.cuda.is_available() is False")
    return torch.device("cuda:0")


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _force(monkeypatch, kernel):
    if kernel is None:
        monkeypatch.delenv("DMCF_CCONV_KERNEL", raising=False)
    else:
        monkeypatch.setenv("DMCF_CCONV_KERNEL", kernel)


def _run(c, dev, name):
    """The case on the GPU, after asserting that it dispatches to the kernel ``name``; returns out as a numpy array."""
    from dmcf_amd import ops
    extent = c.extent if c.row_extents is None else _t(c.row_extents, dev)
    args = (_t(c.filt, dev), _t(c.out_pos, dev), extent, _t(c.inp_pos, dev), _t(c.feat, dev), _t(c.idx.astype(np.int32), dev),
            _t(c.rs.astype(np.int64), dev))
    kw = dict(neighbors_value=_t(c.nval, dev), window=c.window, window_fac=c.window_fac, inp_importance=_t(c.imp_v, dev),
              align_corners=c.align, coordinate_mapping=c.mapping, interpolation=c.interp, normalize=c.normalize,
              symmetric=c.symmetric, sym_axis=c.sym_axis if c.symmetric else 2, bias=_t(c.bias_v, dev),
              neighbors_row_count=_t(c.count, dev),
              filter_tile_mask=ops.block_diagonal_tile_mask(c.tile_mask) if c.tile_mask else 0)
    got = ops.cconv_forward(*args, name_only=True, **kw)
    assert got.startswith(name), f"dispatched to {got}, not {name}"
    if c.tile_mask:
        assert kw["filter_tile_mask"] not in (0, ops.block_diagonal_tile_mask([(0, c.cin, 0, c.cout)]))
    out = _t(c.prior, dev)
    y = ops.cconv_forward(*args, out=out, accumulate=c.prior is not None, **kw)
    torch.cuda.synchronize()
    return y.cpu().numpy()


def _empty_rows_are_exact(c, y):
    """A row without pairs is exactly the bias, or exactly the prior content (plus the bias) under accumulate."""
    empty = np.bincount(c.pw.i, minlength=c.out_pos.shape[0]) == 0
    want = np.zeros_like(y)
    if c.bias_v is not None:
        want = want + c.bias_v
    if c.prior is not None:
        want = want + c.prior
    assert np.array_equal(y[empty], want[empty].astype(np.float32)), "a row without pairs is not exactly bias / prior content"


@pytest.mark.parametrize("cid,kernel,name,spec", MATRIX, ids=[m[0] for m in MATRIX])
def test_kernel_within_the_bar(dev, monkeypatch, cid, kernel, name, spec):
    _force(monkeypatch, kernel)
    c = fr.Case(**spec)
    y = _run(c, dev, name)
    want, A, A1, kbar, keep = c.bar()
    assert (~keep).mean() < fr.NN_MAX_SHARE and (c.interp == "nearest_neighbor" or keep.all())
    if c.padded and c.cut:
        assert c.count[-c.cut:].sum() > 0 and c.pw.i.max() < c.out_pos.shape[0] - c.cut, "no row cut off by the capacity"
    _empty_rows_are_exact(c, y)
    if c.zero_channel is not None:  # a zero filter slice: exactly zero plus the bias
        assert np.array_equal(y[:, c.zero_channel], np.full(y.shape[0], c.bias_v[c.zero_channel], np.float32))
    if c.far_plane:
        assert c.csr_counts[fr.ROW_Y] == 1 and 0 < A[fr.ROW_Y].max() < 1e-2 * A1[fr.ROW_Y].min()
    fr.check_forward("extents" if c.extents else kernel or "auto", y, want, A, A1, kbar, keep)


@pytest.mark.parametrize("case", fr.LATTICE_CASES)
def test_lattice_form(dev, case):
    """ops.lattice_conv through dmcf_amd/lattice.py on the cases of test_lattice_conv_matches_neighbour_list_form, against the
    float64 reference on the equivalent neighbour list."""
    from dmcf_amd import lattice, ops
    lattice._cores().clear()
    L = fr.lattice_case(case)
    cen = _t(L["center"], dev)

    def info(cells, pos, vox):
        lo = cells.min(axis=0) - 1  # a box with a margin, as the candidate box of grid_pos has
        return lattice.LatticeInfo(_t(pos, dev), cen, [vox] * 3, "test", lo, cells.max(axis=0) - lo + 2)
    a, b = info(L["icell"], L["ipos"], L["ivox"]), info(L["ocell"], L["opos"], L["ovox"])
    y = lattice.LatticePair(a, b, L["ratio"]).conv(ops, _t(L["filt"], dev), _t(L["feat"], dev), L["opos"].shape[0], 2 * L["radius"],
                                                   window="poly6", bias=_t(L["bias"], dev)).cpu().numpy()
    nns = ops.fixed_radius_search(_t(L["ipos"], dev), _t(L["opos"], dev), L["radius"], return_distances=False)
    want, A, A1, kbar = fr.lattice_bar(L, nns.neighbors_index.cpu().numpy(), nns.neighbors_row_splits.cpu().numpy())
    fr.check_forward("lattice", y, want, A, A1, kbar)


def test_report_worst_ratio():
    """Prints the worst err / bar of every kernel of this file (run with -s)."""
    print("worst err/bar", {k: round(v, 4) for k, v in fr.WORST.items()})
