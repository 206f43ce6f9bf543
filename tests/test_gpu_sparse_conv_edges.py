"""The voxel convolution's kernels on the GPU at their chunk, tile, slab and flag edges, against the float64 reference and the
bars of tests/sparse_conv_edges_ref.py (whose docstring derives them; tests/test_sparse_conv_edges_cpu.py shows on the CPU that a
float32 emulation of the kernels' order lies inside them and that seeded faults do not).  Every case goes through
ops.sparse_gather and ops.sparse_gather_backward, twice: identical bits.

channels    (Cin, Cout) from 1x1 to 481x6 and 65x241, plain and W_TRANSPOSED: cpc 60 down to 1, two and three channel chunks, up
            to four passes of column tiles, a filter of 16 dW chunks whose cells sit on no chunk edge
cells       K below, on and one above multiples of cpc, every cell hit, every chunk edge straddled by one row, the clamp at
            both ends of every axis; [2, 3, 5] under all eight flag combinations
rows        n_rows either side of the 16-row tile and the 64-row workgroup; rows of 0 to 300 pairs, a tenth out of range
slabs       the filter gradient with n_pairs either side of the batches and of the 512-pair slab
accumulate  ``out`` pre-filled, with bias and without; the no-pairs early return
layers      65x241 and a [3, 3, 3] case through ops.sparse_conv and ops.sparse_conv_transpose with autograd

The worst err / bar of each group is printed by test_report_worst_ratio (run with -s)."""
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import sparse_conv_edges_ref as se  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but torch.cuda.is_available() is False")
    return torch.device("cuda:0")


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.array(a)).to(dev)  # (a copy: the cases' arrays are read-only)


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def _run(dev, case):
    """ops.sparse_gather and ops.sparse_gather_backward on the case, twice (identical bits), checked against every bar and
    exact rule.  A list with out-of-range entries gets its inversion from the host (se.transpose drops them).
    -> dict(out, plain, dW, dF) of host arrays (what the case asks for)."""
    from dmcf_amd import ops
    only = case["only"] or ("out", "dW", "dF")
    flags, n_cols = case["flags"], len(case["col_pos"])
    W, rp, cp, x, G = (_t(case[k], dev) for k in ("W", "row_pos", "col_pos", "x", "G"))
    idx, rs = _t(case["idx"], dev), _t(case["row_splits"], dev)
    kw = dict(row_scale=_t(case["row_scale"], dev), col_scale=_t(case["col_scale"], dev))
    geo = (W, rp, cp, x, idx, rs, case["extent"], [float(v) for v in case["offset"]])
    inverted = None
    if ((case["idx"] < 0) | (case["idx"] >= n_cols)).any():
        inv_idx, inv_rs = se.transpose(case["idx"], case["row_splits"], n_cols)
        inverted = types.SimpleNamespace(neighbors_index=_t(inv_idx, dev), neighbors_row_splits=_t(inv_rs, dev))
    bias = _t(case["bias"], dev)

    def forward(fl):
        out = _t(case["out0"], dev) if fl & se.ACCUMULATE else None
        return ops.sparse_gather(*geo, flags=fl, bias=bias, out=out, **kw)

    runs = []
    for _ in range(2):
        got = {}
        if "out" in only:
            got["out"] = forward(flags)
            if flags & se.ACCUMULATE:
                got["plain"] = forward(flags & ~se.ACCUMULATE)
        if "dW" in only or "dF" in only:
            got["dW"], got["dF"] = ops.sparse_gather_backward(*geo, grad_out=G, flags=flags, need_filters="dW" in only,
                                                              need_features="dF" in only, inverted=inverted, **kw)
        runs.append(got)
    torch.cuda.synchronize()
    for k, v in runs[0].items():
        assert (v is None and runs[1][k] is None) or torch.equal(v, runs[1][k]), f"{case['name']}: two calls differ in {k}"
    got = {k: _np(v) for k, v in runs[0].items()}
    se.check_case(case, got)
    return got


@pytest.mark.parametrize("name", se.case_names("channels"))
def test_channels(dev, name):
    _run(dev, se.case("channels", name))


@pytest.mark.parametrize("name", se.case_names("cells"))
def test_cells(dev, name):
    _run(dev, se.case("cells", name))


@pytest.mark.parametrize("name", se.case_names("rows"))
def test_rows(dev, name):
    _run(dev, se.case("rows", name))


@pytest.mark.parametrize("name", se.case_names("slabs"))
def test_slabs(dev, name):
    _run(dev, se.case("slabs", name))


@pytest.mark.parametrize("name", se.case_names("accumulate"))
def test_accumulate(dev, name):
    c = se.case("accumulate", name)
    got = _run(dev, c)
    if name.startswith("no_pairs"):  # the early return of ops.sparse_gather: every row is empty
        want = np.zeros_like(got["out"]) if c["out0"] is None else c["out0"]
        want = want if c["bias"] is None else (want + c["bias"]).astype(np.float32)
        assert np.array_equal(got["out"], want) and not got["dW"].any() and not got["dF"].any()


@pytest.mark.parametrize("which", [0, 1], ids=["65x241", "k3x3x3"])
def test_layers(dev, which):
    """The same shapes through the layers' entry points with autograd: ops.sparse_conv (the column scale as inp_importance,
    normalize) and ops.sparse_conv_transpose (NEGATE, the row scale as out_importance)."""
    from dmcf_amd import ops
    conv, tr = se.layer_cases()[which]
    for c, transposed in ((conv, False), (tr, True)):
        W, x, b = (_t(c[k], dev).requires_grad_(True) for k in ("W", "x", "bias"))
        rp, cp, idx, rs = (_t(c[k], dev) for k in ("row_pos", "col_pos", "idx", "row_splits"))
        off = [float(v) for v in c["offset"]]
        if transposed:
            inv_idx, inv_rs = (_t(a, dev) for a in se.transpose(c["idx"], c["row_splits"], len(c["col_pos"])))
            out = ops.sparse_conv_transpose(W, rp, c["voxel"], off, cp, x, inv_idx, inv_rs, idx, rs,
                                            out_importance=_t(c["row_scale"], dev), bias=b)
        else:
            out = ops.sparse_conv(W, rp, c["voxel"], off, cp, x, idx, rs, inp_importance=_t(c["col_scale"], dev), normalize=True, bias=b)
        assert out.grad_fn is not None
        dW, dF, db = torch.autograd.grad(out, [W, x, b], _t(c["G"], dev))
        se.check_case(c, dict(out=_np(out), dW=_np(dW), dF=_np(dF)))
        assert np.allclose(_np(db), c["G"].astype(np.float64).sum(axis=0), rtol=1e-5, atol=1e-5)
        with torch.no_grad():  # the fused call, bias inside the kernel
            if transposed:
                fused = ops.sparse_conv_transpose(W, rp, c["voxel"], off, cp, x, inv_idx, inv_rs, idx, rs,
                                                  out_importance=_t(c["row_scale"], dev), bias=b)
            else:
                fused = ops.sparse_conv(W, rp, c["voxel"], off, cp, x, idx, rs, inp_importance=_t(c["col_scale"], dev), normalize=True,
                                        bias=b)
        se.check_case(c, dict(out=_np(fused)))


def test_report_worst_ratio():
    """Prints the worst err / bar of every group of this file (run with -s)."""
    print("worst err/bar", {f"{k[0]} {k[1]}": round(v, 4) for k, v in se.WORST.items() if not k[0].startswith(("emulation", "mutated"))})
