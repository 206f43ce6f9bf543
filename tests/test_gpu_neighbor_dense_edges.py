"""PointNet's neighbour-sum kernels on the GPU at their row, tile and slab edges, against the float64 reference and the bars of
tests/neighbor_dense_edges_ref.py (whose docstring derives them; tests/test_neighbor_dense_edges_cpu.py shows on the CPU that a
float32 emulation of the kernels' order lies inside them and that seeded faults do not).  Every case goes through
ops.neighbor_dense and torch.autograd.grad.

widths      EDGE_ROWS (rows of 0 to 640 pairs, a tenth out of range) at eleven Cin x Cout, CSR and padded: identical bits
tiles       n_out either side of the 16-row tile and of the 8-wave workgroup
dx_rows     the backward's gather on rows of the controlled lengths (the forward list is EDGE_ROWS transposed)
slabs       dW and db with n_out either side of 4, 128 and 132 rows, the count channel in every position of a 64-block
one_hot_G   one non-zero row of G at a time: the recorded S_r and c_r of that row alone
slab_cap    n_out above 2048 * 128: rows_per_slab above 128
persistent  more tiles than resident waves: every wave takes a second tile, some a third

The worst err / bar of each group is printed by test_report_worst_ratio (run with -s)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import neighbor_dense_edges_ref as nd  # noqa: E402

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


def _run(dev, case, padded=False, need_x=True, need_w=True, inverted=None):
    """The layer and its gradients, twice (identical bits), checked against every bar and exact rule of the case.
    -> dict(out, dx, dW, db) of host arrays (None for what was not asked or has no operand)."""
    from dmcf_amd import ops
    x = _t(case["x"], dev).requires_grad_(need_x)
    W = _t(case["W"], dev).requires_grad_(need_w)
    b = _t(case["b"], dev)
    if b is not None:
        b.requires_grad_(need_w)
    r, G = _t(case["residual"], dev), _t(case["G"], dev)
    if padded:
        pidx, pbegin, pcount = case["padded"]
        lst = dict(neighbors_index=_t(pidx, dev), neighbors_row_splits=_t(pbegin, dev), neighbors_row_count=_t(pcount, dev))
    else:
        lst = dict(neighbors_index=_t(case["idx"], dev), neighbors_row_splits=_t(case["row_splits"], dev))
    wanted = [("dx", x)] * need_x + [("dW", W)] * need_w + ([("db", b)] if need_w and b is not None else [])
    runs = []
    for _ in range(2):
        y = ops.neighbor_dense(x, W, b, n_in=case["n_in"], relu=case["relu"], residual=r, inverted=inverted, **lst)
        got = dict(out=y.detach())
        if wanted:
            assert y.grad_fn is not None
            for (k, _), g in zip(wanted, torch.autograd.grad(y, [t for _, t in wanted], G)):
                got[k] = g
        runs.append(got)
    torch.cuda.synchronize()
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), f"{case['name']}: two calls differ in {k}"
    got = {k: _np(v) for k, v in runs[0].items()}
    nd.check_case(case, got)
    return got


@pytest.mark.parametrize("name", nd.case_names("widths"))
def test_widths(dev, name):
    """EDGE_ROWS at every width: the 64 / 65 switch of the gather's template, Cin padded to 4 and Cout to 16, widths 1 to 3,
    bias None, relu off.  The padded form of the same rows gives the bits of the CSR form; the kernel is the one named."""
    from dmcf_amd import ops
    c = nd.case("widths", name)
    cin, cout = c["W"].shape
    ops.timer = ops.LaunchTimer()
    try:
        got = _run(dev, c)
        kinds = [(k, m.get("kernel")) for k, m, _, _ in ops.timer.records]
    finally:
        ops.timer = None
    fwd = {m for k, m in kinds if k == "neighbor_dense"}
    bwd = {m for k, m in kinds if k == "neighbor_dense_backward"}
    assert fwd == {nd.gather_name(cin)} and nd.gather_name(cin).endswith("<2>" if cin > 64 else "<1>")
    assert bwd == {nd.gather_name(cout) + ";nd_bwd_weight;nd_bwd_weight_reduce"}  # (the backward's gather has Cout channels in)
    pad = _run(dev, c, padded=True)
    for k in got:
        assert np.array_equal(got[k], pad[k]), f"{name}: the padded form differs from the CSR form in {k}"


@pytest.mark.parametrize("name", nd.case_names("tiles"))
def test_tiles(dev, name):
    _run(dev, nd.case("tiles", name))


@pytest.mark.parametrize("name", nd.case_names("dx_rows"))
def test_dx_rows(dev, name):
    from dmcf_amd import ops
    c = nd.case("dx_rows", name)
    got = _run(dev, c)
    if name == "65x33_relu_inrange":
        # the inversion shared between layers (over every row of x, more than n_in) gives the bits of the layer's own
        shared = ops.SharedInverse(len(c["x"]), _t(c["idx"], dev), _t(c["row_splits"], dev))
        again = _run(dev, c, inverted=shared)
        assert shared._inv is not None
        for k in got:
            assert np.array_equal(got[k], again[k]), k


@pytest.mark.parametrize("name", nd.case_names("slabs"))
def test_slabs(dev, name):
    _run(dev, nd.case("slabs", name), need_x=False)


@pytest.mark.parametrize("name", nd.case_names("one_hot_G"))
def test_one_hot_G(dev, name):
    """n_nz = 1: dW is the recorded S_r times G_r and db the recorded c_r times G_r, for the empty row 0, the row of 640, the
    last row of the first tile, the row of 130 whose first chunk is all out of range, and the last row."""
    c = nd.case("one_hot_G", name)
    got = _run(dev, c)
    _, cr = nd.aggregate(c["x"], c["idx"], c["begin"], c["count"], c["n_in"], True)
    if cr[c["hot"]] == 0:
        assert np.all(got["dW"] == 0) and np.all(got["db"] == 0)


def test_slab_cap(dev):
    """n_out = 2048 * 128 + 5: 1986 slabs of 132 rows; G is non-zero on either side of the first slab edge, in the last row
    and in 20 more rows."""
    c = nd.case("slab_cap", "cap")
    assert nd.bwd_plan(len(c["count"])) == (132, 1986)
    _run(dev, c)


@pytest.mark.parametrize("cin,cout", nd.PERSISTENT_WIDTHS)
def test_persistent(dev, cin, cout):
    """More 16-row tiles than waves resident on the device: a wave's S / count image in LDS is reused, its accumulators are
    reset, and (every 97th row has 65 pairs, every 1009th 130) a second tile enters the second and third chunk."""
    n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
    _, per_cu, resident = nd.launch_plan(cin, cout, n_cu)
    assert resident == 8 * n_cu * per_cu
    c = nd.persistent_case(cin, cout, n_cu)
    n_out = len(c["count"])
    n_tiles = -(-n_out // 16)
    assert n_out == 16 * (2 * resident + 3) + 5 and n_tiles > 2 * resident and n_out % 16 != 0
    assert -(-n_tiles // 8) > n_cu * per_cu  # the grid is capped: resident waves, each with at least two tiles
    backward = (cin, cout) == (8, 16)
    if backward:
        # the backward's gather: the inverted list has n_in rows, Cout channels in and Cin out
        assert -(-c["n_in"] // 16) > nd.launch_plan(cout, cin, n_cu)[2]
    _run(dev, c, need_x=backward, need_w=backward)


def test_report_worst_ratio():
    """Prints the worst err / bar of every group of this file (run with -s)."""
    print("worst err/bar", {k: round(v, 4) for k, v in nd.WORST.items() if not k.startswith(("emulation", "mutated"))})
