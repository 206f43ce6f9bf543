"""SparseConv / SparseConvTranspose on the GPU against the float64 reference of tests/sparse_conv_ref.py: the max-norm lists
against brute force, both forwards and every gradient element by element under |err| <= kbar * 2^-24 * A, the k = 3 forward
against the existing generic CConv kernel, the two layers end to end, determinism of the backward."""
import functools

import numpy as np
import pytest
import torch

import sparse_conv_ref as sr

pytestmark = pytest.mark.gpu

CASES = {c.name: c for c in sr.small_cases()}
NAMES = list(CASES) + ["k3_c8x16_20k"]
WORST = {}


def _case(name):
    return CASES[name] if name in CASES else sr.big_case()


def _dev():
    return torch.device("cuda:0")


def _t(a, grad=False):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(_dev()).requires_grad_(grad)


def _note(group, worst):
    WORST[group] = max(WORST.get(group, 0.0), worst)
    print(f"worst err/bar [{group}]: {WORST[group]:.3g}")


def _rows(index, row_splits):
    """The rows of a CSR list as a sorted array of (row, index) keys."""
    index, rs = np.asarray(index, dtype=np.int64), np.asarray(row_splits, dtype=np.int64)
    row = np.repeat(np.arange(rs.shape[0] - 1), np.diff(rs))
    return np.sort(row * (1 << 32) + index)


def _search(points, queries, radius, ignore=False):
    from dmcf_amd import ops
    nns = ops.fixed_radius_search(_t(points), _t(queries), float(radius), ignore_query_point=ignore, return_distances=False,
                                  metric="Linf")
    return nns.neighbors_index, nns.neighbors_row_splits


@functools.lru_cache(maxsize=None)
def _lists(name):
    """(SparseConv's list, SparseConvTranspose's list of the input points, its inversion) of a case, on the device."""
    from dmcf_amd import ops
    c = _case(name)
    conv = _search(c.inp, c.out - c.shift(), c.radius)
    tr = _search(c.out, c.inp - c.shift(), c.radius)
    inv = ops.invert_neighbors_list(c.out.shape[0], tr[0], tr[1])
    return conv, tr, (inv.neighbors_index, inv.neighbors_row_splits)


@pytest.mark.parametrize("name", NAMES)
def test_linf_lists_equal_brute_force(name):
    c = _case(name)
    conv, tr, _ = _lists(name)
    for (gi, grs), (ri, rrs), what in ((conv, c.conv_list, "queries = outputs"), (tr, c.transpose_list, "queries = inputs")):
        gi, grs = gi.cpu().numpy(), grs.cpu().numpy()
        assert np.array_equal(grs, rrs), (name, what, "row lengths")
        assert np.array_equal(_rows(gi, grs), _rows(ri, rrs)), (name, what, "row sets")
    if name in CASES:
        gi, grs = _search(c.inp, c.inp, c.radius, ignore=True)
        ri, rrs = sr.pair_sets(c.inp, c.inp, c.radius, ignore_query_point=True)
        assert np.array_equal(grs.cpu().numpy(), rrs) and np.array_equal(_rows(gi.cpu().numpy(), rrs), _rows(ri, rrs)), (name, "ignore_query_point")
        again = _search(c.inp, c.out - c.shift(), c.radius)
        assert torch.equal(again[0], conv[0]) and torch.equal(again[1], conv[1]), "two searches differ"


def _run(name, transpose, grad):
    """(out, W, F, bias, importance) of the op on the case's tensors (leaves that record when ``grad``)."""
    from dmcf_amd import ops
    c = _case(name)
    conv, tr, inv = _lists(name)
    W, F, b = _t(c.W, grad), _t(c.F, grad), _t(c.bias, grad)
    if transpose:
        imp = _t(c.out_importance, grad)
        out = ops.sparse_conv_transpose(W, _t(c.out), c.voxel, c.offset, _t(c.inp), F, tr[0], tr[1], inv[0], inv[1],
                                        out_importance=imp, normalize=c.normalize, bias=b)
    else:
        imp = _t(c.inp_importance, grad)
        out = ops.sparse_conv(W, _t(c.out), c.voxel, c.offset, _t(c.inp), F, conv[0], conv[1], inp_importance=imp,
                              normalize=c.normalize, bias=b)
    return out, W, F, b, imp


@pytest.mark.parametrize("transpose", [False, True], ids=["conv", "transpose"])
@pytest.mark.parametrize("name", NAMES)
def test_forward_against_reference(name, transpose):
    c = _case(name)
    out = _run(name, transpose, False)[0]
    ref, A = c.forward(transpose)
    _note("forward" + ("_transpose" if transpose else ""), sr.check(out.cpu().numpy(), ref, A, c.kbar(transpose), name))


@pytest.mark.parametrize("transpose", [False, True], ids=["conv", "transpose"])
@pytest.mark.parametrize("name", NAMES)
def test_gradients_against_reference(name, transpose):
    c = _case(name)
    out, W, F, b, imp = _run(name, transpose, True)
    assert out.requires_grad
    (out * _t(c.G)).sum().backward()
    (dW, aW), (dF, aF), (db, ab), dimp = c.grads(transpose)
    tag = "_transpose" if transpose else ""
    # chains: a filter element sums its cell's pairs (bounded as the rows are); a feature gradient sums the input's pairs over K * Cout
    _note("grad_filters" + tag, sr.check(W.grad.cpu().numpy(), dW, aW, c.kbar(transpose), name + " dW"))
    _note("grad_features" + tag, sr.check(F.grad.cpu().numpy(), dF, aF, c.kbar(transpose, chain_channels=c.cout, columns=True), name + " dF"))
    if b is not None:
        _note("grad_bias" + tag, sr.check(b.grad.cpu().numpy(), db, ab, c.kbar(transpose), name + " dbias"))
    if imp is not None:
        _note("grad_importance" + tag, sr.check(imp.grad.cpu().numpy(), dimp[0], dimp[1], c.kbar(transpose), name + " dimportance"))


@pytest.mark.parametrize("name", [n for n in NAMES if _case(n).kernel_size == [3, 3, 3]])
def test_k3_forward_against_the_generic_cconv_kernel(name):
    """The existing kernel computes the same thing for odd kernels: identity mapping, nearest neighbour, align_corners False."""
    from dmcf_amd import ops
    c = _case(name)
    conv = _lists(name)[0]
    new = _run(name, False, False)[0]
    old = ops.cconv_forward(_t(c.W), _t(c.out), float(sr.extent(c.kernel_size, c.voxel)), _t(c.inp), _t(c.F), conv[0], conv[1],
                            inp_importance=_t(c.inp_importance), align_corners=False, coordinate_mapping="identity",
                            interpolation="nearest_neighbor", normalize=c.normalize, bias=_t(c.bias))
    ref, A = c.forward(False)
    _note("generic_kernel_vs_reference", sr.check(old.cpu().numpy(), ref, A, c.kbar(False), name + " generic"))
    _note("new_vs_generic_kernel", sr.check(new.cpu().numpy(), old.cpu().numpy().astype(np.float64), A, c.kbar(False), name))


@pytest.mark.parametrize("transpose", [False, True], ids=["SparseConv", "SparseConvTranspose"])
@pytest.mark.parametrize("name", ["k3_c5x7_imp_norm_bias", "k4_c8x16_bias", "k2_c5x7_norm", "k122_planar_offset_xy_c5x7"])
def test_layers_end_to_end(name, transpose):
    from dmcf_amd.utils.convolutions import SparseConv, SparseConvTranspose
    c = _case(name)
    layer = (SparseConvTranspose if transpose else SparseConv)(filters=c.cout, kernel_size=c.kernel_size, activation="relu",
                                                               use_bias=c.bias is not None, normalize=c.normalize,
                                                               offset=None if np.array_equal(c.offset, sr.default_offset(c.kernel_size)) else c.offset)
    F = _t(c.F)
    layer.build(c.cin, F.device)
    with torch.no_grad():
        layer.kernel.copy_(_t(c.W))
        if c.bias is not None:
            layer.bias.copy_(_t(c.bias))
    kw = {"out_importance" if transpose else "inp_importance": _t(c.out_importance if transpose else c.inp_importance)}
    out = layer(F, _t(c.inp), _t(c.out), c.voxel, **kw)
    assert not out.requires_grad
    ref, A = c.forward(transpose)
    _note("layers", sr.check(out.cpu().numpy(), np.maximum(ref, 0.0), A, c.kbar(transpose), name))
    nns = layer.nns_inp if transpose else layer.nns
    want = c.transpose_list if transpose else c.conv_list
    assert np.array_equal(nns.neighbors_row_splits.cpu().numpy(), want[1])
    assert abs(layer._avg_neighbors - want[0].size / c.out.shape[0]) < 1e-9
    assert set(layer._conv_values) >= {"filters", "out_positions", "offset", "inp_positions", "inp_features", "neighbors_index",
                                       "neighbors_row_splits", "normalize"}
    # trainable after requires_grad_(True)
    layer.requires_grad_(True)
    layer(F, _t(c.inp), _t(c.out), c.voxel, **kw).square().sum().backward()
    assert layer.kernel.grad is not None and float(layer.kernel.grad.abs().sum()) > 0
    if c.bias is not None:
        assert layer.bias.grad is not None and float(layer.bias.grad.abs().sum()) > 0


@pytest.mark.parametrize("name", ["k3_c32x32", "k3_c8x16_20k"])
def test_backward_is_deterministic(name):
    from dmcf_amd import ops
    c = _case(name)
    conv = _lists(name)[0]
    args = (_t(c.W), _t(c.out), _t(c.inp), _t(c.F), conv[0], conv[1], float(sr.extent(c.kernel_size, c.voxel)), list(c.offset))
    a = ops.sparse_gather_backward(*args, grad_out=_t(c.G))
    b = ops.sparse_gather_backward(*args, grad_out=_t(c.G))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_empty_sets_return_the_bias():
    from dmcf_amd import ops
    dev = _dev()
    W = torch.ones(3, 3, 3, 2, 4, device=dev)
    bias = torch.arange(4, dtype=torch.float32, device=dev)
    P, none = torch.rand(5, 3, device=dev), torch.zeros(0, 3, device=dev)
    e_idx = torch.zeros(0, dtype=torch.int32, device=dev)
    out = ops.sparse_conv(W, P, 1.0, [0, 0, 0], none, torch.zeros(0, 2, device=dev), e_idx, torch.zeros(6, dtype=torch.int64, device=dev),
                          bias=bias)
    assert torch.equal(out, bias.expand(5, 4))
    out = ops.sparse_conv(W, none, 1.0, [0, 0, 0], P, torch.zeros(5, 2, device=dev), e_idx, torch.zeros(1, dtype=torch.int64, device=dev))
    assert tuple(out.shape) == (0, 4)
