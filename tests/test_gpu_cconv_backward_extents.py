"""GPU checks of the CConv / ASCC backward with one filter extent per output point (dmcf_cconv_backward_extents, ABI 2.15) and of
its surfaces: ops.cconv_backward with a tensor extent, and the two that record only on request (record_per_point_extents=True;
without it they refuse, as tests/test_gpu_cconv_backward.py holds them to): ops.cconv_forward under autograd with a tensor
extent, ContinuousConv's training path with extents of rank 1.

The comparison is the rule of tests/test_gpu_cconv_backward.py, element by element against the float64 restatement
(tests/cconv_backward_ref.py, PairWeights with one extent per output row):
    |gpu - ref| <= K_BAR * 2^-24 * A
A: the same gradient formed from the absolute values of every term.  The lists come from ops.radius_search at radii =
extents / 2.  Run with -s: test_report_worst_ratio prints the worst err / bar of every group."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import cconv_backward_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

K_BAR = 256  # (tests/test_gpu_cconv_backward.py)
GROUPS = np.float32(2) * np.array([0.10, 0.13, 0.16, 0.20], dtype=np.float32)


def _dev():
    return torch.device("cuda:0")


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _n(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t


def _group_extents(rng, n):
    return GROUPS[rng.integers(0, len(GROUPS), size=n)]


def _search(inp_pos, out_pos, ext, ignore_query_point=False):
    from dmcf_amd import ops
    nns = ops.radius_search(_t(inp_pos), _t(out_pos), _t(np.float32(0.5) * ext), ignore_query_point=ignore_query_point,
                            return_distances=False)
    return nns.neighbors_index, nns.neighbors_row_splits


def _pad(idx, rs, stride):
    """The CSR list as a padded one: row i = [i * stride, i * stride + count[i]), the slots behind a row's end hold garbage."""
    counts = torch.diff(rs)
    assert int(counts.max()) <= stride
    n = counts.shape[0]
    begin = torch.arange(n + 1, device=rs.device, dtype=torch.int64) * stride
    buf = torch.full((n * stride,), 12345, dtype=torch.int32, device=rs.device)
    rows = torch.repeat_interleave(torch.arange(n, device=rs.device), counts)
    slot = torch.arange(idx.shape[0], device=rs.device) - rs[:-1][rows]
    buf[rows * stride + slot] = idx
    return buf, begin, counts.to(torch.int32)


def _reference(out_pos, inp_pos, idx, rs, ext, filt, feat, G, *, window="poly6", nval=None, imp=None, align_corners=True,
               mapping="ball_to_cube_volume_preserving", interpolation="linear", normalize=False, symmetric=False, sym_axis=2,
               row_count=None):
    """((d filters, d feats), (their A)) in float64 with one extent per output row."""
    ks = list(filt.shape[:3])
    if symmetric:
        ks[sym_axis] *= 2
    pw = ref.PairWeights(out_pos, inp_pos, _n(idx), _n(rs), np.asarray(ext, dtype=np.float32), ks, window=window, nval=_n(nval),
                         inp_importance=imp, align_corners=align_corners, mapping=mapping, interpolation=interpolation,
                         row_count=_n(row_count))
    rkw = dict(normalize=normalize, symmetric=symmetric, sym_axis=sym_axis)
    rw, rf, _ = ref.grads(pw, filt, feat, G, **rkw)
    aw, af, _ = ref.grads(pw, filt, feat, G, abs_mode=True, **rkw)
    return (rw, rf), (aw, af)


def _compare(tag, got, want, bound):
    ref.check(tag + ":filters", _n(got[0]), want[0], bound[0], K_BAR)
    ref.check(tag + ":features", _n(got[1]), want[1], bound[1], K_BAR)


def _case(tag, out_pos, inp_pos, ext, filt, feat, *, padded=False, ignore_query_point=False, seed=0, imp=None, **opt):
    """ops.cconv_backward with the tensor ``ext`` against the reference; returns the call's operands for further calls."""
    from dmcf_amd import ops
    idx, rs = _search(inp_pos, out_pos, ext, ignore_query_point)
    row_count = None
    if padded:
        idx, rs, row_count = _pad(idx, rs, 64)
    nval = None
    if opt.get("window", "poly6") == "explicit":
        nval = _t(np.random.default_rng(seed + 7).uniform(0.1, 1.0, size=idx.shape[0]).astype(np.float32))
    G = np.random.default_rng(seed + 3).normal(size=(out_pos.shape[0], filt.shape[4])).astype(np.float32)
    kw = dict(neighbors_value=nval, window=opt.get("window", "poly6"), inp_importance=_t(imp),
              align_corners=opt.get("align_corners", True), coordinate_mapping=opt.get("mapping", "ball_to_cube_volume_preserving"),
              interpolation=opt.get("interpolation", "linear"), normalize=opt.get("normalize", False),
              symmetric=opt.get("symmetric", False), sym_axis=opt.get("sym_axis", 2), neighbors_row_count=row_count)
    args = (_t(filt), _t(out_pos), _t(ext), _t(inp_pos), _t(feat), idx, rs, _t(G))
    got = ops.cconv_backward(*args, **kw)
    torch.cuda.synchronize()
    want, bound = _reference(out_pos, inp_pos, idx, rs, ext, filt, feat, G, nval=nval, imp=imp, row_count=row_count, **opt)
    _compare(tag, got, want, bound)
    return args, kw, got, want, bound


OPTIONS = [
    dict(),
    dict(window=None),
    dict(window="explicit"),
    dict(window="cubic"),
    dict(normalize=True),
    dict(normalize=True, window="cubic"),
    dict(align_corners=False),
    dict(mapping="ball_to_cube_radial"),
    dict(mapping="identity"),
    dict(interpolation="linear_border"),
    dict(interpolation="nearest_neighbor"),
    dict(imp=True),
    dict(padded=True),
]


@pytest.mark.parametrize("opt", OPTIONS, ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()) or "default")
def test_options_against_float64(opt):
    opt = dict(opt)
    rng = np.random.default_rng(1)
    pos = rng.uniform(0, 1, size=(600, 3)).astype(np.float32)
    cin, cout = 5, 7
    feat = rng.normal(size=(600, cin)).astype(np.float32)
    filt = rng.uniform(-1, 1, size=(4, 4, 4, cin, cout)).astype(np.float32)
    ext = _group_extents(rng, 600)
    if opt.pop("imp", False):
        opt["imp"] = rng.uniform(0.2, 2.0, size=600).astype(np.float32)
    _case("ext_options", pos, pos, ext, filt, feat, **opt)


def test_continuous_extents_on_distinct_sets():
    """Every row its own extent, 300 outputs over 450 other inputs: the inverted list is not the forward list."""
    rng = np.random.default_rng(2)
    inp_pos = rng.uniform(0, 1, size=(450, 3)).astype(np.float32)
    out_pos = rng.uniform(0, 1, size=(300, 3)).astype(np.float32)
    ext = rng.uniform(0.2, 0.4, size=300).astype(np.float32)
    assert np.unique(ext).size == 300
    cin, cout = 5, 7
    feat = rng.normal(size=(450, cin)).astype(np.float32)
    filt = rng.uniform(-1, 1, size=(4, 4, 4, cin, cout)).astype(np.float32)
    args, _, got, _, _ = _case("ext_continuous", out_pos, inp_pos, ext, filt, feat)
    assert tuple(got[1].shape) == (450, cin)
    # NORMALIZE on these sets with the window whose float32 value the reference reproduces bit for bit (poly6).  Not "cubic"
    # here: without a self pair a row can consist of pairs at the window's edge (row 279: two pairs at 1 - s = 1.6e-3, psi =
    # 2.5e-8), where one ulp of the kernel's v_sqrt_f32 moves a_p / psi_i by 1e-4 -- the conditioning of the normalised layer,
    # the scalar call's too, not an error of a sum that A bounds.  (cubic + NORMALIZE: test_options_against_float64's sets.)
    _case("ext_continuous", out_pos, inp_pos, ext, filt, feat, normalize=True)


@pytest.mark.parametrize("sym_axis,cin", [(0, 4), (2, 4), (2, 1), (0, 70)])
def test_ascc_half_kernels(sym_axis, cin):
    """Each pair at the extent of its output row, the centre term of row i at e_i; Cin = 1 / 70: both branches of the final
    contraction of cconv_bwd_input."""
    rng = np.random.default_rng(3)
    pos = rng.uniform(0, 1, size=(600, 3)).astype(np.float32)
    cout = 3
    feat = rng.normal(size=(600, cin)).astype(np.float32)
    sh = [4, 4, 4]
    sh[sym_axis] = 2
    filt = rng.uniform(-1, 1, size=(*sh, cin, cout)).astype(np.float32)
    ext = _group_extents(rng, 600)
    _, _, got, _, _ = _case("ext_ascc", pos, pos, ext, filt, feat, symmetric=True, sym_axis=sym_axis, ignore_query_point=True)
    assert tuple(got[0].shape) == tuple(filt.shape)


@pytest.mark.parametrize("symmetric,normalize", [(False, False), (False, True), (True, False)], ids=["cconv", "normalize", "ascc"])
def test_constant_extents_equal_the_scalar_call(symmetric, normalize):
    """extents = full(n_out, e) and the scalar e do the same arithmetic per pair: identical bits."""
    from dmcf_amd import ops
    rng = np.random.default_rng(4)
    pos = rng.uniform(0, 1, size=(600, 3)).astype(np.float32)
    cin, cout = 5, 7
    e = float(np.float32(0.3))
    P, F = _t(pos), _t(rng.normal(size=(600, cin)).astype(np.float32))
    W = _t(rng.uniform(-1, 1, size=(4, 4, 2 if symmetric else 4, cin, cout)).astype(np.float32))
    G = _t(rng.normal(size=(600, cout)).astype(np.float32))
    nns = ops.fixed_radius_search(P, P, 0.5 * e, ignore_query_point=symmetric, return_distances=False)
    lists = (nns.neighbors_index, nns.neighbors_row_splits)
    kw = dict(window="poly6", symmetric=symmetric, sym_axis=2, normalize=normalize)
    a = ops.cconv_backward(W, P, e, P, F, *lists, G, **kw)
    b = ops.cconv_backward(W, P, torch.full((600,), e, device=_dev()), P, F, *lists, G, **kw)
    c = ops.cconv_backward(W, P, torch.full((600, 1), e, device=_dev()), P, F, *lists, G, **kw)
    for x, y in ((a, b), (a, c)):
        dw, df = (x[0] - y[0]).abs().max().item(), (x[1] - y[1]).abs().max().item()
        assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]), f"largest differences: filters {dw:.3g}, features {df:.3g}"


def _raw_backward(W, P_out, P_inp, F, idx, rs, G, ext, **kw):
    """dmcf_cconv_backward_extents through the C ABI (ops.cconv_backward refuses extents that are not finite and positive)."""
    from dmcf_amd import _lib, ops
    L = _lib.lib()
    a, keep = ops._cconv_args(W, P_out, 1.0, P_inp, F, idx, rs, neighbors_value=None, window=kw.get("window", "poly6"),
                              window_fac=1.0, inp_importance=None, align_corners=True,
                              coordinate_mapping="ball_to_cube_volume_preserving", interpolation="linear",
                              normalize=kw.get("normalize", False), symmetric=kw.get("symmetric", False),
                              sym_axis=kw.get("sym_axis", 2), bias=None, out=None, accumulate=False)
    inv = ops.invert_neighbors_list(P_inp.shape[0], idx, rs)
    gw = torch.full(tuple(W.shape), 7.0, device=W.device)
    gf = torch.full((P_inp.shape[0], W.shape[3]), 7.0, device=W.device)
    b = _lib.CconvBackwardArgs()
    b.struct_size = ctypes.sizeof(_lib.CconvBackwardArgs)
    b.grad_out = G.data_ptr()
    b.inv_index, b.inv_pair = inv.neighbors_index.data_ptr(), inv.pair_index.data_ptr()
    b.inv_row_splits = inv.neighbors_row_splits.data_ptr()
    b.inv_n_rows, b.inv_n_pairs = P_inp.shape[0], inv.neighbors_index.shape[0]
    b.grad_filters, b.grad_inp_features = gw.data_ptr(), gf.data_ptr()
    a.extent = 0.0  # (ignored)
    sized = _lib.CconvArgs.from_buffer_copy(a)
    sized.extent = 1.0
    nbytes = int(L.dmcf_cconv_backward_workspace_bytes(ctypes.byref(sized), ctypes.byref(b)))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=W.device)
    _lib.check(L.dmcf_cconv_backward_extents(ctypes.byref(a), ctypes.byref(b), ctypes.c_void_p(ext.data_ptr()),
                                             ctypes.c_void_p(ws.data_ptr()), nbytes, ops._stream()), "dmcf_cconv_backward_extents")
    torch.cuda.synchronize()
    del keep
    return gw, gf


@pytest.mark.parametrize("mode", ["plain", "normalize", "ascc"])
def test_invalid_rows_are_empty(mode):
    """Rows whose extent is 0, negative, inf or nan contribute nothing: the gradients are those of the list without their pairs."""
    rng = np.random.default_rng(5)
    n = 400
    pos = rng.uniform(0, 1, size=(n, 3)).astype(np.float32)
    cin, cout = 5, 7
    sym = mode == "ascc"
    feat = rng.normal(size=(n, cin)).astype(np.float32)
    filt = rng.uniform(-1, 1, size=(4, 4, 2 if sym else 4, cin, cout)).astype(np.float32)
    G = rng.normal(size=(n, cout)).astype(np.float32)
    ext = _group_extents(rng, n)
    idx, rs = _search(pos, pos, ext, ignore_query_point=sym)
    bad = np.zeros(n, dtype=bool)
    bad_ext = ext.copy()
    for k, v in enumerate((0.0, -0.3, np.inf, np.nan, 0.0, -np.inf)):
        rows = np.arange(7 + k, n, 41)
        bad[rows] = True
        bad_ext[rows] = v
    counts = np.diff(_n(rs))
    assert counts[bad].sum() > 0
    kw = dict(normalize=mode == "normalize", symmetric=sym, sym_axis=2)
    gw, gf = _raw_backward(_t(filt), _t(pos), _t(pos), _t(feat), idx, rs, _t(G), _t(bad_ext), **kw)
    # the reference: the same list with the bad rows emptied (their extents are then irrelevant)
    keep = np.repeat(~bad, counts)
    idx2 = _n(idx)[keep]
    rs2 = np.concatenate([[0], np.cumsum(np.where(bad, 0, counts))]).astype(np.int64)
    want, bound = _reference(pos, pos, idx2, rs2, np.where(bad, np.float32(1), ext), filt, feat, G, **kw)
    _compare("ext_invalid", (gw, gf), want, bound)
    assert np.all(np.isfinite(_n(gw))) and np.all(np.isfinite(_n(gf)))


def test_bitwise_reproducible_and_accumulate():
    from dmcf_amd import ops
    rng = np.random.default_rng(6)
    pos = rng.uniform(0, 1, size=(600, 3)).astype(np.float32)
    cin, cout = 5, 7
    feat = rng.normal(size=(600, cin)).astype(np.float32)
    filt = rng.uniform(-1, 1, size=(4, 4, 4, cin, cout)).astype(np.float32)
    ext = _group_extents(rng, 600)
    args, kw, a, want, bound = _case("ext_plain", pos, pos, ext, filt, feat, normalize=True)
    b = ops.cconv_backward(*args, **kw)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    init_w = rng.normal(size=filt.shape).astype(np.float32)
    init_f = rng.normal(size=feat.shape).astype(np.float32)
    c = ops.cconv_backward(*args, grad_filters=_t(init_w), grad_inp_features=_t(init_f), accumulate=True, **kw)
    # (the sum with the prior content rounds once more, on |prior| + A)
    _compare("ext_accumulate", c, (want[0] + init_w, want[1] + init_f), (bound[0] + np.abs(init_w), bound[1] + np.abs(init_f)))
    # ... and is the plain call's result added once, in float32
    assert torch.equal(c[0], _t(init_w) + a[0]) and torch.equal(c[1], _t(init_f) + a[1])


def test_kernel_names_reach_the_timer():
    from dmcf_amd import ops
    rng = np.random.default_rng(7)
    P = _t(rng.uniform(0, 1, size=(200, 3)).astype(np.float32))
    ext = _t(_group_extents(rng, 200))
    nns = ops.radius_search(P, P, 0.5 * ext, return_distances=False)
    W, F, G = torch.randn(4, 4, 4, 3, 2, device=_dev()), torch.randn(200, 3, device=_dev()), torch.randn(200, 2, device=_dev())
    timer = ops.LaunchTimer()
    old, ops.timer = ops.timer, timer
    try:
        ops.cconv_backward(W, P, ext, P, F, nns.neighbors_index, nns.neighbors_row_splits, G, window="poly6", normalize=True)
        ops.cconv_backward(W, P, 0.3, P, F, nns.neighbors_index, nns.neighbors_row_splits, G, window="poly6", normalize=True)
    finally:
        ops.timer = old
    names = [m["kernel"] for kind, m, *_ in timer.records if kind == "cconv_backward"]
    assert names[0].split(";")[:3] == ["cconv_bwd_norm_ext", "cconv_bwd_input_ext", "cconv_bwd_filter_splat_ext"]
    assert "_ext" not in names[1]


def test_invalid_extents_are_refused_by_ops():
    from dmcf_amd import ops
    P = torch.rand(10, 3, device=_dev())
    W, F, G = torch.ones(4, 4, 4, 2, 3, device=_dev()), torch.rand(10, 2, device=_dev()), torch.rand(10, 3, device=_dev())
    rs = torch.zeros(11, dtype=torch.int64, device=_dev())
    idx = torch.zeros(0, dtype=torch.int32, device=_dev())
    for v in (0.0, -1.0, float("inf"), float("nan")):
        ext = torch.full((10,), 0.2, device=_dev())
        ext[3] = v
        with pytest.raises(ValueError):
            ops.cconv_backward(W, P, ext, P, F, idx, rs, G, window="poly6")
    gw, gf = ops.cconv_backward(W, P, torch.full((10,), 0.2, device=_dev()), P, F, idx, rs, G, window="poly6")
    assert torch.count_nonzero(gw) == 0 and torch.count_nonzero(gf) == 0


def test_autograd_through_ops():
    from dmcf_amd import ops
    rng = np.random.default_rng(8)
    n = 600
    P = _t(rng.uniform(0, 1, size=(n, 3)).astype(np.float32))
    ext = _t(_group_extents(rng, n))
    F = torch.randn(n, 8, device=_dev())
    W = torch.randn(4, 4, 4, 8, 16, device=_dev())
    bias = torch.randn(16, device=_dev())
    nns = ops.radius_search(P, P, 0.5 * ext, return_distances=False)
    lists = (nns.neighbors_index, nns.neighbors_row_splits)
    plain = ops.cconv_forward(W, P, ext, P, F, *lists, window="poly6", bias=bias)
    assert plain.grad_fn is None
    Wg, Fg, bg = W.clone().requires_grad_(True), F.clone().requires_grad_(True), bias.clone().requires_grad_(True)
    eg = ext.clone().reshape(n, 1).requires_grad_(True)
    with pytest.raises(NotImplementedError):  # recording with per-point extents is opt-in
        ops.cconv_forward(Wg, P, eg, P, Fg, *lists, window="poly6", bias=bg)
    out = ops.cconv_forward(Wg, P, eg, P, Fg, *lists, window="poly6", bias=bg, record_per_point_extents=True)
    assert out.grad_fn is not None and torch.equal(out.detach(), plain)
    G = torch.randn_like(out)
    out.backward(G)
    gw, gf = ops.cconv_backward(W, P, ext, P, F, *lists, G, window="poly6")
    assert torch.equal(Wg.grad, gw) and torch.equal(Fg.grad, gf)
    assert torch.allclose(bg.grad, G.sum(0))
    assert eg.grad is None  # extents get no gradient
    # only one of the two wanted
    out = ops.cconv_forward(W, P, ext, P, F.clone().requires_grad_(True), *lists, window="poly6", record_per_point_extents=True)
    assert out.grad_fn is not None
    with pytest.raises(ValueError):
        ops.cconv_forward(Wg, P, ext, P, Fg, *lists, window="poly6", out=torch.empty_like(plain), record_per_point_extents=True)
    with pytest.raises(ValueError):
        ops.cconv_forward(Wg, P, ext, P, Fg, *lists, window="poly6", out=torch.empty_like(plain), accumulate=True,
                          record_per_point_extents=True)
    # the flag changes nothing when nothing records
    assert torch.equal(ops.cconv_forward(W, P, ext, P, F, *lists, window="poly6", bias=bias, record_per_point_extents=True), plain)


# ---- the layer ----------------------------------------------------------------------------------------------------------------

def _poly6(q):
    return torch.clamp(1.0 - q, min=0.0) ** 3


LAYER_CASES = [
    dict(symmetric=False, window="named"),
    dict(symmetric=False, window="callable"),
    dict(symmetric=True, window="named"),
    dict(symmetric=True, window="callable"),
    dict(symmetric=False, window="named", dense=True),
    dict(symmetric=False, window="named", user_list=True),
]


@pytest.mark.parametrize("case", LAYER_CASES, ids=lambda c: ",".join(f"{k}={v}" for k, v in c.items()))
def test_layer_trains_with_rank1_extents(case, monkeypatch):
    """ContinuousConv(record_per_point_extents=True) with requires_grad_(True) and extents of rank 1: the forward against the no_grad forward of the same layer,
    kernel / bias / dense / input-feature gradients against the layer restated in float64."""
    from dmcf_amd import ops
    from dmcf_amd.utils.convolutions import ContinuousConv
    from dmcf_amd.utils.tools.losses import get_window_func
    dev = _dev()
    rng = np.random.default_rng(9)
    n, cin, cout = 500, 5, 6
    sym, dense = case["symmetric"], case.get("dense", False)
    pos = rng.uniform(0, 1, size=(n, 3)).astype(np.float32)
    ext = _group_extents(rng, n)
    P, E = _t(pos), _t(ext)
    x = _t(rng.normal(size=(n, cin)).astype(np.float32))
    layer = ContinuousConv(cout, [4, 4, 4], window_function=get_window_func("poly6") if case["window"] == "named" else _poly6,
                           coordinate_mapping="ball_to_cube_volume_preserving", normalize=not sym, symmetric=sym, sym_axis=2,
                           radius_search_ignore_query_points=sym, use_dense_layer_for_center=dense,
                           activation="relu" if dense else None, device=dev, record_per_point_extents=True)
    extra = {}
    if case.get("user_list"):
        nns = ops.radius_search(P, P, 0.5 * E, return_distances=False)
        imp = torch.rand(nns.neighbors_index.shape[0], device=dev) + 0.1
        extra = dict(user_neighbors_index=nns.neighbors_index, user_neighbors_row_splits=nns.neighbors_row_splits,
                     user_neighbors_importance=imp)
    call = lambda f: layer(f, P, P, E, **extra)  # noqa: E731
    with torch.no_grad():
        call(x)  # (builds the weights)
        gen = torch.Generator(device=dev).manual_seed(5)
        for p in layer.parameters():
            p.copy_(torch.rand(p.shape, device=dev, generator=gen) * 2 - 1)
        y_inf = call(x).clone()
    with pytest.raises(ValueError):
        layer(x, P, P, E[:-1].contiguous())
    layer.requires_grad_(True)
    layer.record_per_point_extents = False  # (the default of the constructor: such a layer refuses, whatever its weights)
    with pytest.raises(NotImplementedError):
        call(x)
    layer.record_per_point_extents = True
    # record the layer's one CConv call and the gradient that reaches its output
    calls, real = [], ops.cconv_forward

    def rec(*a, **k):
        res = real(*a, **k)
        if isinstance(res, torch.Tensor) and res.requires_grad:
            entry = dict(args=a, kw=k)
            res.register_hook(lambda g: entry.__setitem__("grad", g.detach().clone()))
            calls.append(entry)
        return res
    monkeypatch.setattr(ops, "cconv_forward", rec)
    xg = x.clone().requires_grad_(True)
    y = call(xg)
    Gy = torch.randn(y.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(6))
    (y * Gy).sum().backward()
    monkeypatch.setattr(ops, "cconv_forward", real)
    assert len(calls) == 1 and "grad" in calls[0], "the layer's CConv was not recorded by autograd"
    a, k = calls[0]["args"], calls[0]["kw"]
    assert isinstance(a[2], torch.Tensor) and tuple(a[2].shape) == (n,) and not a[2].requires_grad
    assert k["window"] == ("poly6" if case["window"] == "named" and not extra else "explicit")
    assert k["symmetric"] == sym and tuple(layer.kernel.shape[:3]) == ((4, 4, 2) if sym else (4, 4, 4))
    # the layer in float64 on the recorded list
    dims = [4, 4, 4]
    pw = ref.PairWeights(pos, pos, _n(a[5]), _n(a[6]), ext, dims, window=k["window"], window_fac=k.get("window_fac", 1.0),
                         nval=_n(k.get("neighbors_value")))
    rkw = dict(normalize=not sym, symmetric=sym, sym_axis=2)
    W64 = layer.kernel.detach().double().cpu().requires_grad_(True)
    x64 = x.double().cpu().requires_grad_(True)
    b64 = layer.bias.detach().double().cpu().requires_grad_(True)
    with torch.enable_grad():
        pre = ref.conv(pw, W64, x64, **rkw)
        if dense:
            d64 = layer.dense.detach().double().cpu().requires_grad_(True)
            pre = pre + x64 @ d64
        pre = pre + b64
        y64 = torch.relu(pre) if dense else pre
        (y64 * Gy.double().cpu()).sum().backward()
    Gc = np.abs(_n(calls[0]["grad"]).astype(np.float64))  # |gradient reaching the CConv output|
    aw, af, _ = ref.grads(pw, _n(layer.kernel), _n(x), Gc, abs_mode=True, **rkw)
    ya = ref.conv(pw, layer.kernel.detach().double().cpu().abs(), x.double().cpu().abs(), abs_mode=True, **rkw).numpy()
    ya = ya + np.abs(_n(layer.bias))
    xa = np.abs(_n(x).astype(np.float64))
    if dense:
        da = np.abs(_n(layer.dense).astype(np.float64))
        af = af + Gc @ da.T
        ya = ya + xa @ da
        ref.check("ext_layer:dense", _n(layer.dense.grad), d64.grad.numpy(), xa.T @ Gc, K_BAR)
    ref.check("ext_layer:kernel", _n(layer.kernel.grad), W64.grad.numpy(), aw, K_BAR)
    ref.check("ext_layer:bias", _n(layer.bias.grad), b64.grad.numpy(), Gc.sum(0), K_BAR)
    ref.check("ext_layer:x", _n(xg.grad), x64.grad.numpy(), af, K_BAR)
    # (relu: 1-Lipschitz, so the bar of the pre-activation sum carries over)
    ref.check("ext_layer:forward", _n(y), _n(y_inf).astype(np.float64), ya, K_BAR)
    ref.check("ext_layer:forward", _n(y), y64.detach().numpy(), ya, K_BAR)


def test_report_worst_ratio():
    """Prints the worst err / bar of every group above (run with -s)."""
    print("K_BAR", K_BAR, "worst err/bar", {k: round(v, 4) for k, v in ref.WORST.items() if k.startswith("ext_")})
