"""GPU tests of per-point filter extents: the radius search with one radius per query (ops.radius_search / RadiusSearch), the
CConv / ASCC with individual extents (dmcf_cconv_forward_extents) and the rank-1 branch of the layers.

References live here: a float32 numpy brute force with the un-fused ((dx*dx + dy*dy) + dz*dz) for the search, and
oracle.continuous_conv (a scalar extent) called once per distinct extent on the rows that carry it.  Bars: neighbour sets and
squared distances bit-exact, normalised distances within 1 ulp; CConv max |err| / max |ref| <= 1e-5 (2e-5 with windows) and,
per row, |err| <= tol * max |ref_row| + 1e-6 -- small-extent rows next to large ones are checked on their own scale."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

MAPPINGS = ["ball_to_cube_radial", "ball_to_cube_volume_preserving", "identity"]
INTERPOLATIONS = ["linear", "linear_border", "nearest_neighbor"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but torch.cuda.is_available() is False")
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def brute_force(points, queries, radii, ignore_query_point=False):
    """-> (index int32, row_splits int64, d2 float32): rows in ascending point index, float32 un-fused distances."""
    points = np.asarray(points, np.float32)
    queries = np.asarray(queries, np.float32)
    r2 = np.asarray(radii, np.float32) * np.asarray(radii, np.float32)
    idx, cnt, dist = [], [], []
    for q0 in range(0, queries.shape[0], 256):
        q = queries[q0:q0 + 256]
        dx = points[None, :, 0] - q[:, None, 0]
        dy = points[None, :, 1] - q[:, None, 1]
        dz = points[None, :, 2] - q[:, None, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        hit = d2 <= r2[q0:q0 + 256, None]
        if ignore_query_point:
            hit &= ~((dx == 0) & (dy == 0) & (dz == 0))
        rows, cols = np.nonzero(hit)
        idx.append(cols.astype(np.int32))
        dist.append(d2[rows, cols])
        cnt.append(hit.sum(axis=1))
    if queries.shape[0] == 0:
        return np.zeros(0, np.int32), np.zeros(1, np.int64), np.zeros(0, np.float32)
    rs = np.concatenate([[0], np.cumsum(np.concatenate(cnt))]).astype(np.int64)
    return np.concatenate(idx), rs, np.concatenate(dist).astype(np.float32)


def _canonical(idx, rs, *per_pair):
    row = np.repeat(np.arange(len(rs) - 1), np.diff(rs))
    order = np.lexsort((idx, row))
    return (idx[order],) + tuple(p[order] for p in per_pair)


def _scene(seed, n=20000, m=5000, dim=3):
    rng = np.random.default_rng(seed)
    pts = rng.uniform(-1, 1, size=(n, 3)).astype(np.float32)
    pts[1000:1040] = pts[:40]  # coincident points
    qs = rng.uniform(-1.1, 1.1, size=(m, 3)).astype(np.float32)
    qs[:600] = pts[:600]  # queries at points
    if dim == 2:
        pts[:, 2] = 0
        qs[:, 2] = 0
    radii = rng.uniform(0.04, 0.16, size=m).astype(np.float32)  # a 4x range
    radii[::37] = 0.0
    return pts, qs, radii


def _check_rows(res, ref, radii, normalized):
    idx, rs, d = (x.cpu().numpy() for x in res)
    i0, r0, d0 = ref
    assert np.array_equal(rs, r0), "row lengths differ from the brute force"
    a, da = _canonical(idx, rs, d)
    b, db = _canonical(i0, r0, d0)
    assert np.array_equal(a, b), "neighbour sets differ from the brute force"
    if not normalized:
        assert np.array_equal(da.view(np.uint32), db.view(np.uint32)), "squared distances are not bit-exact"
        return
    r2 = np.repeat(np.asarray(radii, np.float32) ** 2, np.diff(r0)).astype(np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        want = np.where(r2 > 0, db / r2, np.float32(0)).astype(np.float32)
    assert np.all(np.abs(da - want) <= np.spacing(want)), "normalised distances beyond 1 ulp of d^2 / r^2"


@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("ignore", [False, True])
def test_radius_search_vs_brute_force(dev, dim, ignore):
    from dmcf_amd import ops
    pts, qs, radii = _scene(1 + dim, dim=dim)
    ref = brute_force(pts, qs, radii, ignore)
    P, Q, R = _t(pts, dev), _t(qs, dev), _t(radii, dev)
    res = ops.radius_search(P, Q, R, ignore_query_point=ignore, normalize_distances=False)
    _check_rows(res, ref, radii, normalized=False)
    res = ops.RadiusSearch(ignore_query_point=ignore, return_distances=True, normalize_distances=True)(P, Q, R)
    _check_rows(res, ref, radii, normalized=True)
    if not ignore:
        # radius-0 rows hold exactly the points at the query's coordinates
        zero = np.nonzero(radii == 0)[0]
        idx, rs = res.neighbors_index.cpu().numpy(), res.neighbors_row_splits.cpu().numpy()
        for i in zero[:40]:
            same = np.nonzero(np.all(pts == qs[i], axis=1))[0]
            assert np.array_equal(np.sort(idx[rs[i]:rs[i + 1]]), same)
        assert any(rs[i + 1] - rs[i] >= 2 for i in zero if i < 40)  # (the coincident points are found twice)


def test_radius_search_points_equal_queries_and_empty(dev):
    from dmcf_amd import ops
    rng = np.random.default_rng(7)
    pts = rng.uniform(0, 1, size=(6000, 3)).astype(np.float32)
    radii = rng.uniform(0.03, 0.12, size=6000).astype(np.float32)
    P, R = _t(pts, dev), _t(radii, dev)
    for ignore in (False, True):
        res = ops.radius_search(P, P, R, ignore_query_point=ignore, normalize_distances=False)
        _check_rows(res, brute_force(pts, pts, radii, ignore), radii, normalized=False)
    # no points: every row empty; no queries: one row split
    res = ops.radius_search(P[:0], P, R)
    assert res.neighbors_row_splits.cpu().numpy().tolist() == [0] * 6001 and res.neighbors_index.numel() == 0
    res = ops.radius_search(P, P[:0], R[:0])
    assert res.neighbors_row_splits.cpu().numpy().tolist() == [0] and res.neighbors_index.numel() == 0
    with pytest.raises(ValueError):
        ops.radius_search(P, P, R[:10])
    bad = R.clone()
    bad[5] = float("nan")
    with pytest.raises(ValueError):
        ops.radius_search(P, P, bad)
    bad[5] = -0.1
    with pytest.raises(ValueError):
        ops.radius_search(P, P, bad)


def test_radius_search_equal_radii_is_fixed_radius_search(dev):
    from dmcf_amd import ops
    pts, qs, _ = _scene(11, n=12000, m=3000)
    P, Q = _t(pts, dev), _t(qs, dev)
    r = 0.09
    a = ops.radius_search(P, Q, torch.full((Q.shape[0],), r, device=dev), normalize_distances=False)
    b = ops.fixed_radius_search(P, Q, r)
    ia, ra, da = (x.cpu().numpy() for x in a)
    ib, rb, db = (x.cpu().numpy() for x in b)
    assert np.array_equal(ra, rb)
    ca, cda = _canonical(ia, ra, da)
    cb, cdb = _canonical(ib, rb, db)
    assert np.array_equal(ca, cb) and np.array_equal(cda, cdb)


# ---------------------------------------------------------------------------------------------------------------------------
# CConv with individual extents


def _conv_scene(seed, n_inp=6000, n_out=1000, values=None, span=(0.08, 0.24)):
    rng = np.random.default_rng(seed)
    inp = rng.uniform(0, 1, size=(n_inp, 3)).astype(np.float32)
    out = rng.uniform(0, 1, size=(n_out, 3)).astype(np.float32)
    if values is None:
        ext = rng.uniform(*span, size=n_out).astype(np.float32)
    else:
        ext = rng.choice(np.asarray(values, np.float32), size=n_out).astype(np.float32)
    idx, rs, d2 = brute_force(inp, out, np.float32(0.5) * ext)
    return rng, inp, out, ext, idx, rs, d2


def _group_ref(oracle, ext, idx, rs, conv, per_row=False):
    """Concatenates oracle results computed per distinct extent (or per row): conv(rows, extent, idx_sub, rs_sub, pair_sel)."""
    n_out = ext.shape[0]
    groups = [np.array([i]) for i in range(n_out)] if per_row else [np.nonzero(ext == e)[0] for e in np.unique(ext)]
    res = None
    for rows in groups:
        lens = rs[rows + 1] - rs[rows]
        sel = np.concatenate([np.arange(rs[i], rs[i + 1]) for i in rows]) if lens.sum() else np.zeros(0, np.int64)
        sub_rs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        o = conv(rows, float(ext[rows[0]]), idx[sel], sub_rs, sel)
        if res is None:
            res = np.zeros((n_out, o.shape[1]), np.float32)
        res[rows] = o
    return res


def _check(got, ref, tol):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    err = np.abs(got - ref)
    scale = max(float(np.abs(ref).max()), 1e-30)
    assert err.max() / scale <= tol, f"max |err| / max |ref| = {err.max() / scale:.3g}"
    row_scale = np.abs(ref).max(axis=1, keepdims=True)
    worst = (err - (tol * row_scale + 1e-6)).max()
    assert worst <= 0, f"element-wise bar exceeded by {worst:.3g}"


def _ext_conv(oracle, filt, out, inp, feat, ext, idx, rs, imp=None, **kw):
    def conv(rows, e, sub_idx, sub_rs, sel):
        return oracle.continuous_conv(filt, out[rows], e, inp, feat, sub_idx, sub_rs,
                                      neighbors_importance=None if imp is None else imp[sel], **kw)
    return conv


@pytest.mark.parametrize("mapping", MAPPINGS)
@pytest.mark.parametrize("interp", INTERPOLATIONS)
@pytest.mark.parametrize("align", [True, False])
def test_cconv_extents_mappings(oracle, dev, mapping, interp, align):
    from dmcf_amd import ops
    rng, inp, out, ext, idx, rs, _ = _conv_scene(3, values=[0.08, 0.1, 0.13, 0.16, 0.2, 0.24])
    filt = rng.uniform(-1, 1, size=(4, 4, 4, 8, 16)).astype(np.float32)
    feat = rng.normal(size=(inp.shape[0], 8)).astype(np.float32)
    for normalize in (False, True):
        kw = dict(align_corners=align, coordinate_mapping=mapping, interpolation=interp, normalize=normalize)
        ref = _group_ref(oracle, ext, idx, rs, _ext_conv(oracle, filt, out, inp, feat, ext, idx, rs, **kw))
        got = ops.cconv_forward(_t(filt, dev), _t(out, dev), _t(ext, dev), _t(inp, dev), _t(feat, dev), _t(idx, dev), _t(rs, dev), **kw)
        _check(got, ref, 1e-5)


@pytest.mark.parametrize("dims", [(4, 4, 4), (3, 3, 3), (1, 8, 8)])
@pytest.mark.parametrize("chans", [(1, 8), (8, 16), (24, 64)])
def test_cconv_extents_shapes(oracle, dev, dims, chans):
    from dmcf_amd import ops
    rng, inp, out, ext, idx, rs, _ = _conv_scene(4, values=[0.08, 0.1, 0.13, 0.16, 0.2, 0.24])
    cin, cout = chans
    filt = rng.uniform(-1, 1, size=(*dims, cin, cout)).astype(np.float32)
    feat = rng.normal(size=(inp.shape[0], cin)).astype(np.float32)
    kw = dict(align_corners=True, coordinate_mapping="ball_to_cube_volume_preserving", interpolation="linear")
    ref = _group_ref(oracle, ext, idx, rs, _ext_conv(oracle, filt, out, inp, feat, ext, idx, rs, **kw))
    got = ops.cconv_forward(_t(filt, dev), _t(out, dev), _t(ext, dev).reshape(-1, 1), _t(inp, dev), _t(feat, dev), _t(idx, dev),
                            _t(rs, dev), **kw)
    _check(got, ref, 1e-5)


@pytest.mark.parametrize("window", ["poly6", "cubic"])
@pytest.mark.parametrize("in_kernel", [False, True])
def test_cconv_extents_windows(oracle, dev, window, in_kernel):
    """A distance window on d^2 / r_i^2: from the list's squared distances, or re-formed from the positions in the kernel."""
    from dmcf_amd import ops
    rng, inp, out, ext, idx, rs, d2 = _conv_scene(5, values=[0.08, 0.1, 0.13, 0.16, 0.2, 0.24])
    filt = rng.uniform(-1, 1, size=(4, 4, 4, 8, 16)).astype(np.float32)
    feat = rng.normal(size=(inp.shape[0], 8)).astype(np.float32)
    r2 = np.repeat((np.float32(0.5) * ext) ** 2, np.diff(rs)).astype(np.float32)
    imp = oracle.window(window, d2 / r2)
    kw = dict(align_corners=True, coordinate_mapping="ball_to_cube_volume_preserving", interpolation="linear")
    ref = _group_ref(oracle, ext, idx, rs, _ext_conv(oracle, filt, out, inp, feat, ext, idx, rs, imp=imp, **kw))
    got = ops.cconv_forward(_t(filt, dev), _t(out, dev), _t(ext, dev), _t(inp, dev), _t(feat, dev), _t(idx, dev), _t(rs, dev),
                            neighbors_value=None if in_kernel else _t(d2, dev), window=window, **kw)
    _check(got, ref, 2e-5)


def test_cconv_extents_continuous_padded_accumulate(oracle, dev):
    """300 rows with continuous random extents (a reference call per row); the same through padded rows; ACCUMULATE + bias."""
    from dmcf_amd import ops
    rng, inp, out, ext, idx, rs, _ = _conv_scene(6, n_inp=2000, n_out=300, span=(0.05, 0.3))
    filt = rng.uniform(-1, 1, size=(4, 4, 4, 8, 16)).astype(np.float32)
    feat = rng.normal(size=(inp.shape[0], 8)).astype(np.float32)
    bias = rng.normal(size=16).astype(np.float32)
    kw = dict(align_corners=False, coordinate_mapping="ball_to_cube_radial", interpolation="linear", normalize=True)
    ref = _group_ref(oracle, ext, idx, rs, _ext_conv(oracle, filt, out, inp, feat, ext, idx, rs, **kw), per_row=True)
    F, O, E, I, X = _t(filt, dev), _t(out, dev), _t(ext, dev), _t(inp, dev), _t(feat, dev)
    _check(ops.cconv_forward(F, O, E, I, X, _t(idx, dev), _t(rs, dev), **kw), ref, 1e-5)
    # padded rows: row i at i * stride, the tail of every row holds a valid but wrong index (never read)
    cnt = np.diff(rs).astype(np.int32)
    stride = int(cnt.max()) + 5
    pidx = np.full(300 * stride, 1, np.int32)
    for i in range(300):
        pidx[i * stride:i * stride + cnt[i]] = idx[rs[i]:rs[i + 1]]
    begin = (np.arange(301) * stride).astype(np.int64)
    got = ops.cconv_forward(F, O, E, I, X, _t(pidx, dev), _t(begin, dev), neighbors_row_count=_t(cnt, dev), **kw)
    _check(got, ref, 1e-5)
    # accumulate into an existing tensor, with the bias
    base = rng.normal(size=(300, 16)).astype(np.float32)
    acc = _t(base, dev)
    ops.cconv_forward(F, O, E, I, X, _t(idx, dev), _t(rs, dev), bias=_t(bias, dev), out=acc, accumulate=True, **kw)
    _check(acc, ref + bias + base, 1e-5)


def test_cconv_extents_invalid_rows_give_the_bias(dev):
    """The C ABI: a row whose extent is not positive and finite is zero plus the bias (ops rejects such extents earlier)."""
    import ctypes
    from dmcf_amd import ops, _lib
    _, inp, out, ext, idx, rs, _ = _conv_scene(8, n_inp=1500, n_out=200)
    filt = np.random.default_rng(8).uniform(-1, 1, size=(4, 4, 4, 8, 16)).astype(np.float32)
    feat = np.random.default_rng(9).normal(size=(inp.shape[0], 8)).astype(np.float32)
    bias = _t(np.arange(16, dtype=np.float32), dev)
    E = _t(ext, dev)
    good = ops.cconv_forward(_t(filt, dev), _t(out, dev), E, _t(inp, dev), _t(feat, dev), _t(idx, dev), _t(rs, dev), bias=bias)
    E[3], E[50], E[77], E[120] = 0.0, -0.1, float("inf"), float("nan")
    res = torch.empty_like(good)
    keep = [_t(a, dev) for a in (filt, out, inp, feat, idx, rs)]
    a, _k = ops._cconv_args(keep[0], keep[1], 1.0, keep[2], keep[3], keep[4], keep[5], neighbors_value=None, window=None,
                            window_fac=1.0, inp_importance=None, align_corners=True,
                            coordinate_mapping="ball_to_cube_volume_preserving", interpolation="linear", normalize=False,
                            symmetric=False, sym_axis=2, bias=bias, out=res, accumulate=False)
    L = _lib.lib()
    nbytes = L.dmcf_cconv_workspace_bytes(ctypes.byref(a))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _lib.check(L.dmcf_cconv_forward_extents(ctypes.byref(a), ctypes.c_void_p(E.data_ptr()), ctypes.c_void_p(ws.data_ptr()), nbytes,
                                            ops._stream()), "dmcf_cconv_forward_extents")
    bad = [3, 50, 77, 120]
    assert torch.equal(res[bad], bias.expand(4, 16))
    rest = [i for i in range(200) if i not in bad]
    assert torch.equal(res[rest], good[rest])
    for v in (0.0, float("nan")):
        E2 = _t(ext, dev)
        E2[7] = v
        with pytest.raises(ValueError):
            ops.cconv_forward(keep[0], keep[1], E2, keep[2], keep[3], keep[4], keep[5])


def test_ascc_extents_two_pass(oracle, dev):
    """SYMMETRIC with individual extents = the two continuous_conv calls + batched matmul of convolutions.py:433-458 with
    extents_rank2 = [n_out, 1], per extent group."""
    from dmcf_amd import ops
    rng = np.random.default_rng(12)
    n = 2500
    pos = rng.uniform(0, 1, size=(n, 3)).astype(np.float32)
    ext = rng.choice(np.float32([0.1, 0.13, 0.17, 0.22]), size=n).astype(np.float32)
    idx, rs, _ = brute_force(pos, pos, np.float32(0.5) * ext, ignore_query_point=True)
    cin, cout, sym_axis = 8, 3, 2
    half = rng.uniform(-1, 1, size=(4, 4, 2, cin, cout)).astype(np.float32)
    feat = rng.normal(size=(n, cin)).astype(np.float32)
    full = oracle.mirror_kernel(half, sym_axis)
    kw = dict(align_corners=True, coordinate_mapping="ball_to_cube_volume_preserving", interpolation="linear", normalize=False)

    def conv(rows, e, sub_idx, sub_rs, sel):
        o = oracle.continuous_conv(full, pos[rows], e, pos, feat, sub_idx, sub_rs, **kw)
        w = oracle.continuous_conv(full.reshape(4, 4, 4, 1, cin * cout), pos[rows], e, pos, np.ones((n, 1), np.float32),
                                   sub_idx, sub_rs, **kw).reshape(-1, cin, cout)
        return o + np.einsum("nc,nco->no", feat[rows], w)

    ref = _group_ref(oracle, ext, idx, rs, conv)
    got = ops.cconv_forward(_t(half, dev), _t(pos, dev), _t(ext, dev), _t(pos, dev), _t(feat, dev), _t(idx, dev), _t(rs, dev),
                            symmetric=True, sym_axis=sym_axis, **kw)
    _check(got, ref, 1e-5)


@pytest.mark.parametrize("mapping,align", [("ball_to_cube_volume_preserving", True), ("ball_to_cube_radial", False)])
def test_constant_extents_match_the_scalar_call(dev, mapping, align):
    from dmcf_amd import ops
    rng, inp, out, _, idx, rs, _ = _conv_scene(13, values=[0.15])
    filt = _t(rng.uniform(-1, 1, size=(4, 4, 4, 8, 16)).astype(np.float32), dev)
    feat = _t(rng.normal(size=(inp.shape[0], 8)).astype(np.float32), dev)
    args = (_t(inp, dev), feat, _t(idx, dev), _t(rs, dev))
    kw = dict(align_corners=align, coordinate_mapping=mapping, interpolation="linear", window="poly6")
    O = _t(out, dev)
    a = ops.cconv_forward(filt, O, torch.full((out.shape[0],), 0.15, device=dev), *args, **kw)
    b = ops.cconv_forward(filt, O, 0.15, *args, **kw)
    assert float((a - b).abs().max()) <= 1e-6 * float(b.abs().max())


# ---------------------------------------------------------------------------------------------------------------------------
# the layers' rank-1 branch


def _liquid3d_layer(dev, cin=8, cout=16):
    from dmcf_amd.utils.convolutions import ContinuousConv
    from dmcf_amd.utils.tools.losses import get_window_func
    conv = ContinuousConv(filters=cout, kernel_size=[4, 4, 4], activation=None, align_corners=True, interpolation="linear",
                          coordinate_mapping="ball_to_cube_volume_preserving", normalize=False,
                          window_function=get_window_func("poly6"), use_dense_layer_for_center=True,
                          kernel_initializer="glorot_uniform", device=dev)
    conv.build(cin, dev)
    with torch.no_grad():
        conv.bias.uniform_(-1, 1)
    return conv


def test_layer_rank1_extents(oracle, dev):
    from dmcf_amd import ops
    rng = np.random.default_rng(21)
    n = 3000
    pos = rng.uniform(0, 1, size=(n, 3)).astype(np.float32)
    ext = rng.choice(np.float32([0.08, 0.1, 0.13, 0.16, 0.2, 0.24]), size=n).astype(np.float32)
    feat = rng.normal(size=(n, 8)).astype(np.float32)
    conv = _liquid3d_layer(dev)
    P, X, E = _t(pos, dev), _t(feat, dev), _t(ext, dev)
    got = conv(X, P, P, E)
    # the composition: RadiusSearch (normalised distances) -> window -> continuous_conv per extent group -> dense + bias
    nns = ops.RadiusSearch(return_distances=True, normalize_distances=True)(P, P, 0.5 * E)
    idx, rs, q = (x.cpu().numpy() for x in nns)
    kern, dense, bias = (t.detach().cpu().numpy() for t in (conv.kernel, conv.dense, conv.bias))
    kw = dict(align_corners=True, coordinate_mapping="ball_to_cube_volume_preserving", interpolation="linear", normalize=False)
    ref = _group_ref(oracle, ext, idx, rs, _ext_conv(oracle, kern, pos, pos, feat, ext, idx, rs, imp=oracle.window("poly6", q), **kw))
    _check(got, ref + feat @ dense + bias, 2e-5)
    # user lists: no search, no window (convolutions.py:341-349)
    ui, urs, _ = brute_force(pos, pos, np.float32(0.5) * ext)
    got = conv(X, P, P, E, user_neighbors_index=_t(ui, dev), user_neighbors_row_splits=_t(urs, dev))
    ref = _group_ref(oracle, ext, ui, urs, _ext_conv(oracle, kern, pos, pos, feat, ext, ui, urs, **kw))
    _check(got, ref + feat @ dense + bias, 1e-5)


def test_point_sampling_rank1_extents(oracle, dev):
    from dmcf_amd.utils.convolutions import PointSampling
    from dmcf_amd.utils.tools.losses import get_window_func
    rng = np.random.default_rng(22)
    inp = rng.uniform(0, 1, size=(4000, 3)).astype(np.float32)
    out = rng.uniform(0, 1, size=(800, 3)).astype(np.float32)
    ext = rng.choice(np.float32([0.1, 0.14, 0.2]), size=800).astype(np.float32)
    feat = rng.normal(size=(4000, 1)).astype(np.float32)
    ps = PointSampling(window_function=get_window_func("poly6"), normalize=True)
    got = ps(_t(feat, dev), _t(inp, dev), _t(out, dev), _t(ext, dev))
    idx, rs, d2 = brute_force(inp, out, np.float32(0.5) * ext)
    q = d2 / np.repeat((np.float32(0.5) * ext) ** 2, np.diff(rs)).astype(np.float32)
    kw = dict(align_corners=False, coordinate_mapping="ball_to_cube_radial", interpolation="linear", normalize=True)
    eye = np.eye(1, dtype=np.float32).reshape(1, 1, 1, 1, 1)
    ref = _group_ref(oracle, ext, idx, rs, _ext_conv(oracle, eye, out, inp, feat, ext, idx, rs, imp=oracle.window("poly6", q), **kw))
    _check(got, ref, 2e-5)


def test_scalar_call_after_rank1_call_is_undisturbed(dev):
    """The rank-1 branch neither uses nor overwrites the layer's packed filter, and never enters the neighbour cache."""
    from dmcf_amd.utils.convolutions import neighbor_cache
    rng = np.random.default_rng(23)
    n = 4000
    P = _t(rng.uniform(0, 1, size=(n, 3)).astype(np.float32), dev)
    X = _t(rng.normal(size=(n, 8)).astype(np.float32), dev)
    E = _t(rng.uniform(0.08, 0.2, size=n).astype(np.float32), dev)
    a = _liquid3d_layer(dev)
    b = _liquid3d_layer(dev)
    with torch.no_grad():
        for pa, pb in zip(a.parameters(), b.parameters()):
            pb.copy_(pa)
    first = a(X, P, P, 0.15)
    a(X, P, P, E)
    again = a(X, P, P, 0.15)
    fresh = b(X, P, P, 0.15)
    assert torch.equal(again, fresh) and torch.equal(again, first)
    with neighbor_cache():
        a(X, P, P, E)
        in_step = a(X, P, P, 0.15)
    with neighbor_cache():
        in_step_fresh = b(X, P, P, 0.15)
    assert torch.equal(in_step, in_step_fresh)
