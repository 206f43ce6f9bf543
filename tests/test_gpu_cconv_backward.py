"""GPU checks of the CConv / ASCC backward pass (dmcf_cconv_backward, dmcf_invert_neighbors_list) and of its autograd surface
(ops.cconv_forward under torch.autograd, the ContinuousConv training path).

Gradients are compared element by element with a float64 restatement (tests/cconv_backward_ref.py):
    |gpu - ref| <= K_BAR * 2^-24 * A
where A is the same gradient formed from the absolute values of every term (|weights|, |f|, |W|, |G|)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import cconv_backward_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

K_BAR = 256
EPS = ref.EPS
WORST = ref.WORST  # (shared with tests/test_gpu_cconv_backward_sets.py, whose report prints every group)


def _dev():
    return torch.device("cuda:0")


def _scene(n, seed, dims=3, scale=1.0):
    rng = np.random.default_rng(seed)
    pos = rng.uniform(0, scale, size=(n, 3)).astype(np.float32)
    if dims == 2:
        pos[:, 2] = 0.0
    return rng, pos


def _check(name, got, want, bound):
    ref.check(name, got, want, bound, K_BAR)


def _run(pos, feat, filt, radius, *, window="poly6", use_dist=False, normalize=False, symmetric=False, sym_axis=2,
         align_corners=True, mapping="ball_to_cube_volume_preserving", interpolation="linear", imp=None, skip_self=False,
         padded=False, ignore_query_point=False, seed=0):
    from dmcf_amd import ops
    dev = _dev()
    P = torch.from_numpy(pos).to(dev)
    F = torch.from_numpy(feat).to(dev)
    W = torch.from_numpy(filt).to(dev)
    ks = list(filt.shape[:3])
    if symmetric:
        ks[sym_axis] *= 2
    extent = float(np.float32(2) * np.float32(radius))
    if padded:
        nns = ops.fixed_radius_search(P, P, radius, ignore_query_point=ignore_query_point, return_distances=True, row_stride=64)
        idx, rs, dist = nns.raw()
        row_count = nns.row_count
        assert int(nns.max_count.max()) <= 64
    else:
        nns = ops.fixed_radius_search(P, P, radius, ignore_query_point=ignore_query_point, return_distances=True)
        idx, rs, dist = nns.neighbors_index, nns.neighbors_row_splits, nns.neighbors_distance
        row_count = None
    nval = None
    if window == "explicit":
        nval = torch.from_numpy(np.random.default_rng(seed + 7).uniform(0.1, 1.0, size=idx.shape[0]).astype(np.float32)).to(dev)
    elif use_dist and window is not None:
        nval = dist
    impt = None if imp is None else torch.from_numpy(imp).to(dev)
    G = torch.from_numpy(np.random.default_rng(seed + 3).normal(size=(pos.shape[0], filt.shape[4])).astype(np.float32)).to(dev)
    kw = dict(neighbors_value=nval, window=window, inp_importance=impt, align_corners=align_corners,
              coordinate_mapping=mapping, interpolation=interpolation, normalize=normalize, symmetric=symmetric,
              sym_axis=sym_axis, neighbors_row_count=row_count, skip_self=skip_self)
    gw, gf = ops.cconv_backward(W, P, extent, P, F, idx, rs, G, **kw)
    torch.cuda.synchronize()
    pw = ref.PairWeights(pos, pos, idx.cpu().numpy(), rs.cpu().numpy(), extent, ks, window=window,
                         nval=None if nval is None else nval.cpu().numpy(), inp_importance=imp, align_corners=align_corners,
                         mapping=mapping, interpolation=interpolation, skip_self=skip_self,
                         row_count=None if row_count is None else row_count.cpu().numpy())
    rkw = dict(normalize=normalize, symmetric=symmetric, sym_axis=sym_axis)
    Gn = G.cpu().numpy()
    rw, rf, _ = ref.grads(pw, filt, feat, Gn, **rkw)
    aw, af, _ = ref.grads(pw, filt, feat, Gn, abs_mode=True, **rkw)
    return (gw.cpu().numpy(), gf.cpu().numpy()), (rw, rf), (aw, af)


def _compare(tag, got, want, bound):
    _check(tag + ":filters", got[0], want[0], bound[0])
    _check(tag + ":features", got[1], want[1], bound[1])


OPTIONS = [
    dict(),
    dict(use_dist=True),
    dict(window=None),
    dict(window="explicit"),
    dict(window="cubic"),
    dict(window="linear"),
    dict(window="peak"),
    dict(window="cubic_grad"),
    dict(normalize=True),
    dict(align_corners=False),
    dict(mapping="ball_to_cube_radial"),
    dict(mapping="identity"),
    dict(interpolation="linear_border"),
    dict(interpolation="nearest_neighbor"),
    dict(interpolation="linear_border", align_corners=False, mapping="ball_to_cube_radial", normalize=True),
    dict(imp=True),
    dict(imp=True, normalize=True, window="cubic"),
    dict(padded=True),
    dict(skip_self=True),
]


@pytest.mark.parametrize("opt", OPTIONS, ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()) or "default")
def test_options_against_float64(opt):
    opt = dict(opt)
    rng, pos = _scene(600, 1)
    cin, cout = 5, 7
    feat = rng.normal(size=(600, cin)).astype(np.float32)
    filt = rng.uniform(-1, 1, size=(4, 4, 4, cin, cout)).astype(np.float32)
    if opt.pop("imp", False):
        opt["imp"] = rng.uniform(0.2, 2.0, size=600).astype(np.float32)
    got, want, bound = _run(pos, feat, filt, 0.15, **opt)
    _compare("options", got, want, bound)


@pytest.mark.parametrize("shape,dims", [((4, 4, 4), 3), ((1, 8, 8), 2), ((1, 8, 1), 2), ((3, 3, 3), 3)])
@pytest.mark.parametrize("cin,cout", [(1, 1), (2, 3), (3, 24), (24, 64), (64, 16)])
def test_shapes_and_channels(shape, dims, cin, cout):
    rng, pos = _scene(400, 2, dims=dims)
    feat = rng.normal(size=(400, cin)).astype(np.float32)
    filt = rng.uniform(-1, 1, size=(*shape, cin, cout)).astype(np.float32)
    got, want, bound = _run(pos, feat, filt, 0.18)
    _compare("shapes", got, want, bound)


@pytest.mark.parametrize("sym_axis", [0, 1, 2])
@pytest.mark.parametrize("window", ["poly6", "peak"])
def test_ascc_half_kernels(sym_axis, window):
    rng, pos = _scene(500, 3)
    cin, cout = 4, 3
    feat = rng.normal(size=(500, cin)).astype(np.float32)
    sh = [6, 6, 6]
    sh[sym_axis] //= 2
    filt = rng.uniform(-1, 1, size=(*sh, cin, cout)).astype(np.float32)
    got, want, bound = _run(pos, feat, filt, 0.15, symmetric=True, sym_axis=sym_axis, window=window, ignore_query_point=True)
    _compare("ascc", got, want, bound)


@pytest.mark.parametrize("padded", [False, True])
def test_ascc_head_shares_the_trunk_list(padded):
    """SKIP_SELF on a list searched WITH the query points, as the ASCC head uses it, on a 2-D [1,8,8] kernel's half."""
    rng, pos = _scene(500, 4, dims=2)
    feat = rng.normal(size=(500, 3)).astype(np.float32)
    filt = rng.uniform(-1, 1, size=(1, 8, 4, 3, 2)).astype(np.float32)
    got, want, bound = _run(pos, feat, filt, 0.15, symmetric=True, sym_axis=2, skip_self=True, padded=padded)
    _compare("ascc_skip", got, want, bound)


def test_invert_matches_stable_argsort():
    from dmcf_amd import ops
    dev = _dev()
    rng = np.random.default_rng(5)
    n_out, n_inp = 300, 250
    counts = rng.integers(0, 9, size=n_out)
    counts[::17] = 0  # empty rows
    rs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    idx = rng.integers(0, n_inp - 20, size=rs[-1]).astype(np.int32)  # the last 20 inputs are never referenced
    attr = rng.normal(size=rs[-1]).astype(np.float32)
    inv = ops.invert_neighbors_list(n_inp, torch.from_numpy(idx).to(dev), torch.from_numpy(rs).to(dev),
                                    torch.from_numpy(attr).to(dev))
    order = np.argsort(idx, kind="stable")
    rows = np.repeat(np.arange(n_out), counts)
    assert np.array_equal(inv.pair_index.cpu().numpy(), order)
    assert np.array_equal(inv.neighbors_index.cpu().numpy(), rows[order])
    assert np.array_equal(inv.neighbors_attributes.cpu().numpy(), attr[order])
    want_rs = np.concatenate([[0], np.cumsum(np.bincount(idx, minlength=n_inp))])
    assert np.array_equal(inv.neighbors_row_splits.cpu().numpy(), want_rs)


def test_invert_padded_and_capacity():
    from dmcf_amd import ops
    dev = _dev()
    rng = np.random.default_rng(6)
    n_out, n_inp, stride = 50, 40, 6
    counts = rng.integers(0, stride + 1, size=n_out).astype(np.int32)
    begin = (np.arange(n_out + 1) * stride).astype(np.int64)
    idx = np.full(n_out * stride, 12345, dtype=np.int32)  # padding slots hold garbage
    for i in range(n_out):
        idx[i * stride:i * stride + counts[i]] = rng.integers(0, n_inp, size=counts[i])
    cap = (n_out - 3) * stride  # the last three rows reach past the buffer: empty
    inv = ops.invert_neighbors_list(n_inp, torch.from_numpy(idx[:cap].copy()).to(dev), torch.from_numpy(begin).to(dev), None,
                                    neighbors_row_count=torch.from_numpy(counts).to(dev))
    p = np.array([i * stride + k for i in range(n_out - 3) for k in range(counts[i])], dtype=np.int64)
    r = np.array([i for i in range(n_out - 3) for k in range(counts[i])], dtype=np.int64)
    order = np.argsort(idx[p], kind="stable")
    m = len(p)
    assert int(inv.neighbors_row_splits[-1]) == m
    assert np.array_equal(inv.pair_index.cpu().numpy()[:m], p[order])
    assert np.array_equal(inv.neighbors_index.cpu().numpy()[:m], r[order])
    assert np.all(inv.neighbors_index.cpu().numpy()[m:] == -1)
    want_rs = np.concatenate([[0], np.cumsum(np.bincount(idx[p], minlength=n_inp))])
    assert np.array_equal(inv.neighbors_row_splits.cpu().numpy(), want_rs)


def test_empty_sets_and_rows():
    from dmcf_amd import ops
    dev = _dev()
    W = torch.ones(4, 4, 4, 2, 3, device=dev)
    P = torch.rand(10, 3, device=dev)
    F = torch.rand(10, 2, device=dev)
    rs = torch.zeros(11, dtype=torch.int64, device=dev)
    idx = torch.zeros(0, dtype=torch.int32, device=dev)
    G = torch.rand(10, 3, device=dev)
    gw, gf = ops.cconv_backward(W, P, 0.2, P, F, idx, rs, G, window="poly6")
    assert torch.count_nonzero(gw) == 0 and torch.count_nonzero(gf) == 0
    gw, gf = ops.cconv_backward(W, P[:0], 0.2, P, F, idx, rs[:1], G[:0], window="poly6")
    assert torch.count_nonzero(gw) == 0 and torch.count_nonzero(gf) == 0


def test_bitwise_reproducible_and_accumulate():
    from dmcf_amd import ops
    rng, pos = _scene(20000, 8, scale=1.5)
    dev = _dev()
    P = torch.from_numpy(pos).to(dev)
    F = torch.randn(20000, 24, device=dev)
    W = torch.randn(4, 4, 4, 24, 16, device=dev)
    G = torch.randn(20000, 16, device=dev)
    nns = ops.fixed_radius_search(P, P, 0.1, return_distances=False)
    args = (W, P, 0.2, P, F, nns.neighbors_index, nns.neighbors_row_splits, G)
    a = ops.cconv_backward(*args, window="poly6")
    b = ops.cconv_backward(*args, window="poly6")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    c = ops.cconv_backward(*args, window="poly6", grad_filters=a[0].clone(), grad_inp_features=a[1].clone(), accumulate=True)
    assert torch.equal(c[0], 2 * a[0]) and torch.equal(c[1], 2 * a[1])


def test_adjoint_identity_200k():
    """<G, conv(f)> == <dF, f> and <G, conv_W(f)> == <dW, W> on a 200k-particle box at the model's radius."""
    from dmcf_amd import ops
    dev = _dev()
    n = 200_000
    rng = np.random.default_rng(9)
    spacing = 0.025  # Liquid3d: particle radius 0.025, first layer radius 4.5 x that
    side = spacing * n ** (1 / 3)
    P = torch.from_numpy(rng.uniform(0, side, size=(n, 3)).astype(np.float32)).to(dev)
    radius = 0.1125
    gen = torch.Generator(device=dev).manual_seed(9)
    for cin, cout, sym in ((24, 24, False), (8, 3, True)):
        F = torch.randn(n, cin, device=dev, generator=gen)
        W = torch.randn(4, 4, 2 if sym else 4, cin, cout, device=dev, generator=gen)
        G = torch.randn(n, cout, device=dev, generator=gen)
        nns = ops.fixed_radius_search(P, P, radius, ignore_query_point=sym, return_distances=False)
        kw = dict(window="poly6", symmetric=sym, sym_axis=2)
        out = ops.cconv_forward(W, P, 2 * radius, P, F, nns.neighbors_index, nns.neighbors_row_splits, **kw)
        gw, gf = ops.cconv_backward(W, P, 2 * radius, P, F, nns.neighbors_index, nns.neighbors_row_splits, G, **kw)
        # (relative to the sum of the absolute terms: the signed sums cancel to a small fraction of it)
        lhs = float((G.double() * out.double()).sum())
        scale = float((G.double() * out.double()).abs().sum())
        assert abs(lhs - float((gf.double() * F.double()).sum())) <= 1e-5 * scale
        assert abs(lhs - float((gw.double() * W.double()).sum())) <= 1e-5 * scale


def test_autograd_through_ops_and_inference_unchanged():
    from dmcf_amd import ops
    rng, pos = _scene(3000, 10)
    dev = _dev()
    P = torch.from_numpy(pos).to(dev)
    F = torch.randn(3000, 8, device=dev)
    W = torch.randn(4, 4, 4, 8, 16, device=dev)
    b = torch.randn(16, device=dev)
    nns = ops.fixed_radius_search(P, P, 0.1, return_distances=False)
    args = (P, 0.2, P)
    lists = (nns.neighbors_index, nns.neighbors_row_splits)
    plain = ops.cconv_forward(W, *args, F, *lists, window="poly6", bias=b)
    assert plain.grad_fn is None
    name = ops.cconv_forward(W, *args, F, *lists, window="poly6", name_only=True)
    Wg, Fg, bg = W.clone().requires_grad_(True), F.clone().requires_grad_(True), b.clone().requires_grad_(True)
    out = ops.cconv_forward(Wg, *args, Fg, *lists, window="poly6", bias=bg)
    assert out.grad_fn is not None
    assert torch.equal(out.detach(), plain)
    with torch.no_grad():
        again = ops.cconv_forward(Wg, *args, Fg, *lists, window="poly6", bias=bg)
    assert again.grad_fn is None and torch.equal(again, plain)
    assert ops.cconv_forward(Wg, *args, Fg, *lists, window="poly6", name_only=True) == name
    G = torch.randn_like(out)
    out.backward(G)
    gw, gf = ops.cconv_backward(W, *args, F, *lists, G, window="poly6")
    assert torch.equal(Wg.grad, gw) and torch.equal(Fg.grad, gf)
    assert torch.allclose(bg.grad, G.sum(0))
    with pytest.raises(ValueError):
        ops.cconv_forward(Wg, *args, Fg, *lists, window="poly6", out=torch.empty_like(plain))
    with pytest.raises(NotImplementedError):
        ops.cconv_forward(Wg, P, torch.full((3000,), 0.2, device=dev), P, Fg, *lists, window="poly6")


def test_layer_packed_cache_sees_optimizer_updates():
    from dmcf_amd.utils.convolutions import ContinuousConv
    from dmcf_amd.utils.tools.losses import get_window_func
    dev = _dev()
    rng, pos = _scene(3000, 11)
    P = torch.from_numpy(pos).to(dev)
    F = torch.randn(3000, 8, device=dev)
    conv = ContinuousConv(16, [4, 4, 4], window_function=get_window_func("poly6"),
                          coordinate_mapping="ball_to_cube_volume_preserving", normalize=False, device=dev)
    with torch.no_grad():
        before = conv(F, P, P, 0.2)
    conv.requires_grad_(True)
    opt = torch.optim.SGD(conv.parameters(), lr=0.1)
    out = conv(F, P, P, 0.2)
    assert out.grad_fn is not None and torch.equal(out.detach(), before)
    out.square().sum().backward()
    assert conv.kernel.grad is not None and conv.bias.grad is not None
    opt.step()
    opt.zero_grad()
    with torch.no_grad():
        after = conv(F, P, P, 0.2)
        conv.invalidate_packed()
        fresh = conv(F, P, P, 0.2)
    assert not torch.equal(after, before)
    assert torch.equal(after, fresh)
    with pytest.raises(NotImplementedError):
        conv(F, P, P, torch.full((3000,), 0.2, device=dev))


def test_report_worst_ratio():
    """Prints the worst err / bar of the comparisons above (run with -s)."""
    print("K_BAR", K_BAR, "worst err/bar", {k: round(v, 4) for k, v in WORST.items()})
