"""GPU checks of the CConv / ASCC backward (dmcf_cconv_backward) on what training runs beyond tests/test_gpu_cconv_backward.py:
distinct output and input sets (particles <-> grid_pos lattice, unbalanced clouds), the filter gradient's slab cap and several
row chunks, GEMM / contraction tile edges and the LDS limit, and the gradients of one ContinuousConv layer in each branch of
its training path.

Gradients are compared element by element with the blocked float64 reference (cconv_backward_ref.grads_blocked):
    |gpu - ref| <= kbar * 2^-24 * A,    A = the same gradient formed from the absolute values of every term
with kbar = K_BAR unless the case's float32 chains are longer than K_BAR covers (_kbars).  Every case asserts that it takes
the path it is named for (cconv_backward_ref.bwd_plan)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import cconv_backward_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

K_BAR = 256
PER_TERM = 64  # roundings one term of a chain carries before it is summed (geometry, window, a_p / psi_i, the products)


def _dev():
    return torch.device("cuda:0")


def _kbars(pw, K, cin, cout, symmetric=False):
    """(kbar of the filter gradient, kbar of the feature gradient) from the chains of float32 sums the plan gives.  A float32 sum
    of n terms errs by at most (n - 1) 2^-24 of the sum of their absolute values, each term adding PER_TERM roundings of its own:
      filters:  B_i over the longest row (L_row pairs), the GEMM over the rows of a slab, the slabs, then the chunks
      features: T_j over the longest inverted row (L_inv pairs, + L_row for the ASCC centre term), then the contraction:
                ceil(K / P) * Cout cells x channels per part and the P = 64 / Cin parts (Cin <= 64), or K * Cout (Cin > 64)
    The bar is K_BAR where the chains are shorter than that covers."""
    pl = ref.bwd_plan(pw.n_out, K, cin, cout)
    l_row = int(np.bincount(pw.i, minlength=1).max()) if pw.i.size else 0
    l_inv = int(np.bincount(pw.j, minlength=1).max()) if pw.j.size else 0
    rps = max(c[2] for c in pl["chunks"]) if pl["chunks"] else 0
    chain_w = l_row + rps + pl["S"] + len(pl["chunks"])
    if cin <= 64:
        parts = 64 // cin
        contraction = -(-K // parts) * cout + parts
    else:
        contraction = K * cout
    chain_f = l_inv + (l_row if symmetric else 0) + contraction
    return max(K_BAR, chain_w + PER_TERM), max(K_BAR, chain_f + PER_TERM)


def _list(inp, out, radius, padded=False, cut=0, ignore_query_point=False):
    """(index, row splits / row begins, squared distances, row counts or None, rows cut); ``padded``: the single-pass padded list
    with the buffer cut so that at least the last ``cut`` rows, one of them not empty, reach past it."""
    from dmcf_amd import ops
    nns = ops.fixed_radius_search(inp, out, radius, ignore_query_point=ignore_query_point, return_distances=True)
    if not padded:
        return nns.neighbors_index, nns.neighbors_row_splits, nns.neighbors_distance, None, 0
    longest = int(torch.diff(nns.neighbors_row_splits).max())
    pn = ops.fixed_radius_search(inp, out, radius, ignore_query_point=ignore_query_point, return_distances=True,
                                 row_stride=longest + 3)
    idx, begin, dist = pn.raw()
    assert int(pn.max_count.max()) <= pn.stride
    cut = max(cut, out.shape[0] - int(np.flatnonzero(pn.row_count.cpu().numpy())[-1]))
    cap = (out.shape[0] - cut) * pn.stride
    return idx[:cap], begin, dist[:cap], pn.row_count, cut


def _grad_case(tag, out_pos, inp_pos, feat, filt, idx, rs, dist, count, extent, *, window="poly6", use_dist=False,
               normalize=False, symmetric=False, sym_axis=2, imp=None, skip_self=False, accumulate=False, seed=0):
    """ops.cconv_backward against the blocked float64 reference; returns (PairWeights, plan)."""
    from dmcf_amd import ops
    dev = _dev()
    n_out, n_inp = out_pos.shape[0], inp_pos.shape[0]
    cin, cout = filt.shape[3], filt.shape[4]
    full = list(filt.shape[:3])
    if symmetric:
        full[sym_axis] *= 2
    K = full[0] * full[1] * full[2]
    rng = np.random.default_rng(seed)
    nval = None
    if window == "explicit":
        nval = torch.from_numpy(rng.uniform(0.1, 1.0, size=idx.shape[0]).astype(np.float32)).to(dev)
    elif use_dist and window is not None:
        nval = dist
    G = rng.normal(size=(n_out, cout)).astype(np.float32)
    P_out, P_inp = torch.from_numpy(out_pos).to(dev), torch.from_numpy(inp_pos).to(dev)
    kw = dict(neighbors_value=nval, window=window, inp_importance=None if imp is None else torch.from_numpy(imp).to(dev),
              normalize=normalize, symmetric=symmetric, sym_axis=sym_axis, neighbors_row_count=count, skip_self=skip_self)
    init_w = init_f = None
    gw = gf = None
    if accumulate:
        init_w = rng.normal(size=filt.shape).astype(np.float32)
        init_f = rng.normal(size=(n_inp, cin)).astype(np.float32)
        gw, gf = torch.from_numpy(init_w).to(dev), torch.from_numpy(init_f).to(dev)
    gw, gf = ops.cconv_backward(torch.from_numpy(filt).to(dev), P_out, extent, P_inp, torch.from_numpy(feat).to(dev), idx, rs,
                                torch.from_numpy(G).to(dev), grad_filters=gw, grad_inp_features=gf, accumulate=accumulate, **kw)
    torch.cuda.synchronize()
    gw, gf = gw.cpu().numpy(), gf.cpu().numpy()
    pw = ref.PairWeights(out_pos, inp_pos, idx.cpu().numpy(), rs.cpu().numpy(), extent, full, window=window,
                         nval=None if nval is None else nval.cpu().numpy(), inp_importance=imp, skip_self=skip_self,
                         row_count=None if count is None else count.cpu().numpy())
    rkw = dict(normalize=normalize, symmetric=symmetric, sym_axis=sym_axis)
    rw, rf = ref.grads_blocked(pw, filt, feat, G, **rkw)
    aw, af = ref.grads_blocked(pw, filt, feat, G, abs_mode=True, **rkw)
    kbar_w, kbar_f = _kbars(pw, K, cin, cout, symmetric)
    if accumulate:
        # (the sum with the prior content rounds once more, on |prior| + A)
        rw, aw = rw + init_w, aw + np.abs(init_w)
        rf, af = rf + init_f, af + np.abs(init_f)
    ref.check(tag + ":filters", gw, rw, aw, kbar_w)
    ref.check(tag + ":features", gf, rf, af, kbar_f)
    unref = np.bincount(pw.j, minlength=n_inp) == 0
    if not accumulate:
        assert np.all(gf[unref] == 0), f"{tag}: an input no pair references has a non-zero gradient"
    return pw, ref.bwd_plan(n_out, K, cin, cout)


# ---- distinct sets ----------------------------------------------------------------------------------------------------------

LATTICE_CASES = [
    dict(direction="p2l", use_dist=True),
    dict(direction="l2p"),
    dict(direction="p2l", padded=True, window="explicit"),
    dict(direction="l2p", padded=True, window=None, normalize=True),
    dict(direction="p2l", normalize=True, imp=True),
    dict(direction="l2p", shape=(1, 8, 8), imp=True),
    dict(direction="p2l", shape=(1, 8, 1), padded=True, normalize=True),
    dict(direction="l2p", shape=(1, 8, 1), window="explicit"),
    dict(direction="p2l", shape=(1, 8, 8), window=None),
]


@pytest.mark.parametrize("case", LATTICE_CASES, ids=lambda c: ",".join(f"{k}={v}" for k, v in c.items()))
def test_particles_and_lattice(case):
    """particles -> grid_pos lattice and back at the model spacing (3-D: voxel 0.1, radius 0.4); the lattice padded by 4 cells,
    so that its outer points have no particle in reach (empty rows; inputs no pair references)."""
    from dmcf_amd import ops
    c = dict(case)
    rng = np.random.default_rng(len(LATTICE_CASES) + LATTICE_CASES.index(case))
    shape = c.get("shape", (4, 4, 4))
    two_d = shape[0] == 1
    part = rng.uniform(0, 1, size=(1000, 3)).astype(np.float32)
    if two_d:
        part[:, 2] = 0.0
    P = torch.from_numpy(part).to(_dev())
    # (2-D: a finer lattice, so that a particle too is in reach of more than 64 lattice points, padded by the most cells, 8)
    voxel = 0.05 if two_d else 0.1
    L = ops.grid_pos(P, np.float32([voxel, voxel, 0.0 if two_d else voxel]), pad=8 if two_d else 4)
    lat = L.cpu().numpy()
    out, inp = (lat, part) if c["direction"] == "p2l" else (part, lat)
    radius = 0.4
    idx, rs, dist, count, cut = _list(torch.from_numpy(inp).to(_dev()), torch.from_numpy(out).to(_dev()), radius,
                                      padded=c.get("padded", False), cut=5)
    cin, cout = 4, 6
    feat = rng.normal(size=(inp.shape[0], cin)).astype(np.float32)
    filt = rng.uniform(-1, 1, size=(*shape, cin, cout)).astype(np.float32)
    imp = rng.uniform(0.2, 2.0, size=inp.shape[0]).astype(np.float32) if c.get("imp") else None
    pw, pl = _grad_case("lattice", out, inp, feat, filt, idx, rs, dist, count, float(np.float32(2) * np.float32(radius)),
                        window=c.get("window", "poly6"), use_dist=c.get("use_dist", False), normalize=c.get("normalize", False),
                        imp=imp, seed=7)
    assert out.shape[0] != inp.shape[0]
    assert np.bincount(pw.j, minlength=inp.shape[0]).max() > 64, "no inverted row longer than 64 pairs"
    if c["direction"] == "p2l":
        assert np.any(np.bincount(pw.i, minlength=out.shape[0]) == 0), "no empty output row"
    else:
        assert np.any(np.bincount(pw.j, minlength=inp.shape[0]) == 0), "no input without a pair"
    if c.get("padded"):
        assert int(count[-cut:].sum()) > 0 and pw.i.max() < out.shape[0] - cut, "no row cut off by the capacity"


@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("n_out,n_inp", [(6000, 300), (300, 6000)])
def test_unbalanced_clouds(n_out, n_inp, padded):
    """Random clouds, one 20x the other, offset so that part of each is out of reach of the other."""
    rng = np.random.default_rng(n_out + 3 * padded)
    inp = rng.uniform(0, 1, size=(n_inp, 3)).astype(np.float32)
    out = rng.uniform(0.4, 1.4, size=(n_out, 3)).astype(np.float32)
    radius = 0.15 if n_inp > n_out else 0.25
    dev = _dev()
    idx, rs, dist, count, cut = _list(torch.from_numpy(inp).to(dev), torch.from_numpy(out).to(dev), radius, padded=padded, cut=7)
    cin, cout = 5, 3
    feat = rng.normal(size=(n_inp, cin)).astype(np.float32)
    filt = rng.uniform(-1, 1, size=(4, 4, 4, cin, cout)).astype(np.float32)
    pw, _ = _grad_case("clouds", out, inp, feat, filt, idx, rs, dist, count, float(np.float32(2) * np.float32(radius)),
                       normalize=True, use_dist=True, seed=11)
    assert np.any(np.bincount(pw.i, minlength=n_out) == 0), "no empty output row"
    assert np.any(np.bincount(pw.j, minlength=n_inp) == 0), "no input without a pair"
    assert np.bincount(pw.j if n_out > n_inp else pw.i).max() > 64, "no row longer than 64 pairs"
    if padded:
        assert int(count[-cut:].sum()) > 0 and pw.i.max() < n_out - cut, "no row cut off by the capacity"


# ---- the filter gradient's plan: slab cap, several chunks ------------------------------------------------------------------

def _same_set(n, radius, shape, cin, cout, seed, symmetric=False, sym_axis=2, **kw):
    rng = np.random.default_rng(seed)
    pos = rng.uniform(0, 1, size=(n, 3)).astype(np.float32)
    P = torch.from_numpy(pos).to(_dev())
    idx, rs, dist, count, _ = _list(P, P, radius, ignore_query_point=symmetric)
    feat = rng.normal(size=(n, cin)).astype(np.float32)
    filt = rng.uniform(-1, 1, size=(*shape, cin, cout)).astype(np.float32)
    return _grad_case(kw.pop("tag"), pos, pos, feat, filt, idx, rs, dist, count, float(np.float32(2) * np.float32(radius)),
                      symmetric=symmetric, sym_axis=sym_axis, seed=seed + 1, **kw)


def test_slab_cap():
    """One chunk of more than 256 x 256 rows with a small M: S = 256 slabs of more than 256 rows each."""
    _, pl = _same_set(70000, 0.033, (4, 4, 4), 3, 5, 21, tag="slab_cap")
    assert len(pl["chunks"]) == 1 and pl["S"] == ref.BWD_MAX_SLABS and pl["rows_per_slab"] > ref.BWD_SLAB_ROWS


@pytest.mark.parametrize("accumulate", [False, True])
def test_chunks_ascc_6x6x6(accumulate):
    """The shipped multi-chunk layer: same-set ASCC, 6x6x6 full kernel, Cin 32 (R = 2^28 / 6912 = 38836 rows): 45000 points
    take two chunks, the last one partial; with normalize, and accumulating into non-zero gradients."""
    _, pl = _same_set(45000, 0.054, (6, 6, 3), 32, 16, 31, symmetric=True, sym_axis=2, normalize=True, accumulate=accumulate,
                      tag="chunks")
    assert pl["R"] == 38836 and len(pl["chunks"]) == 2 and pl["chunks"][-1][1] < pl["R"]


@pytest.mark.parametrize("accumulate", [False, True])
def test_chunks_wide_input(accumulate):
    """4x4x4, Cin 256 (K * Cin = 16384, the LDS limit), Cout 4: R = 16384 rows, 40000 points in three chunks."""
    _, pl = _same_set(40000, 0.05, (4, 4, 4), 256, 4, 41, normalize=True, accumulate=accumulate, use_dist=True, tag="chunks")
    assert pl["R"] == 16384 and len(pl["chunks"]) == 3 and pl["chunks"][-1][1] < pl["R"]


# ---- tile edges and the LDS limit --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,cin,cout", [
    ((3, 3, 3), 7, 65), ((2, 3, 3), 5, 96), ((3, 3, 3), 3, 130),     # GEMM grid 2 / 2 / 3 tiles wide in y
    ((3, 3, 3), 65, 4), ((5, 5, 5), 96, 5), ((2, 2, 2), 128, 66),    # cconv_bwd_input's Cin > 64 branch
    ((4, 4, 4), 256, 3), ((4, 4, 4), 3, 256),                        # K * Cin, K * Cout = 16384: the largest accepted
])
def test_tile_edges(shape, cin, cout):
    K = shape[0] * shape[1] * shape[2]
    assert ref.bwd_supported(K, cin, cout)
    assert cout > 64 or cin > 64
    _same_set(500, 0.15, shape, cin, cout, 51 + cin + cout, normalize=True, tag="tiles")


@pytest.mark.parametrize("cin,cout", [(257, 3), (3, 257)])
def test_one_past_the_lds_limit(cin, cout):
    """K * Cin or K * Cout = 16384 + K: DmcfError (DMCF_EUNSUPPORTED), the output tensors untouched."""
    from dmcf_amd import _lib, ops
    assert not ref.bwd_supported(64, cin, cout)
    dev = _dev()
    P = torch.rand(200, 3, device=dev)
    nns = ops.fixed_radius_search(P, P, 0.2, return_distances=False)
    W = torch.randn(4, 4, 4, cin, cout, device=dev)
    gw = torch.full_like(W, 3.5)
    gf = torch.full((200, cin), -1.25, device=dev)
    with pytest.raises(_lib.DmcfError):
        ops.cconv_backward(W, P, 0.4, P, torch.randn(200, cin, device=dev), nns.neighbors_index, nns.neighbors_row_splits,
                           torch.randn(200, cout, device=dev), window="poly6", grad_filters=gw, grad_inp_features=gf)
    torch.cuda.synchronize()
    assert bool((gw == 3.5).all()) and bool((gf == -1.25).all())


# ---- one ContinuousConv layer in each branch of its training path -----------------------------------------------------------

def _layer(**kw):
    from dmcf_amd.utils.convolutions import ContinuousConv
    from dmcf_amd.utils.tools.losses import get_window_func
    args = dict(filters=6, kernel_size=[4, 4, 4], window_function=get_window_func("poly6"),
                coordinate_mapping="ball_to_cube_volume_preserving", normalize=True, device=_dev())
    args.update(kw)
    return ContinuousConv(**args)


def _recorder(target, calls):
    """ops.cconv_forward through ``target``, keeping each recorded call's arguments and the gradient that reaches its output."""
    def rec(*a, **k):
        res = target(*a, **k)
        if isinstance(res, torch.Tensor) and res.requires_grad:
            entry = dict(args=a, kw=k)
            res.register_hook(lambda g: entry.__setitem__("grad", g.detach().clone()))
            calls.append(entry)
        return res
    return rec


def _abs_terms(entry):
    """The recorded call's (A of its filter gradient, A of its feature gradient, A of its output) in float64."""
    a, k = entry["args"], entry["kw"]
    filters, out_pos, extent, inp_pos, feats, idx, rs = a[:7]
    sym, axis = k.get("symmetric", False), k.get("sym_axis", 2)
    dims = list(filters.shape[:3])
    if sym:
        dims[axis] *= 2
    cpu = lambda t: None if t is None else t.detach().cpu().numpy()  # noqa: E731
    pw = ref.PairWeights(cpu(out_pos), cpu(inp_pos), cpu(idx), cpu(rs), extent, dims, window=k.get("window"),
                         window_fac=k.get("window_fac", 1.0), nval=cpu(k.get("neighbors_value")),
                         inp_importance=cpu(k.get("inp_importance")), align_corners=k.get("align_corners", True),
                         mapping=k.get("coordinate_mapping"), interpolation=k.get("interpolation", "linear"),
                         skip_self=k.get("skip_self", False), row_count=cpu(k.get("neighbors_row_count")))
    rkw = dict(normalize=k.get("normalize", False), symmetric=sym, sym_axis=axis)
    aw, af = ref.grads_blocked(pw, cpu(filters), cpu(feats), cpu(entry["grad"]), abs_mode=True, **rkw)
    ay = ref.conv(pw, torch.from_numpy(np.abs(cpu(filters))).double(), torch.from_numpy(np.abs(cpu(feats))).double(),
                  abs_mode=True, **rkw)
    return aw, af, ay.numpy()


def _layer_grads(layer, x, call, G, calls):
    xg = x.clone().requires_grad_(True)
    for p in layer.parameters():
        p.grad = None
    y = call(layer, xg)
    (y * G).sum().backward()
    g = {n: p.grad.detach().cpu().numpy() for n, p in layer.named_parameters() if p.grad is not None}
    g["x"] = xg.grad.detach().cpu().numpy()
    return y.detach(), g


def _layer_case(tag, layer, x, call, monkeypatch, acc=None, extra_bias=None):
    """Gradients of kernel, bias, dense and the input features of ``call(layer, x)`` on the HIP path against the same layer whose
    ops.cconv_forward is the float64 shim; the training forward against the inference forward.  Bars from the absolute terms of
    the layer's one CConv call (recorded with the gradient reaching it)."""
    from dmcf_amd import ops
    with torch.no_grad():
        call(layer, x)  # (builds the weights)
        gen = torch.Generator(device=x.device).manual_seed(5)
        for p in layer.parameters():
            p.copy_(torch.rand(p.shape, device=x.device, generator=gen) * 2 - 1)
    layer.requires_grad_(False)
    with torch.no_grad():
        if acc is not None:
            layer.accumulate_into, layer.extra_bias = acc.clone(), extra_bias
        y_inf = call(layer, x).clone()
    layer.requires_grad_(True)
    real = ops.cconv_forward
    calls = []
    monkeypatch.setattr(ops, "cconv_forward", _recorder(real, calls))
    G = torch.randn(y_inf.shape, device=x.device, generator=torch.Generator(device=x.device).manual_seed(6))
    acc_before = None if acc is None else acc.clone()
    if acc is not None:
        layer.accumulate_into, layer.extra_bias = acc, extra_bias
    y, got = _layer_grads(layer, x, call, G, calls)
    assert len(calls) == 1 and "grad" in calls[0], "the layer's CConv was not recorded by autograd"
    entry = calls[0]
    if acc is not None:
        assert torch.equal(acc, acc_before), "accumulate_into was written"
        y_plain = call(layer, x)  # (the same kernels: bitwise the same conv output)
        assert torch.equal(y, (acc + y_plain.detach()) + extra_bias)
    monkeypatch.setattr(ops, "cconv_forward", _recorder(ref.float64_cconv(real), []))
    if acc is not None:
        layer.accumulate_into, layer.extra_bias = acc, extra_bias
    y_ref, want = _layer_grads(layer, x, call, G, [])
    monkeypatch.setattr(ops, "cconv_forward", real)
    assert set(got) == set(want)
    aw, af, ay = _abs_terms(entry)
    Gc = np.abs(entry["grad"].cpu().numpy().astype(np.float64))
    xa = np.abs(x.cpu().numpy().astype(np.float64))
    # the kernel's A: the recorded filter's, summed back through the circular expansion
    if layer.circular:
        with torch.enable_grad():
            exp = layer._expanded_kernel()
            a_kernel = torch.autograd.grad(exp, layer.kernel, torch.from_numpy(aw).to(exp))[0].double().cpu().numpy()
    else:
        a_kernel = aw
    a_x = af.copy()
    ya = ay.copy()
    if layer.dense is not None:
        dense = np.abs(layer.dense.detach().cpu().numpy().astype(np.float64))
        a_x += Gc @ dense.T
        ya += xa @ dense
        ref.check(tag + ":dense", got["dense"], want["dense"], xa.T @ Gc, K_BAR)
    if layer.bias is not None:
        ref.check(tag + ":bias", got["bias"], want["bias"], Gc.sum(0), K_BAR)
        ya += np.abs(layer.bias.detach().cpu().numpy())
    if acc is not None:
        ya += np.abs(acc.cpu().numpy()) + np.abs(extra_bias.cpu().numpy())
    ref.check(tag + ":kernel", got["kernel"], want["kernel"], a_kernel, K_BAR)
    ref.check(tag + ":x", got["x"], want["x"], a_x, K_BAR)
    # (relu, tanh: 1-Lipschitz, so the bar of the pre-activation sum carries over)
    ref.check(tag + ":forward", y.cpu().numpy(), y_inf.cpu().numpy().astype(np.float64), ya, K_BAR)
    ref.check(tag + ":forward", y.cpu().numpy(), y_ref.cpu().numpy().astype(np.float64), ya, K_BAR)
    return entry


def _cloud(n, seed, lo=0.0, hi=1.0):
    return torch.from_numpy(np.random.default_rng(seed).uniform(lo, hi, size=(n, 3)).astype(np.float32)).to(_dev())


EXTENT = 0.3


def test_layer_own_search_csr(monkeypatch):
    P = _cloud(1500, 61)
    x = torch.randn(1500, 5, device=_dev())
    e = _layer_case("layer", _layer(), x, lambda l, f: l(f, P, P, EXTENT), monkeypatch)
    assert e["kw"]["neighbors_row_count"] is None and e["kw"]["window"] == "poly6"


def test_layer_own_search_padded(monkeypatch):
    from dmcf_amd import ops
    P = _cloud(1500, 62)
    x = torch.randn(1500, 5, device=_dev())
    layer = _layer()
    frs = layer.fixed_radius_search
    layer.fixed_radius_search = lambda points, queries, radius, **kw: frs(points, queries, radius, row_stride=64, **kw)
    e = _layer_case("layer", layer, x, lambda l, f: l(f, P, P, EXTENT), monkeypatch)
    assert e["kw"]["neighbors_row_count"] is not None
    assert isinstance(layer.nns, ops.PaddedNeighborList) and int(layer.nns.max_count.max()) <= 64


def test_layer_callable_window(monkeypatch):
    """A window that is a plain callable: the padded list turned into CSR, its values as the explicit window."""
    P = _cloud(1500, 63)
    x = torch.randn(1500, 5, device=_dev())
    layer = _layer(window_function=lambda q: torch.clamp(1.0 - q, min=0.0) ** 3)
    frs = layer.fixed_radius_search
    layer.fixed_radius_search = lambda points, queries, radius, **kw: frs(points, queries, radius, row_stride=64, **kw)
    e = _layer_case("layer", layer, x, lambda l, f: l(f, P, P, EXTENT), monkeypatch)
    assert e["kw"]["window"] == "explicit" and e["kw"]["neighbors_row_count"] is None


def test_layer_user_neighbors_with_importance(monkeypatch):
    from dmcf_amd import ops
    P, Q = _cloud(1200, 64), _cloud(900, 65, 0.2, 1.2)
    nns = ops.fixed_radius_search(P, Q, 0.5 * EXTENT, return_distances=False)
    imp = torch.rand(nns.neighbors_index.shape[0], device=_dev()) + 0.1
    x = torch.randn(1200, 5, device=_dev())
    e = _layer_case("layer", _layer(), x, lambda l, f: l(f, P, Q, EXTENT, user_neighbors_index=nns.neighbors_index,
                                                         user_neighbors_row_splits=nns.neighbors_row_splits,
                                                         user_neighbors_importance=imp), monkeypatch)
    assert e["kw"]["window"] == "explicit"


def test_layer_inp_importance(monkeypatch):
    P = _cloud(1500, 66)
    x = torch.randn(1500, 5, device=_dev())
    s = torch.rand(1500, device=_dev()) * 2 + 0.1
    e = _layer_case("layer", _layer(), x, lambda l, f: l(f, P, P, EXTENT, inp_importance=s), monkeypatch)
    assert e["kw"]["inp_importance"] is not None


def test_layer_dense_center_and_activation(monkeypatch):
    P = _cloud(1500, 67)
    x = torch.randn(1500, 5, device=_dev())
    layer = _layer(use_dense_layer_for_center=True, activation="relu", normalize=False)
    _layer_case("layer", layer, x, lambda l, f: l(f, P, P, EXTENT), monkeypatch)
    assert layer.dense is not None and layer.dense.grad is not None


def test_layer_accumulate_into_and_extra_bias(monkeypatch):
    P = _cloud(1500, 68)
    x = torch.randn(1500, 5, device=_dev())
    acc = torch.randn(1500, 6, device=_dev())
    eb = torch.randn(6, device=_dev())
    _layer_case("layer", _layer(), x, lambda l, f: l(f, P, P, EXTENT), monkeypatch, acc=acc, extra_bias=eb)


def test_layer_ascc_ignoring_query_points(monkeypatch):
    P = _cloud(1500, 69)
    x = torch.randn(1500, 5, device=_dev())
    layer = _layer(symmetric=True, sym_axis=2, normalize=False, radius_search_ignore_query_points=True)
    e = _layer_case("layer", layer, x, lambda l, f: l(f, P, P, EXTENT), monkeypatch)
    assert e["kw"]["symmetric"] and tuple(layer.kernel.shape[:3]) == (4, 4, 2)


def test_layer_distinct_sets_hash_table(monkeypatch):
    from dmcf_amd import ops
    P, Q = _cloud(1400, 70), _cloud(700, 71, 0.3, 1.3)
    ht = ops.build_spatial_hash_table(P, float(np.float32(0.5) * np.float32(EXTENT)), n_queries=700)
    x = torch.randn(1400, 5, device=_dev())
    e = _layer_case("layer", _layer(), x, lambda l, f: l(f, P, Q, EXTENT, fixed_radius_search_hash_table=ht), monkeypatch)
    assert e["args"][1].shape[0] == 700 and e["args"][3].shape[0] == 1400


def test_layer_circular(monkeypatch):
    """A circular kernel that is not symmetric: the ring kernel expanded by torch, its gradient summed back over the rings."""
    P = _cloud(1500, 72)
    x = torch.randn(1500, 5, device=_dev())
    layer = _layer(circular=True)
    e = _layer_case("layer", layer, x, lambda l, f: l(f, P, P, EXTENT), monkeypatch)
    assert tuple(layer.kernel.shape) == (2, 5, 6) and tuple(e["args"][0].shape) == (4, 4, 4, 5, 6)
    with pytest.raises(NotImplementedError):
        _layer(circular=True, symmetric=True, normalize=False)(x.requires_grad_(True), P, P, EXTENT)


def test_report_worst_ratio():
    """Prints the worst err / bar of every group of both backward test files (run with -s)."""
    print("worst err/bar", {k: round(v, 4) for k, v in ref.WORST.items()})
