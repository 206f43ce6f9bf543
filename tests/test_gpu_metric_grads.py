"""Gradients of the point-cloud ops on the GPU (dmcf_amd/csrc/metrics_bwd.hip, ABI 2.13) against the float64 restatement
tests/metric_grads_ref.py, element-wise within 16 2^-24 A (A: the same gradient summed over the absolute values of its terms):
nn_distance (3-D, 2-D, n != m, duplicated points, one distance output only), match_cost on the HIP approx_match match, the
match-free EMD gradient (padded items, bits of an item alone), emd's recording forward (same bits, only when a gradient is
wanted), gather_point with repeated indices, determinism, and chamfer_loss / emd_loss end to end."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import metric_grads_ref as G  # noqa: E402
import metrics_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
WORST = {}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but torch.cuda.is_available() is False")
    yield torch.device("cuda:0")
    print("\nworst err/bar:", {k: float("%.3g" % v) for k, v in sorted(WORST.items())})


def _t(a, dev, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    return t.requires_grad_(grad)


def _close(got, ref, A, key, ulps=16):
    got = got.detach().double().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    bar = ulps * U * np.asarray(A) + 1e-30
    err = np.abs(got - ref)
    WORST[key] = max(WORST.get(key, 0.0), float((err / bar).max()))
    assert (err <= bar).all(), (key, float((err / bar).max()))


def _np(t):
    return t.detach().cpu().numpy()


# ----------------------------------------------------------------------------------------------------------------------
# 1. nn_distance
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["3d", "2d", "dup", "only1", "only2"])
def test_nn_distance_backward(dev, case):
    from dmcf_amd import ops
    rng = np.random.default_rng(10)
    b, n, m = 3, 700, 460
    dim = 2 if case == "2d" else 3
    x1, x2 = rng.uniform(size=(b, n, dim)), rng.uniform(size=(b, m, dim))
    if case == "dup":  # exact duplicates in both sets: ties go to the lowest index
        x1[:, 300:400] = x1[:, :100]
        x2[:, 200:260] = x2[:, :60]
        x2[:, 100:150] = x1[:, 500:550]
    g1, g2 = rng.normal(size=(b, n)), rng.normal(size=(b, m))
    a, c = _t(x1, dev, True), _t(x2, dev, True)
    d1, i1, d2, i2 = ops.nn_distance(a, c)
    assert d1.requires_grad and d2.requires_grad and not i1.requires_grad and not i2.requires_grad
    if case == "only1":
        (d1 * _t(g1, dev)).sum().backward()
        g2 = None
    elif case == "only2":
        (d2 * _t(g2, dev)).sum().backward()
        g1 = None
    else:
        ((d1 * _t(g1, dev)).sum() + (d2 * _t(g2, dev)).sum()).backward()
    f1, f2 = np.float64(np.float32(x1)), np.float64(np.float32(x2))
    gf1 = None if g1 is None else np.float64(np.float32(g1))
    gf2 = None if g2 is None else np.float64(np.float32(g2))
    r1, r2, A1, A2 = G.nn_distance_grad(f1, f2, gf1, gf2, _np(i1), _np(i2))
    _close(a.grad, r1[..., :dim], A1[..., :dim], "nn_" + case)
    _close(c.grad, r2[..., :dim], A2[..., :dim], "nn_" + case)
    if case == "dup":  # x1[300:400] copies x1[:100]: a tie between a point and its copy goes to the point
        gi2 = _np(i2)
        assert not ((gi2 >= 300) & (gi2 < 400)).any()
        assert np.array_equal(_np(i1)[:, 500:550], np.broadcast_to(np.arange(100, 150), (b, 50)))


# ----------------------------------------------------------------------------------------------------------------------
# 2. / 3. match_cost on the HIP match, and the match-free EMD gradient
# ----------------------------------------------------------------------------------------------------------------------
def _sets(rng, b, n, m, dim=3):
    x1, x2 = rng.uniform(size=(b, n, 3)), rng.uniform(size=(b, m, 3)) * 0.8 + 0.1
    if dim == 2:
        x1[..., 2] = 0.0
        x2[..., 2] = 0.0
    return np.float32(x1), np.float32(x2)


@pytest.mark.parametrize("dim", [3, 2])
def test_match_cost_and_emd_backward(dev, dim):
    from dmcf_amd import ops
    rng = np.random.default_rng(20 + dim)
    b, n, m = 2, 1000, 700
    x1, x2 = _sets(rng, b, n, m, dim)
    g = np.float32([0.75, -1.25])
    match = ops.approx_match(_t(x1, dev), _t(x2, dev))
    ref1, ref2, A1, A2 = G.match_cost_grad(x1, x2, _np(match).astype(np.float64), g)
    a, c = _t(x1, dev, True), _t(x2, dev, True)
    (ops.match_cost(a, c, match) * _t(g, dev)).sum().backward()
    _close(a.grad, ref1, A1, f"match_cost_{dim}d")
    _close(c.grad, ref2, A2, f"match_cost_{dim}d")
    a2, c2 = _t(x1, dev, True), _t(x2, dev, True)
    cost = ops.emd(a2, c2)
    (cost * _t(g, dev)).sum().backward()
    _close(a2.grad, ref1, A1, f"emd_{dim}d")
    _close(c2.grad, ref2, A2, f"emd_{dim}d")
    # the match-free gradient against the dense one on the device: the same bar
    _close(a2.grad, _np(a.grad).astype(np.float64), A1, f"emd_vs_dense_{dim}d")
    _close(c2.grad, _np(c.grad).astype(np.float64), A2, f"emd_vs_dense_{dim}d")


def test_emd_backward_padded_items(dev):
    from dmcf_amd import ops
    rng = np.random.default_rng(30)
    b, n, m = 3, 900, 640
    x1, x2 = _sets(rng, b, n, m)
    cn, cm = [900, 500, 0], [640, 333, 200]
    g = np.float32([1.0, 2.0, 3.0])
    a, c = _t(x1, dev, True), _t(x2, dev, True)
    (ops.emd(a, c, cn, cm) * _t(g, dev)).sum().backward()
    ga, gc = _np(a.grad), _np(c.grad)
    assert (ga[1, 500:] == 0).all() and (gc[1, 333:] == 0).all()
    assert (ga[2] == 0).all() and (gc[2] == 0).all()  # an item with an empty set
    match = ops.approx_match(_t(x1, dev), _t(x2, dev), cn, cm)
    r1, r2, A1, A2 = G.match_cost_grad(x1, x2, _np(match).astype(np.float64), g)
    _close(ga, r1, A1, "emd_padded")
    _close(gc, r2, A2, "emd_padded")
    # item 1 alone: the same bits
    a1, c1 = _t(x1[1:2, :500], dev, True), _t(x2[1:2, :333], dev, True)
    (ops.emd(a1, c1) * _t(g[1:2], dev)).sum().backward()
    assert torch.equal(a1.grad[0], a.grad[1, :500]) and torch.equal(c1.grad[0], c.grad[1, :333])


def _rows_ref(xr, xc, w_rc, g):
    """float64 on the device: rows' gradients g sum_c w[r, c] (x_r - x_c) / max(|d|, 1e-10) and their A."""
    diff = xr[:, None, :] - xc[None, :, :]
    t = g * (w_rc / torch.sqrt(torch.clamp((diff ** 2).sum(-1), min=1e-20)))[:, :, None] * diff
    return t.sum(1), t.abs().sum(1)


def test_emd_and_dense_backward_multi_tile_chunks(dev):
    """b = 1, n = m = 13 000: mt_plan gives 51 row blocks x 41 splits of 2 tiles (chunk 512), so every workgroup walks two LDS
    tiles.  The match-free and the dense gradients against float64 on 300 sampled rows of each set.  A row here sums 13 000
    terms, 13 times as many as in the cases above, and the rounding of float32 sums in sequence grows like the square root of
    their number: the bar is 64 2^-24 A (16 sqrt(13) = 58, rounded up)."""
    from dmcf_amd import ops
    rng = np.random.default_rng(90)
    n = 13000
    x1, x2 = _sets(rng, 1, n, n)
    g = np.float32([1.5])
    match = ops.approx_match(_t(x1, dev), _t(x2, dev))
    a, c = _t(x1, dev, True), _t(x2, dev, True)
    (ops.match_cost(a, c, match) * _t(g, dev)).sum().backward()
    a2, c2 = _t(x1, dev, True), _t(x2, dev, True)
    (ops.emd(a2, c2) * _t(g, dev)).sum().backward()
    X1, X2, M = _t(x1[0], dev).double(), _t(x2[0], dev).double(), match[0].double()
    r1 = torch.from_numpy(rng.choice(n, 300, replace=False)).to(dev)
    r2 = torch.from_numpy(rng.choice(n, 300, replace=False)).to(dev)
    ref1, A1 = _rows_ref(X1[r1], X2, M[:, r1].T, float(g[0]))
    ref2, A2 = _rows_ref(X2[r2], X1, M[r2, :], float(g[0]))
    for got1, got2, key in ((a.grad, c.grad, "dense_multi_tile"), (a2.grad, c2.grad, "emd_multi_tile")):
        _close(got1[0][r1], _np(ref1), _np(A1), key, ulps=64)
        _close(got2[0][r2], _np(ref2), _np(A2), key, ulps=64)


def test_nn_distance_backward_collapsed_cloud(dev):
    """A distant cloud: every point of xyz2 has the same nearest point in xyz1 and vice versa, so one point gathers thousands of
    sources (the workgroup path of the inversion) while the others take the one-thread path."""
    from dmcf_amd import ops
    rng = np.random.default_rng(95)
    b, n, m = 2, 3000, 5000
    x1 = rng.uniform(size=(b, n, 3))
    x2 = rng.uniform(size=(b, m, 3)) * 0.1 + 10.0
    x2[1, :100] = x1[1, :100] + 1e-3  # item 1: 100 points near their own partner, the rest far away
    g1, g2 = rng.normal(size=(b, n)), rng.normal(size=(b, m))
    a, c = _t(x1, dev, True), _t(x2, dev, True)
    d1, i1, d2, i2 = ops.nn_distance(a, c)
    ((d1 * _t(g1, dev)).sum() + (d2 * _t(g2, dev)).sum()).backward()
    assert np.bincount(_np(i2)[0]).max() > 256 and np.bincount(_np(i1)[0]).max() > 256  # (kInvShort in metrics_bwd.hip)
    r1, r2, A1, A2 = G.nn_distance_grad(np.float64(np.float32(x1)), np.float64(np.float32(x2)), np.float64(np.float32(g1)),
                                        np.float64(np.float32(g2)), _np(i1), _np(i2))
    _close(a.grad, r1, A1, "nn_collapsed")
    _close(c.grad, r2, A2, "nn_collapsed")


def test_backward_helpers_validate_operands(dev):
    """Shapes, dtypes and devices of the public backward helpers are checked before anything is launched."""
    from dmcf_amd import _lib, ops
    x1, x2 = torch.zeros(2, 5, 3, device=dev), torch.zeros(2, 4, 3, device=dev)
    lv, gc = torch.zeros(2, 10, 9, device=dev), torch.ones(2, device=dev)
    with pytest.raises(ValueError):
        ops.emd_with_levels(x1[0], x2[0])  # [n, 3]: not a batch
    with pytest.raises(ValueError):
        ops.emd_backward(x1, x2, lv[:, :, :8], gc)
    with pytest.raises(_lib.DmcfError):
        ops.emd_backward(x1, x2, lv, gc.cpu())
    with pytest.raises(ValueError):
        ops.match_cost_backward(x1, x2, torch.zeros(2, 5, 4, device=dev), gc)
    i1, i2 = torch.zeros(2, 5, dtype=torch.int32, device=dev), torch.zeros(2, 4, dtype=torch.int32, device=dev)
    with pytest.raises(TypeError):
        ops.nn_distance_backward(x1, x2, i1.long(), i2, torch.ones(2, 5, device=dev), None)
    with pytest.raises(ValueError):
        ops.nn_distance_backward(x1, x2, i1, i2[:, :3], None, torch.ones(2, 4, device=dev))
    with pytest.raises(ValueError):
        ops.gather_point_backward(torch.ones(4, 3, device=dev), torch.zeros(5, dtype=torch.int32, device=dev), 10)
    with pytest.raises(_lib.DmcfError):
        ops.gather_point_backward(torch.ones(4, 3, device=dev), torch.zeros(4, dtype=torch.int32), 10)


# ----------------------------------------------------------------------------------------------------------------------
# 4. the recording forward: same bits, and only when a gradient is wanted
# ----------------------------------------------------------------------------------------------------------------------
class _Counting:
    def __init__(self, real):
        self.real, self.calls = real, {}

    def __getattr__(self, name):
        if name.startswith("dmcf_emd"):
            self.calls[name] = self.calls.get(name, 0) + 1
        return getattr(self.real, name)


def test_emd_recording_forward(dev, monkeypatch):
    from dmcf_amd import _lib, ops
    rng = np.random.default_rng(40)
    x1, x2 = _sets(rng, 2, 800, 600)
    counts = ([800, 555], [600, 321])
    spy = _Counting(_lib.lib())
    monkeypatch.setattr(_lib, "_lib", spy)
    with torch.no_grad():
        plain = ops.emd(_t(x1, dev, True), _t(x2, dev, True), *counts)
    assert spy.calls.get("dmcf_emd_with_levels", 0) == 0 and spy.calls.get("dmcf_emd", 0) == 1
    plain2 = ops.emd(_t(x1, dev), _t(x2, dev), *counts)  # grad mode on, nothing requires grad
    assert spy.calls.get("dmcf_emd_with_levels", 0) == 0 and spy.calls.get("dmcf_emd", 0) == 2
    rec = ops.emd(_t(x1, dev, True), _t(x2, dev), *counts)
    assert spy.calls.get("dmcf_emd_with_levels", 0) == 1 and spy.calls.get("dmcf_emd", 0) == 2
    assert rec.grad_fn is not None and plain.grad_fn is None
    assert torch.equal(rec.detach(), plain) and torch.equal(plain, plain2)
    # the recorded ratios: zeros past the counts
    _, levels = ops.emd_with_levels(_t(x1, dev), _t(x2, dev), *counts)
    lv = _np(levels)
    assert lv.shape == (2, ops.EMD_LEVELS, 1400)
    assert (lv[1, :, 555:800] == 0).all() and (lv[1, :, 800 + 321:] == 0).all() and (lv[0, :, :800] > 0).any()


# ----------------------------------------------------------------------------------------------------------------------
# 5. gather_point
# ----------------------------------------------------------------------------------------------------------------------
def test_gather_point_backward(dev):
    from dmcf_amd import ops
    rng = np.random.default_rng(50)
    n, k, ch = 5000, 20000, 3
    inp = _t(rng.normal(size=(1, n, ch)), dev, True)
    ii = rng.integers(0, 4000, size=k)
    ii[rng.choice(k, 6000, replace=False)] = 7  # one row gathered 6000 times (the workgroup path), rows >= 4000 untouched
    idx = torch.from_numpy(ii.reshape(1, k).astype(np.int32)).to(dev)
    go = rng.normal(size=(1, k, ch)).astype(np.float32)
    out = ops.gather_point(inp, idx)
    assert torch.equal(out.detach()[0], inp.detach()[0][idx[0].long()])
    (out * _t(go, dev)).sum().backward()
    ref, A = G.gather_point_grad(go[0].astype(np.float64), _np(idx)[0], n)
    _close(inp.grad[0], ref, A, "gather_point")
    assert (_np(inp.grad)[0, 4000:] == 0).all()
    tg = torch.zeros(n, ch, dtype=torch.float64, device=dev).index_add_(0, idx[0].long(), _t(go[0], dev).double())
    _close(inp.grad[0], _np(tg), A, "gather_point_index_add")


# ----------------------------------------------------------------------------------------------------------------------
# 6. determinism
# ----------------------------------------------------------------------------------------------------------------------
def test_backward_determinism(dev):
    from dmcf_amd import ops
    rng = np.random.default_rng(60)
    x1, x2 = _sets(rng, 2, 1500, 1100)
    x1[:, 700:800] = x1[:, :100]  # ties and many sources per target
    idx = torch.from_numpy(rng.integers(0, 50, size=(1, 3000)).astype(np.int32)).to(dev)
    go = _t(rng.normal(size=(1, 3000, 3)), dev)

    def grads():
        a, c = _t(x1, dev, True), _t(x2, dev, True)
        d1, _, d2, _ = ops.nn_distance(a, c)
        (d1.sum() + 2 * d2.sum() + ops.emd(a, c).sum()).backward()
        p = _t(x1[:1], dev, True)
        (ops.gather_point(p, idx) * go).sum().backward()
        return a.grad, c.grad, p.grad

    for u, v in zip(grads(), grads()):
        assert torch.equal(u, v)


# ----------------------------------------------------------------------------------------------------------------------
# 7. end to end through the reference-path modules
# ----------------------------------------------------------------------------------------------------------------------
def test_chamfer_and_emd_loss_end_to_end(dev):
    from dmcf_amd.utils.tools import losses
    from dmcf_amd.utils.tools.nn_distance import chamfer_loss
    rng = np.random.default_rng(70)
    t, p = _sets(rng, 2, 600, 450)
    a, c = _t(t, dev, True), _t(p, dev, True)
    chamfer_loss(a, c).sum().backward()
    rt, rp, At, Ap = G.chamfer_grad(t, p)
    _close(a.grad, rt, At, "chamfer_loss")
    _close(c.grad, rp, Ap, "chamfer_loss")
    a, c = _t(t, dev, True), _t(p, dev, True)
    losses.emd_loss(a, c).sum().backward()
    from dmcf_amd import ops
    match = ops.approx_match(_t(t, dev), _t(p, dev))
    g = np.float32([1.0 / 600] * 2)
    r1, r2, A1, A2 = G.match_cost_grad(t, p, _np(match).astype(np.float64), g)
    _close(a.grad, r1, A1 + 1e-7 * np.abs(r1), "emd_loss")
    _close(c.grad, r2, A2 + 1e-7 * np.abs(r2), "emd_loss")


@pytest.mark.parametrize("which", ["chamfer", "emd"])
def test_gradient_steps_reduce_distance(dev, which):
    from dmcf_amd.utils.tools import losses
    from dmcf_amd.utils.tools.nn_distance import chamfer_loss
    rng = np.random.default_rng(80)
    target = _t(rng.uniform(size=(1, 400, 3)), dev)
    x = _t(rng.uniform(size=(1, 400, 3)) * 0.5 + 0.5, dev, True)
    loss = (lambda: chamfer_loss(target, x).sum()) if which == "chamfer" else (lambda: losses.emd_loss(target, x).sum())
    lr = 100.0 if which == "chamfer" else 12.0  # steps of about half the offset (Chamfer) / 0.03 (EMD)
    first = float(loss().detach())
    for _ in range(10):
        x.grad = None
        v = loss()
        v.backward()
        with torch.no_grad():
            x -= lr * x.grad
    last = float(loss().detach())
    assert last < 0.9 * first, (first, last)
