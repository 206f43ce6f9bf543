"""The window sum with row splits on the GPU (ABI 2.22: dmcf_frs_window_sum_batched, dmcf_frs_window_sum_backward_batched;
ops.window_sum(points_row_splits=, queries_row_splits=), losses.compute_density / density_loss with row splits).

Scene: the shared batch of tests/batched_scene.py plus an empty fourth item.  The points of item b are [fluid_b, slab], the
queries its fluid points; items 0 and 2 occupy the same coordinates, so a walk that left its slab of the cell table would
roughly double item 0's sums.  A 3-D variant draws the fluid's z in [0, 0.1].  Radius 0.1: 8 - 25 neighbours per query.

The forward is held to the float64 oracle per item under the bar of tests/test_gpu_ops.py (rtol 2e-5, atol 2e-5 max|ref|), the
gradient to tests/density_grad_ref.py per item under the bar of tests/test_gpu_density_grad.py (256 * 2^-24 * A).  The batched
and the un-batched sums are not expected to agree bit for bit (one grid geometry serves all items, so the scan meets the
candidates in another order); the counts are."""
import numpy as np
import pytest

import batched_scene as scene
import cconv_backward_ref as cref
import density_grad_ref as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

RADIUS = 0.1
K_BAR = 256


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but torch.cuda.is_available() is False")
    return torch.device("cuda:0")


def _t(a, dev, grad=False):
    return torch.from_numpy(np.array(a, dtype=np.float32)).to(dev).requires_grad_(grad)


def _scene(dim):
    """-> (points [n, 3], points row splits, queries [m, 3], queries row splits): four items, the last one empty."""
    rng = np.random.RandomState(5)
    fluid = [f.copy() for f in scene.fluid_items()]
    if dim == 3:
        z = rng.uniform(0.0, 0.1, size=fluid[2].shape[0]).astype(np.float32)
        fluid[0][:, 2], fluid[2][:, 2] = z[:fluid[0].shape[0]], z  # (items 0 and 2 stay coincident)
        fluid[1][:, 2] = 0.05
    slab = scene.slab()[0]
    empty = np.zeros((0, 3), dtype=np.float32)
    pts, prs = scene.concat([np.concatenate([f, slab]) for f in fluid] + [empty])
    qs, qrs = scene.concat(fluid + [empty])
    return pts, prs, qs, qrs


SCENES = {dim: _scene(dim) for dim in (2, 3)}


def _ref_sum(oracle, out, inp, win, ignore):
    """oracle.compute_density (float64 sums of the float32 window values) with the search's ignore_query_point."""
    if not ignore:
        return oracle.compute_density(out, inp, RADIUS, win)
    idx, rs, _ = oracle.fixed_radius_search(inp, out, RADIUS, ignore_query_point=True)
    seg = np.repeat(np.arange(out.shape[0]), np.diff(rs))
    q = (((inp[idx] - out[seg]) ** 2).sum(axis=-1) / np.float32(RADIUS) ** 2).astype(np.float32)
    w = q if win is None else oracle.window(win, q)
    return np.bincount(seg, weights=w.astype(np.float64), minlength=out.shape[0]).astype(np.float32)


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("ignore", [False, True], ids=["keep_self", "ignore_query_point"])
def test_forward_against_the_oracle_per_item(oracle, dev, dim, ignore):
    from dmcf_amd import ops
    pts, prs, qs, qrs = SCENES[dim]
    P, Q = _t(pts, dev), _t(qs, dev)
    table = ops.build_spatial_hash_table(P, RADIUS, n_queries=Q.shape[0], points_row_splits=prs)
    for window in ops.WINDOWS:
        out = ops.window_sum(P, Q, RADIUS, window, ignore_query_point=ignore, hash_table=table, points_row_splits=prs,
                             queries_row_splits=qrs)
        assert isinstance(out, torch.Tensor) and out.shape == (Q.shape[0],) and out.dtype == torch.float32
        got = out.cpu().numpy()
        for b in range(3):
            pb, qb = pts[prs[b]:prs[b + 1]], qs[qrs[b]:qrs[b + 1]]
            gb = got[qrs[b]:qrs[b + 1]]
            if window is None:  # the counts: exactly the un-batched call on the slices, and the oracle's rows
                one = ops.window_sum(_t(pb, dev), _t(qb, dev), RADIUS, None, ignore_query_point=ignore)
                assert torch.equal(out[qrs[b]:qrs[b + 1]], one), (b, "counts")
                rs = oracle.fixed_radius_search(pb, qb, RADIUS, ignore_query_point=ignore)[1]
                assert np.array_equal(gb, np.diff(rs).astype(np.float32))
                continue
            if window == "explicit":  # the sum of d^2: the oracle's identity branch sums q = d^2 / R^2
                ref = _ref_sum(oracle, qb, pb, None, ignore)
                gb = gb / np.float32(RADIUS) ** 2
            else:
                ref = _ref_sum(oracle, qb, pb, window, ignore)
            err = np.abs(gb - ref).max() / max(np.abs(ref).max(), 1e-30)
            print(f"dim {dim} ignore {ignore} {window} item {b}: max err / max|ref| {err:.2e}")
            np.testing.assert_allclose(gb, ref, rtol=2e-5, atol=2e-5 * np.abs(ref).max(), err_msg=f"{window} item {b}")


@pytest.mark.parametrize("dim", [2, 3])
def test_item_max(dev, dim):
    from dmcf_amd import ops, _lib
    pts, prs, qs, qrs = SCENES[dim]
    P, Q = _t(pts, dev), _t(qs, dev)
    for window in ops.WINDOWS:
        if window == "cubic_grad":
            continue
        for ignore in (False, True):
            out, item_max = ops.window_sum(P, Q, RADIUS, window, ignore_query_point=ignore, points_row_splits=prs,
                                           queries_row_splits=qrs, return_item_max=True)
            assert item_max.shape == (4,) and item_max.dtype == torch.float32
            for b in range(3):
                assert torch.equal(item_max[b], out[qrs[b]:qrs[b + 1]].max()), (window, ignore, b)
            assert float(item_max[3]) == 0.0  # the empty item
            assert torch.equal(out, ops.window_sum(P, Q, RADIUS, window, ignore_query_point=ignore, points_row_splits=prs,
                                                   queries_row_splits=qrs))
    with pytest.raises(_lib.DmcfError):  # its sums can be negative: the integer maximum on the bits would not order them
        ops.window_sum(P, Q, RADIUS, "cubic_grad", points_row_splits=prs, queries_row_splits=qrs, return_item_max=True)
    # under autograd: (out, item_max) with item_max outside the graph
    Pg = _t(pts, dev, True)
    out, item_max = ops.window_sum(Pg, Q, RADIUS, "poly6", points_row_splits=prs, queries_row_splits=qrs, return_item_max=True)
    assert out.grad_fn is not None and not item_max.requires_grad
    assert torch.equal(item_max[2], out[qrs[2]:qrs[3]].max().detach())


def _pairs(P, Q, ignore):
    from dmcf_amd import ops
    nns = ops.fixed_radius_search(P, Q, RADIUS, ignore_query_point=ignore, return_distances=False)
    return nns.neighbors_index.cpu().numpy(), nns.neighbors_row_splits.cpu().numpy()


def _check(name, got, want, bound):
    try:
        cref.check(name, got, want, bound, K_BAR)
    finally:
        print(f"{name}: worst err/bar {cref.WORST.get(name, 0.0):.3g}")


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("ignore", [False, True], ids=["keep_self", "ignore_query_point"])
@pytest.mark.parametrize("window", R.WINDOWS)
def test_gradient_distinct_sets_per_item(dev, window, ignore, dim):
    from dmcf_amd import ops
    pts, prs, qs, qrs = SCENES[dim]
    P, Q = _t(pts, dev, True), _t(qs, dev, True)
    G = np.random.default_rng(5).normal(size=qs.shape[0]).astype(np.float32)
    out = ops.window_sum(P, Q, RADIUS, window, ignore_query_point=ignore, points_row_splits=prs, queries_row_splits=qrs)
    assert out.grad_fn is not None
    gp, gq = torch.autograd.grad(out, [P, Q], _t(G, dev))
    gp, gq = gp.cpu().numpy(), gq.cpu().numpy()
    assert gp.shape == pts.shape and gq.shape == qs.shape and np.isfinite(gp).all() and np.isfinite(gq).all()
    for b in range(3):
        pb, qb = pts[prs[b]:prs[b + 1]], qs[qrs[b]:qrs[b + 1]]
        idx, rs = _pairs(_t(pb, dev), _t(qb, dev), ignore)
        rp, rq, ap, aq = R.WindowSum(pb, qb, idx, rs, RADIUS, window).grads(G[qrs[b]:qrs[b + 1]])
        _check(f"batched:distinct:points:{dim}d", gp[prs[b]:prs[b + 1]], rp, ap)
        _check(f"batched:distinct:queries:{dim}d", gq[qrs[b]:qrs[b + 1]], rq, aq)


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("ignore", [False, True], ids=["keep_self", "ignore_query_point"])
@pytest.mark.parametrize("window", R.WINDOWS)
def test_gradient_same_set_per_item(dev, window, ignore, dim):
    from dmcf_amd import ops
    _, _, qs, qrs = SCENES[dim]
    P = _t(qs, dev, True)
    G = np.random.default_rng(6).normal(size=qs.shape[0]).astype(np.float32)
    out = ops.window_sum(P, P, RADIUS, window, ignore_query_point=ignore, points_row_splits=qrs, queries_row_splits=qrs)
    (g,) = torch.autograd.grad(out, [P], _t(G, dev))
    g = g.cpu().numpy()
    assert np.isfinite(g).all()
    for b in range(3):
        pb = qs[qrs[b]:qrs[b + 1]]
        T = _t(pb, dev)
        idx, rs = _pairs(T, T, ignore)
        r, _, a, _ = R.WindowSum(pb, pb, idx, rs, RADIUS, window, same=True).grads(G[qrs[b]:qrs[b + 1]])
        _check(f"batched:same:{dim}d", g[qrs[b]:qrs[b + 1]], r, a)


def test_gradient_of_an_item_ignores_the_other_items(dev):
    """Item 2 lies on item 0: moving item 2's points must not change one bit of item 0's rows (nor of item 1's)."""
    from dmcf_amd import ops
    pts, prs, qs, qrs = SCENES[3]
    G = _t(np.random.default_rng(7).normal(size=qs.shape[0]), dev)

    def run(pts_, qs_):
        P, Q = _t(pts_, dev, True), _t(qs_, dev, True)
        out = ops.window_sum(P, Q, RADIUS, "cubic", points_row_splits=prs, queries_row_splits=qrs)
        return (out.detach(),) + torch.autograd.grad(out, [P, Q], G)

    base = run(pts, qs)
    # item 2's fluid points move by up to 0.02, except the ones that span its bounding box, and stay inside that box: the
    # boxes of all points and of all queries -- and with them the one grid geometry of each structure, on which the order of
    # the additions depends -- stay what they were
    fluid = qs[qrs[2]:qrs[3]]
    lo, hi = fluid.min(0), fluid.max(0)
    inner = ((fluid > lo) & (fluid < hi)).all(1)
    assert inner.sum() >= 250
    jitter = np.random.default_rng(12).uniform(-0.02, 0.02, size=fluid.shape).astype(np.float32)
    new = np.where(inner[:, None], np.clip(fluid + jitter, lo, hi), fluid).astype(np.float32)
    moved_p, moved_q = pts.copy(), qs.copy()
    moved_p[prs[2]:prs[2] + new.shape[0]] = new
    moved_q[qrs[2]:qrs[3]] = new
    other = run(moved_p, moved_q)
    assert not torch.equal(base[0][qrs[2]:qrs[3]], other[0][qrs[2]:qrs[3]])  # (the perturbation did something)
    for b in (0, 1):
        assert torch.equal(base[0][qrs[b]:qrs[b + 1]], other[0][qrs[b]:qrs[b + 1]])
        assert torch.equal(base[1][prs[b]:prs[b + 1]], other[1][prs[b]:prs[b + 1]])
        assert torch.equal(base[2][qrs[b]:qrs[b + 1]], other[2][qrs[b]:qrs[b + 1]])


def test_identical_calls_give_identical_bits(dev):
    from dmcf_amd import ops
    pts, prs, qs, qrs = SCENES[3]
    G = _t(np.random.default_rng(8).normal(size=qs.shape[0]), dev)
    runs = []
    for _ in range(2):
        P, Q = _t(pts, dev, True), _t(qs, dev, True)
        out, item_max = ops.window_sum(P, Q, RADIUS, "poly6", points_row_splits=prs, queries_row_splits=qrs, return_item_max=True)
        S = _t(qs, dev, True)
        same = ops.window_sum(S, S, RADIUS, "peak", ignore_query_point=True, points_row_splits=qrs, queries_row_splits=qrs)
        runs.append((out.detach(), item_max) + torch.autograd.grad(out, [P, Q], G) + torch.autograd.grad(same, [S], G))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_row_splits_forms_and_table_reuse(dev, monkeypatch):
    """Row splits as a list, a CPU tensor, a device tensor and an ops.RowSplits give the same bits; a matching batched
    hash_table is reused, another one is replaced."""
    from dmcf_amd import ops, _lib
    pts, prs, qs, qrs = SCENES[2]
    P, Q = _t(pts, dev), _t(qs, dev)
    want = ops.window_sum(P, Q, RADIUS, "poly6", points_row_splits=prs, queries_row_splits=qrs)
    forms = [(torch.tensor(prs), torch.tensor(qrs)), (torch.tensor(prs, device=dev), torch.tensor(qrs, device=dev)),
             (ops.RowSplits(prs, torch.tensor(prs, device=dev)), ops.RowSplits(qrs, None))]
    for p_, q_ in forms:
        assert torch.equal(ops.window_sum(P, Q, RADIUS, "poly6", points_row_splits=p_, queries_row_splits=q_), want)
    table = ops.build_spatial_hash_table(P, RADIUS, n_queries=Q.shape[0], points_row_splits=prs)
    built = []
    real = ops.build_spatial_hash_table
    monkeypatch.setattr(ops, "build_spatial_hash_table", lambda *a, **k: built.append(1) or real(*a, **k))
    assert torch.equal(ops.window_sum(P, Q, RADIUS, "poly6", hash_table=table, points_row_splits=prs, queries_row_splits=qrs), want)
    assert built == []
    plain = real(P, RADIUS, n_queries=Q.shape[0])  # (an un-batched structure does not serve)
    assert torch.equal(ops.window_sum(P, Q, RADIUS, "poly6", hash_table=plain, points_row_splits=prs, queries_row_splits=qrs), want)
    assert built == [1]
    # with both row splits None the call is the call it was: the bare tensor
    one = ops.window_sum(P, Q, RADIUS, "poly6")
    assert isinstance(one, torch.Tensor) and one.shape == (Q.shape[0],)
    with pytest.raises(_lib.DmcfError):
        ops.window_sum(P.cpu(), Q, RADIUS, "poly6", points_row_splits=prs, queries_row_splits=qrs)


@pytest.mark.parametrize("win", ["poly6", "cubic", None, "callable"])
def test_losses_with_row_splits_against_the_per_item_calls(dev, win):
    from dmcf_amd.utils.tools.losses import compute_density, density_loss, get_window_func
    pts, prs, qs, qrs = SCENES[3]
    prs, qrs = prs[:4], qrs[:4]  # (density_loss takes no empty item)
    pts, qs = pts[:prs[-1]], qs[:qrs[-1]]
    w = (lambda q: torch.clamp((1 - q) ** 3, 0, 1)) if win == "callable" else get_window_func(win)
    rng = np.random.default_rng(9)
    moved = qs + rng.normal(0, 0.01, size=qs.shape).astype(np.float32)
    moved_in = pts.copy()
    for b in range(3):  # the warm-up's case: the in set is [the out set, boundary]
        moved_in[prs[b]:prs[b] + qrs[b + 1] - qrs[b]] = moved[qrs[b]:qrs[b + 1]]
    Q, P, M, MI = _t(qs, dev), _t(pts, dev), _t(moved, dev), _t(moved_in, dev)
    d = compute_density(Q, P, RADIUS, win=w, out_row_splits=qrs, in_row_splits=prs)
    ds = compute_density(Q, None, RADIUS, win=w, out_row_splits=qrs)
    for b in range(3):
        one = compute_density(Q[qrs[b]:qrs[b + 1]], P[prs[b]:prs[b + 1]], RADIUS, win=w)
        torch.testing.assert_close(d[qrs[b]:qrs[b + 1]], one, rtol=2e-5, atol=2e-5 * float(one.abs().max()))
        one = compute_density(Q[qrs[b]:qrs[b + 1]], None, RADIUS, win=w)
        torch.testing.assert_close(ds[qrs[b]:qrs[b + 1]], one, rtol=2e-5, atol=2e-5 * float(one.abs().max()))
    for use_max in (False, True):
        for eps in ((0.01, -0.5) if not use_max else (0.01,)):  # (eps < 0: the relu term is not all zero)
            got = density_loss(Q, M, P, MI, radius=RADIUS, eps=eps, win=w, use_max=use_max, row_splits=qrs, in_row_splits=prs)
            assert got.shape == (3,)
            for b in range(3):
                a, e, ia, ie = qrs[b], qrs[b + 1], prs[b], prs[b + 1]
                want = density_loss(Q[a:e], M[a:e], P[ia:ie], MI[ia:ie], radius=RADIUS, eps=eps, win=w, use_max=use_max).item()
                print(f"{win} use_max {use_max} eps {eps} item {b}: batched {got[b].item():.6g} per item {want:.6g}")
                if np.isnan(want):  # (win=None: the lone particle of item 1 has density 0, and 0 / 0 in either form)
                    assert win is None and b == 1 and use_max and np.isnan(got[b].item())
                    continue
                assert abs(got[b].item() - want) <= 1e-4 * max(abs(want), 1e-3)
