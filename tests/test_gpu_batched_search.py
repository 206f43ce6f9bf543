"""GPU tests of the batched neighbour search (points_row_splits / queries_row_splits in ops.fixed_radius_search,
ops.radius_search, FixedRadiusSearch, RadiusSearch, build_spatial_hash_table) and of ContinuousConv on a batch in one call.

Reference and scenes: tests/batched_search_ref.py (a float32 brute force per item; tests/test_batched_search_ref_cpu.py holds
it to the oracle and the scenes to their conditions).  Bars of the search, as in tests/test_gpu_radius_search.py: row lengths
equal, per-row index sets equal, squared distances bit-exact, normalised distances within 1 ulp.  Bars of the layer: the
forward element-wise within (kbar * A + C_GEO * A1) * 2^-24 of the float64 reference (cconv_forward_ref.check_forward), both
gradients within kbar * 2^-24 * A (cconv_backward_ref.check), with kbar, A and A1 formed as tests/test_gpu_cconv_forward_bar.py
and tests/test_gpu_cconv_backward_sets.py form them."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import batched_search_ref as bs  # noqa: E402
import cconv_backward_ref as ref  # noqa: E402
import cconv_forward_ref as fr  # noqa: E402
import frs_regimes as fg  # noqa: E402
from test_gpu_cconv_backward_sets import _kbars  # noqa: E402
from test_gpu_radius_search import _canonical, _check_rows, brute_force  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but torch.cuda.is_available() is False")
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)  # (a copy: the scenes are read-only)


def _search(s, dev, ignore=False, form="list", **kw):
    """ops.fixed_radius_search on scene ``s`` with its row splits given as a list, a CPU tensor or a device tensor."""
    from dmcf_amd import ops
    conv = {"list": lambda a: [int(v) for v in a], "cpu": lambda a: torch.from_numpy(np.array(a)),
            "device": lambda a: _t(np.array(a), dev)}[form]
    return ops.fixed_radius_search(_t(s["points"], dev), _t(s["queries"], dev), s["radius"], ignore_query_point=ignore,
                                   points_row_splits=conv(s["prs"]), queries_row_splits=conv(s["qrs"]), **kw)


def _header(s, dev):
    """The header of the batched structure of scene ``s``, read back from the device (frs_regimes.decode)."""
    from dmcf_amd import ops
    table = ops.build_spatial_hash_table(_t(s["points"], dev), s["radius"], n_queries=s["queries"].shape[0],
                                         points_row_splits=[int(v) for v in s["prs"]])
    return fg.decode(table)


def _check_scene(name, dev, ignore=False, dim=3, form="list", **kw):
    s = bs.scene(name, dim)
    res = _search(s, dev, ignore, form, **kw)
    assert res.neighbors_index.dtype == torch.int32 and res.neighbors_row_splits.dtype == torch.int64
    assert res.neighbors_row_splits.shape[0] == s["queries"].shape[0] + 1
    _check_rows(res, bs.reference(name, ignore, dim), None, normalized=False)
    h = _header(s, dev)
    assert h["ncells"] * (len(s["prs"]) - 1) <= h["table"], "the slabs of the batch do not fit the cell table"
    return s, res


@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("ignore", [False, True])
def test_overlapping_items(dev, dim, ignore):
    s, res = _check_scene("overlapping", dev, ignore, dim)
    # every index of a row lies in the row's own item
    idx, rs = res.neighbors_index.cpu().numpy(), res.neighbors_row_splits.cpu().numpy()
    item_of_query = np.repeat(np.arange(5), np.diff(s["qrs"]))
    item_of_pair = np.repeat(item_of_query, np.diff(rs))
    assert np.all(idx >= s["prs"][item_of_pair]) and np.all(idx < s["prs"][item_of_pair + 1])


def test_row_splits_forms_and_capacity_hint(dev):
    ref_rows = bs.reference("overlapping")
    for form in ("cpu", "device"):
        _check_scene("overlapping", dev, form=form)
    # an estimate of the pair count: count and write are enqueued back to back, the result is validated when it is read (and
    # repeated with exact buffers if the estimate was too small), as without row splits
    s, _ = _check_scene("overlapping", dev, capacity_hint=int(ref_rows[1][-1]))
    _check_rows(_search(s, dev, capacity_hint=1), ref_rows, None, normalized=False)


def test_layers_pass_row_splits_on(dev):
    from dmcf_amd import ops
    s = bs.scene("overlapping")
    P, Q = _t(s["points"], dev), _t(s["queries"], dev)
    res = ops.FixedRadiusSearch(return_distances=True, ignore_query_point=True)(
        P, Q, s["radius"], points_row_splits=_t(s["prs"], dev), queries_row_splits=_t(s["qrs"], dev))
    _check_rows(res, bs.reference("overlapping", True), None, normalized=False)
    res = ops.FixedRadiusSearch(return_distances=False)(P, Q, torch.tensor(s["radius"]), list(s["prs"]), list(s["qrs"]))
    assert res.neighbors_distance.numel() == 0
    assert np.array_equal(res.neighbors_row_splits.cpu().numpy(), bs.reference("overlapping")[1])


def test_item_edges(dev):
    """The first and the last query of every item, each against the brute force over its own item alone."""
    s, res = _check_scene("edges", dev)
    idx, rs, d2 = (x.cpu().numpy() for x in res)
    checked = 0
    for b in range(len(s["prs"]) - 1):
        pts, qs, p0, q0 = bs.item_rows(s, b)
        for name, q in (("first", 0), ("last", qs.shape[0] - 1)):
            if qs.shape[0] == 0:
                continue
            row = slice(rs[q0 + q], rs[q0 + q + 1])
            if pts.shape[0] == 0:
                assert row.start == row.stop, f"{name} query of item {b}: an item without points has neighbours"
                continue
            i0, _, d0 = brute_force(pts, qs[q:q + 1], np.float32([s["radius"]]))
            order = np.argsort(idx[row])
            assert np.array_equal(idx[row][order], i0 + p0), f"{name} query of item {b}"
            assert np.array_equal(d2[row][order].view(np.uint32), d0.view(np.uint32)), f"{name} query of item {b}"
            checked += 1
    assert checked == 8


def test_strays_and_far_items(dev):
    s, res = _check_scene("strays", dev)
    _check_scene("strays", dev, ignore=True)
    idx, rs = res.neighbors_index.cpu().numpy(), res.neighbors_row_splits.cpu().numpy()
    for q, p in zip(s["stray_queries"], s["stray_points"]):
        assert p in idx[rs[q]:rs[q + 1]]
    for q in s["foreign_queries"]:
        assert rs[q] == rs[q + 1], "a query found the stray point of another item"
    # the one grid of the call is coarse: asserted from the device's header
    assert fg.cells_per_radius(_header(s, dev)) < 0.95


def test_many_items(dev):
    _check_scene("many", dev)
    _check_scene("many", dev, ignore=True, form="device")


def test_table_bound(dev):
    s, _ = _check_scene("table_bound", dev)
    _check_scene("table_bound", dev, ignore=True)
    # the build had to take cells coarser than R / 3 (tests/test_batched_search_ref_cpu.py predicts it): the device's header
    assert fg.cells_per_radius(_header(s, dev)) < 2.9


def test_one_item_is_the_unbatched_search(dev):
    from dmcf_amd import ops
    s = bs.scene("overlapping")
    P, Q = _t(s["points"], dev), _t(s["queries"], dev)
    n, m = P.shape[0], Q.shape[0]
    for ignore in (False, True):
        a = ops.fixed_radius_search(P, Q, s["radius"], ignore_query_point=ignore, points_row_splits=[0, n], queries_row_splits=[0, m])
        b = ops.fixed_radius_search(P, Q, s["radius"], ignore_query_point=ignore)
        ia, ra, da = (x.cpu().numpy() for x in a)
        ib, rb, db = (x.cpu().numpy() for x in b)
        assert np.array_equal(ra, rb)
        ca, cda = _canonical(ia, ra, da)
        cb, cdb = _canonical(ib, rb, db)
        assert np.array_equal(ca, cb) and np.array_equal(cda.view(np.uint32), cdb.view(np.uint32))
    radii = _t(np.random.default_rng(3).uniform(0.04, 0.16, size=m).astype(np.float32), dev)
    a = ops.radius_search(P, Q, radii, points_row_splits=[0, n], queries_row_splits=[0, m])
    b = ops.radius_search(P, Q, radii)
    ia, ra, da = (x.cpu().numpy() for x in a)
    ib, rb, db = (x.cpu().numpy() for x in b)
    assert np.array_equal(ra, rb)
    ca, cda = _canonical(ia, ra, da)
    cb, cdb = _canonical(ib, rb, db)
    assert np.array_equal(ca, cb) and np.array_equal(cda.view(np.uint32), cdb.view(np.uint32))


def test_hash_table_remembers_its_row_splits(dev):
    from dmcf_amd import ops
    s = bs.scene("overlapping")
    P, Q = _t(s["points"], dev), _t(s["queries"], dev)
    prs, qrs = [int(v) for v in s["prs"]], [int(v) for v in s["qrs"]]
    table = ops.build_spatial_hash_table(P, s["radius"], n_queries=Q.shape[0], points_row_splits=_t(s["prs"], dev))
    assert table.row_splits == tuple(prs) and table.row_splits_dev.is_cuda
    built = []
    real = ops.build_spatial_hash_table

    def counting(*a, **kw):
        built.append(kw.get("points_row_splits"))
        return real(*a, **kw)

    ops.build_spatial_hash_table = counting
    try:
        res = ops.fixed_radius_search(P, Q, s["radius"], hash_table=table, points_row_splits=prs, queries_row_splits=qrs)
        assert built == [], "a table with the call's row splits was rebuilt"
        _check_rows(res, bs.reference("overlapping"), None, normalized=False)
        # a table built with other splits (one item) is rebuilt, not searched
        other = real(P, s["radius"], n_queries=Q.shape[0], points_row_splits=[0, P.shape[0]])
        res = ops.fixed_radius_search(P, Q, s["radius"], hash_table=other, points_row_splits=prs, queries_row_splits=qrs)
        assert len(built) == 1 and built[0] is not None
        _check_rows(res, bs.reference("overlapping"), None, normalized=False)
        # and the un-batched search does not take a batched table
        res = ops.fixed_radius_search(P, Q, s["radius"], hash_table=table)
        assert len(built) == 2 and built[1] is None
        want = brute_force(s["points"], s["queries"], np.full(Q.shape[0], s["radius"], np.float32))
        _check_rows(res, want, None, normalized=False)
    finally:
        ops.build_spatial_hash_table = real


@pytest.mark.parametrize("ignore", [False, True])
def test_radius_search(dev, ignore):
    """The overlapping scene with a radius per query over a 4x range, every 37th radius 0."""
    from dmcf_amd import ops
    s = bs.scene("overlapping")
    m = s["queries"].shape[0]
    radii = np.random.default_rng(41).uniform(0.05, 0.2, size=m).astype(np.float32)
    radii[::37] = 0.0
    want = bs.batched_brute_force(s["points"], s["queries"], radii, s["prs"], s["qrs"], ignore)
    P, Q, R = _t(s["points"], dev), _t(s["queries"], dev), _t(radii, dev)
    splits = dict(points_row_splits=list(s["prs"]), queries_row_splits=_t(s["qrs"], dev))
    res = ops.radius_search(P, Q, R, ignore_query_point=ignore, normalize_distances=False, **splits)
    _check_rows(res, want, radii, normalized=False)
    res = ops.RadiusSearch(ignore_query_point=ignore, return_distances=True, normalize_distances=True)(P, Q, R, **splits)
    _check_rows(res, want, radii, normalized=True)
    if not ignore:
        # a radius-0 row holds exactly the points of its item at the query's coordinates (item 3 coincides with item 0)
        idx, rs = res.neighbors_index.cpu().numpy(), res.neighbors_row_splits.cpu().numpy()
        seen = 0
        for i in np.nonzero(radii == 0)[0]:
            b = int(np.searchsorted(s["qrs"], i, side="right") - 1)
            pts, _, p0, _ = bs.item_rows(s, b)
            same = np.nonzero(np.all(pts == s["queries"][i], axis=1))[0] + p0
            assert np.array_equal(np.sort(idx[rs[i]:rs[i + 1]]), same)
            seen += same.size
        assert seen > 0


# ---- the layer ---------------------------------------------------------------------------------------------------------------


def _layer_case(dev, same, window, rank1=False):
    from dmcf_amd.utils.convolutions import ContinuousConv
    from dmcf_amd.utils.tools.losses import get_window_func
    s = bs.layer_scene()
    inp, out = s["inp"], (s["inp"] if same else s["out"])
    irs, ors = s["irs"], (s["irs"] if same else s["ors"])
    G = s["grad_same"] if same else s["grad_sep"]
    ext = (s["ext_same"] if same else s["ext_sep"]) if rank1 else np.float32(bs.LAYER_EXTENT)
    idx, rs, _ = bs.batched_brute_force(inp, out, np.float32(0.5) * ext, irs, ors)
    tag = f"batched layer {'same' if same else 'separate'} {window}{' rank1' if rank1 else ''}"

    layer = ContinuousConv(filters=16, kernel_size=[4, 4, 4], use_bias=False, window_function=get_window_func(window), device=dev,
                           record_per_point_extents=rank1)
    layer.build(8, dev)
    with torch.no_grad():
        layer.kernel.copy_(_t(s["filt"], dev))
    P_inp = _t(inp, dev)
    P_out = P_inp if same else _t(out, dev)
    extent = _t(ext, dev) if rank1 else float(ext)
    splits = dict(inp_positions_row_splits=_t(irs, dev), out_positions_row_splits=[int(v) for v in ors])

    with torch.no_grad():
        y_inf = layer(_t(s["feat"], dev), P_inp, P_out, extent, **splits)
    li, lr, _ = layer.nns
    assert np.array_equal(lr.cpu().numpy(), rs), f"{tag}: the layer's list is not the batched list"
    assert np.array_equal(_canonical(li.cpu().numpy(), rs)[0], _canonical(idx, rs)[0])

    layer.requires_grad_(True)
    X = _t(s["feat"], dev).requires_grad_(True)
    y = layer(X, P_inp, P_out, extent, **splits)
    (y * _t(G, dev)).sum().backward()
    gw, gf = layer.kernel.grad.cpu().numpy(), X.grad.cpu().numpy()

    pw = ref.PairWeights(out, inp, idx, rs, ext, [4, 4, 4], window=window, window_fac=1.0, mapping=layer.coordinate_mapping,
                         interpolation=layer.interpolation, align_corners=layer.align_corners, f64=True)
    kw = dict(normalize=layer.normalize)
    want, A, A1 = fr.forward_bar(pw, s["filt"], s["feat"], window=window, window_fac=1.0, **kw)
    kbar = fr.kbar_of(pw, 8)
    fr.check_forward(tag + ":inference", y_inf.cpu().numpy(), want, A, A1, kbar)
    fr.check_forward(tag + ":recording", y.detach().cpu().numpy(), want, A, A1, kbar)
    rw, rf, _ = ref.grads(pw, s["filt"], s["feat"], G, **kw)
    aw, af, _ = ref.grads(pw, s["filt"], s["feat"], G, abs_mode=True, **kw)
    kbar_w, kbar_f = _kbars(pw, 64, 8, 16)
    print(f"{tag}: pairs {idx.size}, kbar {kbar} / {kbar_w} / {kbar_f}, worst err / bar: filters "
          f"{np.max(np.abs(gw - rw) / (kbar_w * ref.EPS * np.maximum(aw, 1e-6 * aw.max()))):.3g}, features "
          f"{np.max(np.abs(gf - rf) / (kbar_f * ref.EPS * np.maximum(af, 1e-6 * af.max()))):.3g}")
    ref.check(tag + ":filters", gw, rw, aw, kbar_w)
    ref.check(tag + ":features", gf, rf, af, kbar_f)
    # an input point no output of its item reaches gets no gradient; an output without input points is exactly zero
    unref = np.bincount(pw.j, minlength=inp.shape[0]) == 0
    assert np.all(gf[unref] == 0)
    empty = np.diff(rs) == 0
    assert np.all(y.detach().cpu().numpy()[empty] == 0)
    return pw


@pytest.mark.parametrize("window", [None, "poly6"])
@pytest.mark.parametrize("same", [True, False])
def test_layer(dev, same, window):
    pw = _layer_case(dev, same, window)
    if not same:  # (item 1's outputs have no input points)
        assert np.all(np.bincount(pw.i, minlength=250)[200:] == 0)
    assert pw.i.size > 0


def test_layer_rank1_extents(dev):
    from dmcf_amd.utils.convolutions import ContinuousConv
    _layer_case(dev, False, "poly6", rank1=True)
    _layer_case(dev, True, None, rank1=True)
    # recording through extents of rank 1 stays opt-in, with row splits as without
    s = bs.layer_scene()
    layer = ContinuousConv(filters=16, kernel_size=[4, 4, 4], use_bias=False, device=dev)
    P = _t(s["inp"], dev)
    with pytest.raises(NotImplementedError):
        layer(_t(s["feat"], dev).requires_grad_(True), P, P, _t(s["ext_same"], dev), inp_positions_row_splits=list(s["irs"]),
              out_positions_row_splits=list(s["irs"]))
