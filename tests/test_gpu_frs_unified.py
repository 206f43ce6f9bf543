"""A single point set is a batch of one item (dmcf_amd/csrc/frs.hip: every kernel and every host phase of the radius search is
one template / one function for both families of entry points).

  1. dmcf_frs_build and dmcf_frs_build_batched(points, [0, n]) leave the same structure, byte for byte;
  2. the window sum and its gradient with [0, n] / [0, m] are the un-batched ones, bit for bit;
  3. both families stay inside a workspace of exactly dmcf_frs_workspace_bytes[_batched] bytes;
  4. an un-batched window_sum handed a batched table builds one of its own, and window_sum_backward refuses the mix.

Bit-for-bit cases run under DMCF_FRS_NO_SMALL_BUILD: a batched build never takes the single-workgroup build, which adds the box
sums in another order than the general one (the grid may then sit an ulp elsewhere, and with it the order a lane adds its terms
in).  With at most 512 points the general build's box has two partial sums per axis, whose order does not matter."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import frs_regimes as fg  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
GUARD = 4096


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but torch.cuda.is_available() is False")
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


# ---- 1. one item is the single set, at the C level ---------------------------------------------------------------------------

# (scene of frs_regimes, radius, what the device's header must show).  257 points: two frs_count_cells blocks, the second with
# one point.  div3's uniform cube at R = 0.396: cells of R / 3 are 0.132 wide, 8 per axis, 512 cells for 257 points -- one point
# per two cells holds (256 <= 257) and 512 <= 4096.  coarse's clumps between the cube's corners at the scene's own R = 0.02:
# 50^3 cells of edge R do not fit the table of 4096.
ONE_ITEM = {
    "div3": (0.396, lambda h: 2.9 < fg.cells_per_radius(h) <= 3.0 and [int(v) for v in h["dims"]] == [8, 8, 8]),
    "coarse": (0.02, lambda h: fg.cells_per_radius(h) < 0.95 and h["ncells"] <= h["table"]),
}
HEADER_FIELDS = ["origin", "inv_cell", "dims", "ncells", "bb_min", "bb_max", "radius", "n_points", "sum", "sumsq"]


@pytest.mark.parametrize("n", [257, 0])
@pytest.mark.parametrize("name", list(ONE_ITEM))
def test_one_item_build_is_the_single_set_build(dev, monkeypatch, name, n):
    from dmcf_amd import _lib, ops
    monkeypatch.setenv("DMCF_FRS_NO_SMALL_BUILD", "1")
    L = _lib.lib()
    radius, regime = ONE_ITEM[name]
    scene = fg.SCENES[name]
    pts = scene.draw(n, scene.seed) if n else np.zeros((0, 3), F)
    P = _t(pts, dev)
    splits = _t(np.array([0, n], np.int64), dev)
    nbytes = L.dmcf_frs_workspace_bytes(n, 0)
    assert nbytes == L.dmcf_frs_workspace_bytes_batched(n, 0, 1) > 0
    one = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    many = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    _lib.check(L.dmcf_frs_build(_p(P), n, radius, _p(one), nbytes, ops._stream()), "dmcf_frs_build")
    _lib.check(L.dmcf_frs_build_batched(_p(P), n, _p(splits), 1, radius, _p(many), nbytes, ops._stream()), "dmcf_frs_build_batched")
    torch.cuda.synchronize()
    a = fg.decode(ops.SpatialHashTable(P, radius, one, 0))
    b = fg.decode(ops.SpatialHashTable(P, radius, many, 0, row_splits=(0, n), row_splits_dev=splits))
    if n:
        assert regime(a), (fg.cells_per_radius(a), a["dims"], a["ncells"])
    for key in HEADER_FIELDS + ["cell_start", "sorted_xyz", "sorted_index"]:
        assert np.asarray(a[key]).tobytes() == np.asarray(b[key]).tobytes(), f"{name} n {n}: {key} differs"
    assert a["cell_start"][-1] == n and len(a["sorted_index"]) == n


# ---- 2. window sum and its gradient, one item against un-batched ---------------------------------------------------------------

def _cloud(n, m, seed):
    """n uniform points in the unit cube; m queries, the first half of them points of the set."""
    rng = np.random.default_rng(seed)
    pts = rng.uniform(0, 1, size=(n, 3)).astype(F)
    qs = np.concatenate([pts[:m // 2], rng.uniform(0, 1, size=(m - m // 2, 3)).astype(F)])
    return pts, qs, rng


@pytest.mark.parametrize("ignore", [False, True])
@pytest.mark.parametrize("window", ["poly6", "cubic"])
def test_one_item_window_sum_and_gradient_bits(dev, monkeypatch, window, ignore):
    """m = 70: 18 workgroups of four waves, the last with two."""
    from dmcf_amd import ops
    monkeypatch.setenv("DMCF_FRS_NO_SMALL_BUILD", "1")
    monkeypatch.delenv("DMCF_FRS_SET", raising=False)
    n, m, radius = 257, 70, 0.25
    pts, qs, rng = _cloud(n, m, 11)
    P, Q = _t(pts, dev), _t(qs, dev)
    a = ops.window_sum(P, Q, radius, window, ignore_query_point=ignore)
    b = ops.window_sum(P, Q, radius, window, ignore_query_point=ignore, points_row_splits=[0, n], queries_row_splits=[0, m])
    a, b = a.cpu().numpy(), b.cpu().numpy()
    assert a.shape == (m,) and a.max() > 1.0, "the scene has no neighbours to sum"
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "sums differ"
    cq, cp = _t(rng.normal(size=m).astype(F), dev), _t(rng.normal(size=n).astype(F), dev)
    one = ops.build_spatial_hash_table(P, radius, n_queries=m)
    many = ops.build_spatial_hash_table(P, radius, n_queries=m, points_row_splits=[0, n])
    for coefs in ((cq, cp), (cq, None), (None, cp)):
        ga = ops.window_sum_backward(Q, one, radius, window, *coefs, ignore_query_point=ignore)
        gb = ops.window_sum_backward(Q, many, radius, window, *coefs, ignore_query_point=ignore, queries_row_splits=[0, m])
        ga, gb = ga.cpu().numpy(), gb.cpu().numpy()
        assert ga.shape == (m, 3) and np.abs(ga).max() > 0
        assert np.array_equal(ga.view(np.uint32), gb.view(np.uint32)), "gradients differ"


# ---- 3. exact-size workspace between guards ------------------------------------------------------------------------------------

def _run_family(dev, P, Q, radius, splits, slack):
    """build, count, write, window sum and window-sum backward through the C entry points, on a workspace of exactly the
    bytes the library asks for plus ``slack``, between two GUARD-byte regions of 0xA5.  -> (results, the two guards)."""
    from dmcf_amd import _lib, ops
    L = _lib.lib()
    n, m = P.shape[0], Q.shape[0]
    stream = ops._stream()
    if splits is None:
        nbytes = L.dmcf_frs_workspace_bytes(n, m)
        item, sfx, build_item = (), "", ()
    else:
        prs, qrs = (_t(np.array(s, np.int64), dev) for s in splits)
        batch = len(splits[0]) - 1
        nbytes = L.dmcf_frs_workspace_bytes_batched(n, m, batch)
        item, sfx, build_item = (_p(qrs), batch), "_batched", (_p(prs), batch)
    nbytes += slack
    buf = torch.full((GUARD + nbytes + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    ws = buf[GUARD:GUARD + nbytes]
    assert ws.data_ptr() % 256 == 0

    def call(name, *args):
        _lib.check(getattr(L, name + sfx)(*args, stream), name + sfx)

    call("dmcf_frs_build", _p(P), n, *build_item, radius, _p(ws), nbytes)
    rs = torch.empty(m + 1, dtype=torch.int64, device=dev)
    call("dmcf_frs_count", _p(Q), m, *item, n, radius, 1, _p(ws), nbytes, _p(rs))
    total = int(rs[-1].item())
    index = torch.full((total + 64,), -7, dtype=torch.int32, device=dev)
    dist = torch.full((total + 64,), -7.0, dtype=torch.float32, device=dev)
    call("dmcf_frs_write", _p(Q), m, *item, n, radius, 1, _p(ws), nbytes, _p(rs), _p(index), _p(dist), total)
    out = torch.full((m,), -7.0, dtype=torch.float32, device=dev)
    extra = () if splits is None else (None,)  # (item_max)
    call("dmcf_frs_window_sum", _p(Q), m, *item, n, radius, 0, ops.WINDOWS["poly6"], _p(ws), nbytes, _p(out), *extra)
    cq = torch.ones(m, dtype=torch.float32, device=dev)
    grad = torch.full((m, 3), -7.0, dtype=torch.float32, device=dev)
    call("dmcf_frs_window_sum_backward", _p(Q), m, *item, n, radius, 0, ops.WINDOWS["poly6"], _p(cq), None, _p(ws), nbytes, _p(grad))
    torch.cuda.synchronize()
    results = [t.cpu().numpy() for t in (rs, index, dist, out, grad)]
    return total, results, (buf[:GUARD].cpu().numpy(), buf[GUARD + nbytes:].cpu().numpy())


@pytest.mark.parametrize("family", ["single, one-workgroup build", "single, general build", "batched"])
def test_exact_workspace_between_guards(dev, monkeypatch, family):
    """n = m = 70; the batch has three items, the middle one empty."""
    if family == "single, one-workgroup build":
        monkeypatch.delenv("DMCF_FRS_NO_SMALL_BUILD", raising=False)
    else:
        monkeypatch.setenv("DMCF_FRS_NO_SMALL_BUILD", "1")
    n = m = 70
    pts, qs, _ = _cloud(n, m, 12)
    P, Q = _t(pts, dev), _t(qs, dev)
    splits = ([0, 30, 30, 70], [0, 25, 25, 70]) if family == "batched" else None
    total, exact, guards = _run_family(dev, P, Q, 0.3, splits, 0)
    assert total > m, "the scene has no neighbours"
    for g in guards:
        assert len(g) == GUARD and np.all(g == 0xA5), f"{family}: a guard next to the workspace was written"
    _, roomy, _ = _run_family(dev, P, Q, 0.3, splits, 1 << 20)
    for what, a, b in zip(("row splits", "index", "distances", "window sums", "gradient"), exact, roomy):
        assert a.tobytes() == b.tobytes(), f"{family}: {what} depend on the size of the workspace"
    assert np.all(exact[1][total:] == -7) and np.all(exact[2][total:] == -7), "written beyond the last row"


# ---- 4. a batched table does not serve an un-batched call ---------------------------------------------------------------------

def test_unbatched_window_sum_does_not_use_a_batched_table(dev, monkeypatch):
    from dmcf_amd import ops
    monkeypatch.delenv("DMCF_FRS_SET", raising=False)
    rng = np.random.default_rng(13)
    pts = rng.uniform(0, 0.1, size=(16, 3)).astype(F)  # two items of 8 points in one cube whose diagonal is below the radius
    P = _t(pts, dev)
    radius, splits = 0.25, [0, 8, 16]
    batched = ops.build_spatial_hash_table(P, radius, points_row_splits=splits)
    want = ops.window_sum(P, P, radius, "poly6").cpu().numpy()
    got = ops.window_sum(P, P, radius, "poly6", hash_table=batched).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    per_item = ops.window_sum(P, P, radius, "poly6", hash_table=batched, points_row_splits=splits, queries_row_splits=splits)
    assert np.all(want > per_item.cpu().numpy()), "the items do not overlap: the misuse would not show"
    g = torch.ones(16, dtype=torch.float32, device=dev)
    with pytest.raises(ValueError):
        ops.window_sum_backward(P, batched, radius, "poly6", coef_queries=g)
    single = ops.build_spatial_hash_table(P, radius)
    with pytest.raises(ValueError):
        ops.window_sum_backward(P, single, radius, "poly6", coef_queries=g, queries_row_splits=splits)
