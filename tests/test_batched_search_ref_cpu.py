"""CPU checks of the batched search's reference (tests/batched_search_ref.py): the helper against the oracle's brute force called
once per item, and the conditions on the scenes that keep tests/test_gpu_batched_search.py from passing vacuously."""
import numpy as np
import pytest

pytest.importorskip("torch")  # (tests/test_gpu_radius_search.py, whose brute force the reference is, imports it)

import batched_search_ref as bs  # noqa: E402
from test_gpu_radius_search import brute_force, _canonical  # noqa: E402

SEARCH_SCENES = ["overlapping", "edges", "strays", "many", "table_bound"]


@pytest.mark.parametrize("ignore", [False, True])
@pytest.mark.parametrize("name,dim", [("overlapping", 3), ("overlapping", 2), ("edges", 3), ("strays", 3)])
def test_reference_is_the_oracle_per_item(oracle, name, dim, ignore):
    s = bs.scene(name, dim)
    idx, rs, d2 = bs.reference(name, ignore, dim)
    assert rs.shape[0] == s["queries"].shape[0] + 1 and rs[0] == 0 and rs[-1] == idx.shape[0] == d2.shape[0]
    for b in range(len(s["prs"]) - 1):
        pts, qs, p0, q0 = bs.item_rows(s, b)
        if qs.shape[0] == 0:
            continue
        lo, hi = rs[q0], rs[q0 + qs.shape[0]]
        if pts.shape[0] == 0:
            assert lo == hi
            continue
        i0, r0, d0 = oracle.fixed_radius_search(np.ascontiguousarray(pts), np.ascontiguousarray(qs), s["radius"], ignore,
                                                bruteforce=True)
        assert np.array_equal(rs[q0:q0 + qs.shape[0] + 1] - lo, r0), f"item {b}: row lengths"
        a, da = _canonical(idx[lo:hi] - p0, r0, d2[lo:hi])
        c, dc = _canonical(i0, r0, d0)
        assert np.array_equal(a, c), f"item {b}: neighbour sets"
        assert np.array_equal(da.view(np.uint32), dc.view(np.uint32)), f"item {b}: squared distances"


def test_per_query_radii_follow_the_query():
    s = bs.scene("overlapping")
    m = s["queries"].shape[0]
    radii = np.random.default_rng(1).uniform(0.04, 0.16, size=m).astype(np.float32)
    radii[::37] = 0
    idx, rs, d2 = bs.batched_brute_force(s["points"], s["queries"], radii, s["prs"], s["qrs"])
    assert np.all(d2 <= np.repeat(radii * radii, np.diff(rs)))
    pts, qs, p0, q0 = bs.item_rows(s, 3)
    i3, r3, _ = brute_force(pts, qs, radii[q0:q0 + qs.shape[0]])
    assert np.array_equal(np.diff(rs)[q0:q0 + qs.shape[0]], np.diff(r3))


@pytest.mark.parametrize("dim", [3, 2])
def test_overlapping_scene_would_show_a_leak(dim):
    """Searched as ONE point set the scene has strictly more pairs than searched by item: pairs across items exist."""
    s = bs.scene("overlapping", dim)
    for ignore in (False, True):
        _, rs_all, _ = brute_force(s["points"], s["queries"], np.full(s["queries"].shape[0], s["radius"], np.float32), ignore)
        _, rs_item, _ = bs.reference("overlapping", ignore, dim)
        assert rs_all[-1] > rs_item[-1]
        assert np.all(np.diff(rs_all) >= np.diff(rs_item))
    # the sizes the scene promises, the coincident items, the queries on points
    assert np.diff(s["prs"]).tolist() == list(bs.OVERLAP_POINTS) and np.diff(s["qrs"]).tolist() == list(bs.OVERLAP_QUERIES)
    p0, p3 = bs.item_rows(s, 0)[0], bs.item_rows(s, 3)[0]
    assert np.array_equal(p3, p0[:700])
    on = 0
    for b in range(5):
        pts, qs, _, _ = bs.item_rows(s, b)
        if pts.shape[0] and qs.shape[0]:
            on += int(np.sum((qs[:, None, :] == pts[None, :, :]).all(-1).any(1)))
    assert on >= s["on_points"] == 600
    assert np.abs(s["points"]).max() <= 1 and np.abs(s["queries"]).max() <= 1


@pytest.mark.parametrize("name", SEARCH_SCENES)
def test_rows_are_long_enough(name):
    for dim in ((3, 2) if name == "overlapping" else (3,)):
        s = bs.scene(name, dim)
        means = bs.mean_row_lengths(s, bs.reference(name, False, dim))
        assert means, "no item with points and queries"
        assert min(means.values()) >= 8, {b: round(v, 2) for b, v in means.items() if v < 8}


def test_strays_have_neighbours_in_their_item_only():
    s = bs.scene("strays")
    idx, rs, _ = bs.reference("strays")
    for q, p in zip(s["stray_queries"], s["stray_points"]):
        assert p in idx[rs[q]:rs[q + 1]], "a stray point without its in-item neighbour query"
    for q in s["foreign_queries"]:  # (item 1's queries at the same places: the un-batched search would pair them)
        assert rs[q + 1] == rs[q]
        assert np.square(s["points"][s["stray_points"]] - s["queries"][q]).sum(1).min() <= np.float32(s["radius"]) ** 2
    assert np.array_equal(s["points"][s["stray_points"]], bs.STRAYS)


def test_edges_scene_has_the_empty_items():
    s = bs.scene("edges")
    npts, nq = np.diff(s["prs"]), np.diff(s["qrs"])
    assert npts[0] == nq[0] == 0 and npts[-1] == nq[-1] == 0          # first and last
    assert npts[2] == npts[3] == 0 and nq[3] == 0 and nq[2] > 0        # twice in a row, one of them with queries
    assert 1 in nq.tolist() and 2 in nq.tolist()


def test_many_and_table_bound_sizes():
    s = bs.scene("many")
    npts = np.diff(s["prs"])
    assert npts.shape[0] == 130 and npts.min() == 50 and npts.max() == 400 and np.all(s["points"][:, 2] == 0)
    t = bs.scene("table_bound")
    n = t["points"].shape[0]
    assert n == 16 * 2025 and t["points"].min() == 0 and t["points"].max() == 1
    # cells of edge 1.001 R / 3 over the unit square, times 16 items, against the table of 4 n entries (dmcf_amd/csrc/frs.hip)
    per_axis = np.floor(1.0 / (t["radius"] * 1.001 / 3)) + 1
    assert per_axis * per_axis * 16 > 4 * n


def test_layer_scene_sizes():
    s = bs.layer_scene()
    assert np.diff(s["irs"]).tolist() == [300, 0, 450] and np.diff(s["ors"]).tolist() == [200, 50, 0]
    assert np.abs(s["inp"]).max() <= 0.5 and np.abs(s["out"]).max() <= 0.5
    for e in (s["ext_same"], s["ext_sep"]):
        assert len(np.unique(e)) == 2
