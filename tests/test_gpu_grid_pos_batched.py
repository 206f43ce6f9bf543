"""grid_pos and points_aabb with row splits (ABI 2.21) against the un-batched calls on every item's slice: bit for bit, in order."""
import numpy as np
import pytest

import batched_scene as scene

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

V = scene.VOXEL


@pytest.fixture(scope="module")
def batch():
    from dmcf_amd import ops  # noqa: F401  (loads the library)
    pos, rs = scene.concat(scene.fluid_items())
    return torch.from_numpy(pos).cuda(), rs


def _per_item(ops, pos, rs, voxel, **kw):
    center = kw.pop("center", None)
    out = []
    for b in range(len(rs) - 1):
        item = pos[rs[b]:rs[b + 1]].clone()
        if item.shape[0] == 0:
            out.append(pos.new_zeros((0, 3)))
            continue
        out.append(ops.grid_pos(item, voxel, center=None if center is None else center[b], **kw))
    return out


def _check(ops, pos, rs, voxel, got, splits, **kw):
    want = _per_item(ops, pos, rs, voxel, **kw)
    host = [0]
    for w in want:
        host.append(host[-1] + w.shape[0])
    assert list(splits.host) == host
    assert splits.dev.dtype == torch.int64 and splits.dev.is_cuda and splits.dev.tolist() == host
    assert got.shape == (host[-1], 3) and got.dtype == torch.float32
    for b, w in enumerate(want):
        assert torch.equal(got[host[b]:host[b + 1]], w), f"item {b}"
    return host


@pytest.mark.parametrize("flat", [False, True])
@pytest.mark.parametrize("pad", [0, 1])
@pytest.mark.parametrize("centralize", [False, True])
def test_items_equal_the_unbatched_call(batch, centralize, pad, flat):
    from dmcf_amd import ops
    pos, rs = batch
    if not flat:  # a 3-D cloud of the same items
        g = torch.Generator().manual_seed(3)
        pos = pos.clone()
        pos[:, 2] = (torch.rand(scene.COUNTS[2], generator=g) * 0.2)[torch.tensor(
            list(range(180)) + [0] + list(range(260)))].cuda()
    voxel = np.array([V, V, 0.0 if flat else V], dtype=np.float32)
    for _ in range(2):  # (the second call sizes its tables from the first one's cells: the estimate path)
        got, splits = ops.grid_pos(pos, voxel, centralize=centralize, pad=pad, row_splits=rs)
        host = _check(ops, pos, rs, voxel, got, splits, centralize=centralize, pad=pad)
        assert not splits.sparse
    assert host[1] > 0 and host[2] - host[1] > 0 and host[3] - host[2] >= host[1]
    # items 0 and 2 share coordinates: item 2's lattice holds every point of item 0's when neither is centred on its own mean
    if not centralize:
        a = {tuple(r) for r in got[host[0]:host[1]].tolist()}
        c = {tuple(r) for r in got[host[2]:host[3]].tolist()}
        assert a <= c


def test_two_levels_and_an_empty_item(batch):
    from dmcf_amd import ops
    pos, rs = batch
    rs4 = rs + [rs[-1]]  # a fourth, empty item
    rs5 = [0, 0] + rs4[1:]  # ... and an empty first one
    for splits_in in (rs4, rs5, torch.tensor(rs4), torch.tensor(rs4).cuda()):
        host_in = splits_in.tolist() if isinstance(splits_in, torch.Tensor) else splits_in
        sizes = [np.array([V * s, V * s, 0.0], dtype=np.float32) for s in (2, 4)]
        res = ops.grid_pos_many(pos, sizes, centralize=True, pad=1, row_splits=splits_in)
        assert len(res) == 2
        for voxel, (got, splits) in zip(sizes, res):
            host = _check(ops, pos, host_in, voxel, got, splits, centralize=True, pad=1)
            assert host[-1] == host[-2]
        assert res[0][0].shape[0] > res[1][0].shape[0]


def test_given_centers(batch):
    from dmcf_amd import ops
    pos, rs = batch
    centers = torch.tensor([[0.01, 0.02, 0.0], [0.3, 5.0, 0.0], [-0.013, 0.007, 0.0]], device="cuda")
    voxel = np.array([V, V, 0.0], dtype=np.float32)
    got, splits = ops.grid_pos(pos, voxel, centralize=True, center=centers, row_splits=rs)
    _check(ops, pos, rs, voxel, got, splits, centralize=True, center=centers)


def test_one_item_is_the_unbatched_call(batch):
    from dmcf_amd import ops
    pos, rs = batch
    voxel = np.array([V, V, 0.0], dtype=np.float32)
    for centralize in (False, True):
        got, splits = ops.grid_pos(pos, voxel, centralize=centralize, pad=1, row_splits=[0, pos.shape[0]])
        want = ops.grid_pos(pos, voxel, centralize=centralize, pad=1)
        assert torch.equal(got, want)
        assert list(splits.host) == [0, want.shape[0]] and splits.dev.tolist() == [0, want.shape[0]]


def test_large_item_sums_like_the_unbatched_call():
    """More than one block per item, and more blocks than one wavefront has lanes: the mean's two-stage sum."""
    from dmcf_amd import ops
    g = torch.Generator().manual_seed(11)
    pos = (torch.rand(40000, 3, generator=g) * torch.tensor([2.0, 1.0, 0.0])).cuda()
    rs = [0, 300, 20300, 40000]
    voxel = np.array([V, V, 0.0], dtype=np.float32)
    got, splits = ops.grid_pos(pos, voxel, centralize=True, row_splits=rs)
    _check(ops, pos, rs, voxel, got, splits, centralize=True)


def test_sparse_items_take_the_hashed_table(batch, monkeypatch):
    """A correction of the issue's case.  It asks for items that lie 1e4 voxels apart, "so the per-call sparse rule selects the
    hashed table".  The same issue makes every item's cells local to the item's own box, and then the distance between items
    does not enter the cell count at all: such a call is small and DENSE, which is asserted here -- with the bit-exact
    comparison -- as the right behaviour.  The hashed table is reached the two ways that remain: an item whose OWN points lie
    1e4 voxels apart on two axes (a box of 1e8 cells: the rule as shipped fires), and the shared scene with the rule's
    thresholds set to zero (items 0 and 2 hash the same local cells and must stay apart by the item in the key).  Each
    asserts that the hashed table was taken and compares every item bit for bit."""
    from dmcf_amd import ops
    pos, rs = batch
    voxel = np.array([V, V, 0.0], dtype=np.float32)
    # the items 1e4 voxels apart: every item's cells are local to its own box, so the call stays small and dense ...
    apart = pos.clone()
    for b in range(3):
        apart[rs[b]:rs[b + 1], :2] += b * 1.0e4 * V
    got, splits = ops.grid_pos(apart, voxel, pad=1, row_splits=rs)
    _check(ops, apart, rs, voxel, got, splits, pad=1)
    assert not splits.sparse
    # ... and an item whose own points lie 1e4 voxels apart on two axes has a box of 1e8 cells: the sparse rule of the call
    spread = apart.clone()
    spread[rs[2]:rs[2] + 50, :2] -= 1.0e4 * V
    for centralize in (False, True):
        got, splits = ops.grid_pos(spread, voxel, centralize=centralize, pad=1, row_splits=rs)
        assert splits.sparse
        _check(ops, spread, rs, voxel, got, splits, centralize=centralize, pad=1)
    # the hashed table on the shared scene itself (the rule forced): items 0 and 2 hash the same local cells, keyed apart
    monkeypatch.setattr(ops, "GRID_MIN_CELLS", 0)
    monkeypatch.setattr(ops, "GRID_MAX_CELLS_PER_POINT", 0)
    got, splits = ops.grid_pos(pos, voxel, pad=1, hyst=0.2, row_splits=rs)
    assert splits.sparse
    monkeypatch.undo()
    _check(ops, pos, rs, voxel, got, splits, pad=1, hyst=0.2)


def test_non_finite_positions_raise(batch):
    from dmcf_amd import ops, _lib
    pos, rs = batch
    bad = pos.clone()
    bad[rs[1], 0] = float("nan")
    with pytest.raises(_lib.DmcfError, match="not finite"):
        ops.grid_pos(bad, np.array([V, V, 0.0], dtype=np.float32), row_splits=rs)


def test_points_aabb_items(batch):
    from dmcf_amd import ops
    pos, rs = batch
    rs4 = rs + [rs[-1]]
    mn, mx = ops.points_aabb(pos, row_splits=rs4)
    assert mn.shape == (4, 3) and mx.shape == (4, 3)
    for b in range(3):
        a, c = ops.points_aabb(pos[rs[b]:rs[b + 1]].clone())
        assert torch.equal(mn[b], a) and torch.equal(mx[b], c)
    assert torch.equal(mn[3], torch.full((3,), 3.0e38, device="cuda"))
    assert torch.equal(mx[3], torch.full((3,), -3.0e38, device="cuda"))
    big = torch.rand(5000, 3, generator=torch.Generator().manual_seed(5)).cuda()  # more points than one pass of a block
    mn, mx = ops.points_aabb(big, row_splits=[0, 4999, 5000])
    a, c = ops.points_aabb(big[:4999].clone())
    assert torch.equal(mn[0], a) and torch.equal(mx[0], c)
    assert torch.equal(mn[1], big[4999]) and torch.equal(mx[1], big[4999])


def test_dilated_pos_with_row_splits(batch):
    from dmcf_amd.utils.tools import losses
    pos, rs = batch
    voxel = np.array([V, V, 0.0], dtype=np.float32)
    dil, pcnt, idx, level_rs = losses.get_dilated_pos(pos, [1, 2, 4], voxel_size=voxel, centralize=True, pad=1, row_splits=rs)
    assert dil[0] is pos and list(level_rs[0].host) == rs and idx == [None]
    assert pcnt == [d.shape[0] for d in dil]
    for k, s in ((1, 2), (2, 4)):
        for b in range(3):
            want = losses.grid_pos(pos[rs[b]:rs[b + 1]].clone(), voxel * np.float32(s), centralize=True, pad=1)
            h = level_rs[k].host
            assert torch.equal(dil[k][h[b]:h[b + 1]], want)
