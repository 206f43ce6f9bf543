"""CPU checks of the batched search (ABI 2.20: dmcf_frs_*_batched, dmcf_radius_search_*_batched) and of its Python surface:
symbols, host-side validation and the errors raised before any launch.  No device is touched."""
import ctypes
import os
import re

import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["dmcf_frs_workspace_bytes_batched", "dmcf_frs_build_batched", "dmcf_frs_count_batched", "dmcf_frs_write_batched",
       "dmcf_radius_search_count_batched", "dmcf_radius_search_write_batched"]
EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -4
FAKE = 1 << 20  # a non-NULL, 256-byte aligned device address: validation returns before anything could dereference it


@pytest.fixture(scope="module")
def hip_lib():
    from dmcf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_symbols_exported_declared_and_listed(hip_lib):
    from dmcf_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dmcf_hip.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", text), f"{name} not declared in dmcf_hip.h"
        assert name in _lib.SYMBOLS
        assert hasattr(hip_lib, name)


def test_version(hip_lib):
    assert hip_lib.dmcf_version() >= 22000


def test_workspace_bytes(hip_lib):
    L = hip_lib
    assert L.dmcf_frs_workspace_bytes_batched(1000, 500, 1) == L.dmcf_frs_workspace_bytes(1000, 500)
    assert L.dmcf_frs_workspace_bytes_batched(1000, 500, 16) >= L.dmcf_frs_workspace_bytes(1000, 500)
    # one cell per item at least: more items than the un-batched table has cells make the table grow
    assert L.dmcf_frs_workspace_bytes_batched(10, 10, 100000) > L.dmcf_frs_workspace_bytes(10, 10) + 2 * 4 * 90000
    for bad in ((-1, 5, 2), (5, -1, 2), (5, 5, 0), (5, 5, -3), (5, 5, (1 << 26) + 1)):
        assert L.dmcf_frs_workspace_bytes_batched(*bad) == 0


def test_host_validation(hip_lib):
    from dmcf_amd import ops
    L = hip_lib
    n = m = 100
    B = 3
    nb = L.dmcf_frs_workspace_bytes_batched(n, m, B)
    p = q = r = ws = rs = prs = idx = ctypes.c_void_p(FAKE)
    walks = (ops.FRS_OPEN3D_VOXEL_WALK, ops.FRS_OPEN3D_CORNER_VOXELS, ops.FRS_OPEN3D_VOXEL_WALK | ops.FRS_IGNORE_QUERY_POINT)
    # build: null row splits, batch < 1, null / misaligned / too small workspace, a radius that is not positive
    assert L.dmcf_frs_build_batched(p, n, None, B, 0.5, ws, nb, None) == EINVAL
    for batch in (0, -1, (1 << 26) + 1):
        assert L.dmcf_frs_build_batched(p, n, prs, batch, 0.5, ws, nb, None) == EINVAL
    assert L.dmcf_frs_build_batched(p, n, prs, B, 0.5, None, nb, None) == EINVAL
    assert L.dmcf_frs_build_batched(p, n, prs, B, 0.5, ctypes.c_void_p(FAKE + 8), nb, None) == EINVAL
    assert L.dmcf_frs_build_batched(p, n, prs, B, 0.0, ws, nb, None) == EINVAL
    assert L.dmcf_frs_build_batched(None, n, prs, B, 0.5, ws, nb, None) == EINVAL
    assert L.dmcf_frs_build_batched(p, n, prs, B, 0.5, ws, 1024, None) == EWORKSPACE
    # fixed radius: count and write
    assert L.dmcf_frs_count_batched(q, m, None, B, n, 0.5, 0, ws, nb, rs, None) == EINVAL
    assert L.dmcf_frs_write_batched(q, m, None, B, n, 0.5, 0, ws, nb, rs, idx, None, 10, None) == EINVAL
    for batch in (0, -1):
        assert L.dmcf_frs_count_batched(q, m, prs, batch, n, 0.5, 0, ws, nb, rs, None) == EINVAL
        assert L.dmcf_frs_write_batched(q, m, prs, batch, n, 0.5, 0, ws, nb, rs, idx, None, 10, None) == EINVAL
    for flag in walks:
        assert L.dmcf_frs_count_batched(q, m, prs, B, n, 0.5, flag, ws, nb, rs, None) == EINVAL
        assert L.dmcf_frs_write_batched(q, m, prs, B, n, 0.5, flag, ws, nb, rs, idx, None, 10, None) == EINVAL
    assert L.dmcf_frs_count_batched(q, m, prs, B, n, 0.5, ops.FRS_METRIC_LINF, ws, nb, rs, None) == EUNSUPPORTED
    assert L.dmcf_frs_write_batched(q, m, prs, B, n, 0.5, ops.FRS_METRIC_LINF, ws, nb, rs, idx, None, 10, None) == EUNSUPPORTED
    assert L.dmcf_frs_count_batched(q, m, prs, B, n, 0.5, 16, ws, nb, rs, None) == EINVAL  # an unknown bit
    assert L.dmcf_frs_count_batched(q, m, prs, B, n, 0.5, 0, None, nb, rs, None) == EINVAL
    assert L.dmcf_frs_count_batched(q, m, prs, B, n, 0.5, 0, ws, nb, None, None) == EINVAL
    assert L.dmcf_frs_count_batched(q, m, prs, B, n, 0.5, 0, ws, nb - 1, rs, None) == EWORKSPACE
    assert L.dmcf_frs_write_batched(q, m, prs, B, n, 0.5, 0, ws, nb - 1, rs, idx, None, 10, None) == EWORKSPACE
    assert L.dmcf_frs_write_batched(q, m, prs, B, n, 0.5, 0, ws, nb, rs, None, None, 10, None) == EINVAL
    assert L.dmcf_frs_write_batched(q, 0, prs, B, n, 0.5, 0, ws, nb, rs, None, None, 0, None) == 0  # no queries: nothing to do
    # a radius per query
    assert L.dmcf_radius_search_count_batched(q, m, None, B, n, r, 0.5, 0, ws, nb, rs, None) == EINVAL
    assert L.dmcf_radius_search_count_batched(q, m, prs, 0, n, r, 0.5, 0, ws, nb, rs, None) == EINVAL
    assert L.dmcf_radius_search_count_batched(q, m, prs, B, n, None, 0.5, 0, ws, nb, rs, None) == EINVAL
    assert L.dmcf_radius_search_count_batched(q, m, prs, B, n, r, float("nan"), 0, ws, nb, rs, None) == EINVAL
    assert L.dmcf_radius_search_count_batched(q, m, prs, B, n, r, 0.5, 0, ws, nb - 1, rs, None) == EWORKSPACE
    assert L.dmcf_radius_search_write_batched(q, m, None, B, n, r, 0.5, 0, ws, nb, rs, idx, None, 10, None) == EINVAL
    assert L.dmcf_radius_search_write_batched(q, m, prs, -2, n, r, 0.5, 0, ws, nb, rs, idx, None, 10, None) == EINVAL
    assert L.dmcf_radius_search_write_batched(q, m, prs, B, n, r, 0.5, 0, ws, nb - 1, rs, idx, None, 10, None) == EWORKSPACE
    for flag in walks + (ops.FRS_METRIC_LINF,):
        assert L.dmcf_radius_search_count_batched(q, m, prs, B, n, r, 0.5, flag, ws, nb, rs, None) == EINVAL
        assert L.dmcf_radius_search_write_batched(q, m, prs, B, n, r, 0.5, flag, ws, nb, rs, idx, None, 10, None) == EINVAL


P4 = torch.zeros(4, 3)
WHOLE = torch.tensor([0, 4])


def _searches():
    from dmcf_amd import ops
    frs = ops.FixedRadiusSearch(return_distances=True)
    rad = ops.RadiusSearch(return_distances=True, normalize_distances=True)
    r4 = torch.full((4,), 0.5)
    return [
        lambda **kw: ops.fixed_radius_search(P4, P4, 0.5, **kw),
        lambda **kw: frs(P4, P4, 0.5, **kw),
        lambda **kw: ops.radius_search(P4, P4, r4, **kw),
        lambda **kw: rad(P4, P4, r4, **kw),
    ]


def test_one_row_splits_argument_alone_is_not_implemented():
    for search in _searches():
        for kw in (dict(points_row_splits=WHOLE), dict(queries_row_splits=WHOLE), dict(points_row_splits=[0, 4])):
            with pytest.raises(NotImplementedError, match="needs both points_row_splits and queries_row_splits"):
                search(**kw)
    # (malformed, and alone: still the first check)
    from dmcf_amd import ops
    with pytest.raises(NotImplementedError):
        ops.fixed_radius_search(P4, P4, 0.5, points_row_splits=[3, 1])
    with pytest.raises(NotImplementedError):
        ops.radius_search(P4, P4, torch.full((4,), 0.5), queries_row_splits=[3, 1])


def test_options_without_a_batched_form(monkeypatch):
    from dmcf_amd import ops
    both = dict(points_row_splits=WHOLE, queries_row_splits=WHOLE)
    with pytest.raises(NotImplementedError, match="row_stride"):
        ops.fixed_radius_search(P4, P4, 0.5, row_stride=8, **both)
    with pytest.raises(NotImplementedError, match="row_stride"):
        ops.FixedRadiusSearch()(P4, P4, 0.5, row_stride=8, **both)
    with pytest.raises(NotImplementedError, match="Linf"):
        ops.fixed_radius_search(P4, P4, 0.5, return_distances=False, metric="Linf", **both)
    with pytest.raises(NotImplementedError, match="Linf"):
        ops.FixedRadiusSearch(metric="Linf")(P4, P4, 0.5, **both)
    for name in ("open3d", "open3d_corners"):
        monkeypatch.setenv("DMCF_FRS_SET", name)
        with pytest.raises(NotImplementedError, match="DMCF_FRS_SET"):
            ops.fixed_radius_search(P4, P4, 0.5, **both)
        with pytest.raises(NotImplementedError, match="DMCF_FRS_SET"):
            ops.FixedRadiusSearch()(P4, P4, 0.5, **both)
    monkeypatch.delenv("DMCF_FRS_SET")
    # with nothing in the way the call reaches the device check, as the un-batched call does
    from dmcf_amd import _lib
    with pytest.raises(_lib.DmcfError):
        ops.fixed_radius_search(P4, P4, 0.5, **both)


MALFORMED = [
    ([1, 4], [0, 4]),            # does not start at 0
    ([0, 4], [2, 4]),
    ([0, 3, 2, 4], [0, 1, 2, 4]),  # decreases
    ([0, 1, 2, 4], [0, 3, 2, 4]),
    ([0, 3], [0, 4]),            # does not end at n / m
    ([0, 4], [0, 5]),
    ([0, 2, 4], [0, 4]),         # lengths differ
    ([0, 4], [0, 1, 4]),
    ([4], [4]),                  # fewer than 2 entries
    ([], []),
]


@pytest.mark.parametrize("prs,qrs", MALFORMED)
def test_malformed_row_splits(prs, qrs):
    forms = [(prs, qrs), (torch.tensor(prs, dtype=torch.int64), torch.tensor(qrs, dtype=torch.int64))]
    for search in _searches():
        for a, b in forms:
            with pytest.raises(ValueError):
                search(points_row_splits=a, queries_row_splits=b)


def test_row_splits_types():
    from dmcf_amd import ops
    with pytest.raises(TypeError):
        ops.fixed_radius_search(P4, P4, 0.5, points_row_splits=torch.tensor([0, 4], dtype=torch.int32), queries_row_splits=WHOLE)
    with pytest.raises(ValueError):
        ops.fixed_radius_search(P4, P4, 0.5, points_row_splits=torch.tensor([[0, 4]]), queries_row_splits=WHOLE)
    with pytest.raises(ValueError):
        ops.fixed_radius_search(P4, P4, 0.5, points_row_splits=[0, 1.5, 4], queries_row_splits=[0, 1, 4])


def test_hash_table_validates_its_row_splits_before_the_device():
    from dmcf_amd import ops, _lib
    for bad in ([1, 4], [0, 3], [0, 3, 2, 4], [4]):
        with pytest.raises(ValueError):
            ops.build_spatial_hash_table(P4, 0.5, points_row_splits=bad)
    with pytest.raises(_lib.DmcfError):  # well-formed: on to the device check
        ops.build_spatial_hash_table(P4, 0.5, points_row_splits=[0, 1, 4])


def test_layer_errors_before_the_device():
    from dmcf_amd.utils.convolutions import ContinuousConv
    conv = ContinuousConv(filters=4, kernel_size=[4, 4, 4], device="cpu")
    x, pos = torch.zeros(4, 2), torch.zeros(4, 3)
    with pytest.raises(NotImplementedError, match="needs both"):
        conv(x, pos, pos, 0.5, inp_positions_row_splits=[0, 4])
    with pytest.raises(NotImplementedError, match="needs both"):
        conv(x, pos, pos, 0.5, out_positions_row_splits=[0, 4])
    with pytest.raises(ValueError):
        conv(x, pos, pos, 0.5, inp_positions_row_splits=[0, 3], out_positions_row_splits=[0, 4])
    with pytest.raises(ValueError):  # a user list and row splits
        conv(x, pos, pos, 0.5, inp_positions_row_splits=[0, 4], out_positions_row_splits=[0, 4],
             user_neighbors_index=torch.zeros(0, dtype=torch.int32), user_neighbors_row_splits=torch.zeros(5, dtype=torch.int64))
    ascc = ContinuousConv(filters=3, kernel_size=[4, 4, 4], symmetric=True, normalize=False, device="cpu")
    with pytest.raises(NotImplementedError, match="symmetric"):
        ascc(x, pos, pos, 0.5, inp_positions_row_splits=[0, 4], out_positions_row_splits=[0, 4])
