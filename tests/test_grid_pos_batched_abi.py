"""CPU checks of grid_pos / points_aabb with row splits (ABI 2.21: dmcf_grid_pos_*_batched, dmcf_points_aabb_batched), of their
Python surface and of the batched model step's refusals: symbols, host-side validation, the errors raised before any launch,
and the host formulation of the batched lattice.  No device is touched."""
import ctypes
import os
import re

import numpy as np
import pytest

import batched_scene as scene

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["dmcf_grid_pos_workspace_bytes_batched", "dmcf_grid_pos_bounds_batched", "dmcf_grid_pos_count_batched",
       "dmcf_grid_pos_write_batched", "dmcf_points_aabb_batched"]
EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -4
FAKE = 1 << 20  # a non-NULL, 256-byte aligned device address: validation returns before anything could dereference it
V = scene.VOXEL


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
    assert hip_lib.dmcf_version() >= 22100


def test_signatures(hip_lib):
    """The argument lists of include/dmcf_hip.h, as the loader declares them: the un-batched phase with
    (row_splits, batch) after n_points, and the output row splits as count's last argument before the stream."""
    c = ctypes
    f3 = c.POINTER(c.c_float)
    L = hip_lib
    assert L.dmcf_grid_pos_workspace_bytes_batched.argtypes == [c.c_int64, c.c_int64]
    for phase, extra in (("bounds", []), ("count", [c.c_void_p]), ("write", [])):
        one = list(getattr(L, f"dmcf_grid_pos_{phase}").argtypes)
        many = list(getattr(L, f"dmcf_grid_pos_{phase}_batched").argtypes)
        assert many == one[:2] + [c.c_void_p, c.c_int64] + one[2:-1] + extra + [one[-1]], phase
        assert f3 in many
    assert L.dmcf_points_aabb_batched.argtypes == [c.c_void_p, c.c_int64, c.c_void_p, c.c_int64, c.c_void_p, c.c_void_p]


def test_workspace_bytes(hip_lib):
    L = hip_lib
    assert L.dmcf_grid_pos_workspace_bytes_batched(1000, 1) > 2 * 1000 * (4 + 8)  # a count and a row offset per candidate row
    assert L.dmcf_grid_pos_workspace_bytes_batched(1000, 16) > L.dmcf_grid_pos_workspace_bytes_batched(1000, 1)
    assert L.dmcf_grid_pos_workspace_bytes_batched(0, 3) > 0
    for bad in ((-1, 2), (5, 0), (5, -3)):
        assert L.dmcf_grid_pos_workspace_bytes_batched(*bad) == 0


def test_error_returns(hip_lib):
    L = hip_lib
    n, B = 100, 3
    nb = L.dmcf_grid_pos_workspace_bytes_batched(n, B)
    p = rs = ws = tab = out = ors = ctypes.c_void_p(FAKE)
    vs = (ctypes.c_float * 3)(0.1, 0.1, 0.1)
    bounds = lambda batch=B, rs_=rs, ws_=ws, nb_=nb, pad=0: L.dmcf_grid_pos_bounds_batched(  # noqa: E731
        p, n, rs_, batch, vs, 1, None, pad, 0.1, ws_, nb_, None)
    count = lambda batch=B, rs_=rs, ws_=ws, nb_=nb, cells=64, ors_=ors: L.dmcf_grid_pos_count_batched(  # noqa: E731
        p, n, rs_, batch, vs, 1, 0, 0.1, ws_, nb_, tab, cells, ors_, None)
    write = lambda batch=B, rs_=rs, ws_=ws, nb_=nb, out_=out, cap=10: L.dmcf_grid_pos_write_batched(  # noqa: E731
        p, n, rs_, batch, vs, 1, 0, 0.1, ws_, nb_, tab, 64, out_, cap, None)
    for call in (bounds, count, write):
        for batch in (0, -1):
            assert call(batch=batch) == EINVAL
        assert call(rs_=None) == EINVAL
        assert call(ws_=None) == EINVAL
        assert call(ws_=ctypes.c_void_p(FAKE + 8)) == EINVAL
        assert call(nb_=nb - 1) == EWORKSPACE
        assert call(nb_=1024) == EWORKSPACE
    assert bounds(pad=9) == EINVAL
    assert count(ors_=None) == EINVAL
    assert count(cells=-48) == EINVAL  # hashed: a power of two of slots
    assert write(out_=None) == EINVAL
    assert write(cap=-1) == EINVAL
    assert L.dmcf_points_aabb_batched(p, n, rs, 0, out, None) == EINVAL
    assert L.dmcf_points_aabb_batched(p, n, None, B, out, None) == EINVAL
    assert L.dmcf_points_aabb_batched(p, n, rs, B, None, None) == EINVAL
    assert L.dmcf_points_aabb_batched(None, n, rs, B, out, None) == EINVAL


P4 = torch.zeros(4, 3)
MALFORMED = [[1, 4], [0, 3], [0, 3, 2, 4], [4], [], [0, 1.5, 4]]


@pytest.mark.parametrize("bad", MALFORMED)
def test_malformed_row_splits_raise_before_the_device(bad):
    from dmcf_amd import ops
    from dmcf_amd.utils.tools import losses
    voxel = np.array([V, V, 0.0], dtype=np.float32)
    forms = [bad] + ([torch.tensor(bad, dtype=torch.int64)] if all(isinstance(v, int) for v in bad) else [])
    for rs in forms:
        with pytest.raises(ValueError):
            ops.grid_pos(P4, voxel, row_splits=rs)
        with pytest.raises(ValueError):
            ops.grid_pos_many(P4, [voxel, 2 * voxel], row_splits=rs)
        with pytest.raises(ValueError):
            ops.points_aabb(P4, row_splits=rs)
        with pytest.raises(ValueError):
            losses.grid_pos(P4, voxel, row_splits=rs)
        with pytest.raises(ValueError):
            losses.get_dilated_pos(P4, [1, 2], voxel_size=voxel, row_splits=rs)


def test_row_splits_types_and_options():
    from dmcf_amd import ops, _lib
    from dmcf_amd.utils.tools import losses
    voxel = np.array([V, V, 0.0], dtype=np.float32)
    with pytest.raises(TypeError):
        ops.grid_pos(P4, voxel, row_splits=torch.tensor([0, 4], dtype=torch.int32))
    with pytest.raises(ValueError):
        ops.grid_pos(P4, voxel, row_splits=torch.tensor([[0, 4]]))
    with pytest.raises(ValueError, match="center"):
        ops.grid_pos(P4, voxel, centralize=True, center=torch.zeros(3), row_splits=[0, 1, 4])
    with pytest.raises(NotImplementedError, match="return_box"):
        ops.grid_pos(P4, voxel, return_box=True, row_splits=[0, 4])
    with pytest.raises(NotImplementedError, match="return_box"):
        losses.grid_pos(P4, voxel, return_box=True, row_splits=[0, 4])
    # well-formed: on to the device check, as the un-batched call
    with pytest.raises(_lib.DmcfError):
        ops.grid_pos(P4, voxel, row_splits=[0, 1, 4])
    with pytest.raises(_lib.DmcfError):
        ops.points_aabb(P4, row_splits=[0, 1, 4])
    # both forms of row splits in one object: taken as they are
    rs = ops.RowSplits([0, 1, 4], torch.tensor([0, 1, 4]))
    assert ops._host_row_splits(rs, "row_splits") == ((0, 1, 4), rs.dev)


def test_fps_levels_with_row_splits_raise():
    from dmcf_amd.utils.tools import losses
    with pytest.raises(NotImplementedError, match="farthest"):
        losses.get_dilated_pos(P4, [1, 2], voxel_size=None, row_splits=[0, 2, 4])
    # (no coarse level: nothing to sample)
    dil, pcnt, idx, level_rs = losses.get_dilated_pos(P4, [1], voxel_size=None, row_splits=[0, 2, 4])
    assert dil[0] is P4 and pcnt == [4] and idx == [None] and list(level_rs[0].host) == [0, 2, 4]


@pytest.mark.parametrize("centralize", [False, True])
@pytest.mark.parametrize("pad", [0, 1])
def test_host_form_is_the_loop_over_the_items(centralize, pad):
    from dmcf_amd.utils.tools import losses
    items = scene.fluid_items() + [np.zeros((0, 3), dtype=np.float32)]
    pos, rs = scene.concat(items)
    pos = torch.from_numpy(pos)
    voxel = np.array([V, V, 0.0], dtype=np.float32)
    got, splits = losses.grid_pos(pos, voxel, centralize=centralize, pad=pad, row_splits=rs)
    host = [0]
    for b in range(4):
        item = pos[rs[b]:rs[b + 1]]
        want = losses.grid_pos(item, voxel, centralize=centralize, pad=pad) if item.shape[0] else pos.new_zeros((0, 3))
        host.append(host[-1] + want.shape[0])
        assert torch.equal(got[host[b]:host[b + 1]], want)
    assert list(splits.host) == host and splits.dev.tolist() == host and splits.dev.dtype == torch.int64
    assert host[4] == host[3] and got.shape[0] == host[-1]
    # every level of get_dilated_pos, with its row splits
    dil, pcnt, idx, level_rs = losses.get_dilated_pos(pos, [1, 2, 4], voxel_size=voxel, centralize=centralize, pad=pad, row_splits=rs)
    assert dil[0] is pos and list(level_rs[0].host) == rs and pcnt == [d.shape[0] for d in dil]
    for k, s in ((1, 2), (2, 4)):
        want, ws = losses.grid_pos(pos, voxel * np.float32(s), centralize=centralize, pad=pad, row_splits=rs)
        assert torch.equal(dil[k], want) and level_rs[k].host == ws.host
    # without row splits the call is the call it was: three results
    assert len(losses.get_dilated_pos(pos, [1, 2], voxel_size=voxel)) == 3


def _item():
    z = torch.zeros(4, 3)
    return [z, z, z, None, z, z]


def test_step_batched_refuses_before_any_launch():
    from dmcf_amd import models
    from tools import configs
    base = dict(configs.WATERRAMPS)
    for extra, what in ((dict(use_bnds=False), "use_bnds"), (dict(dens_feats=True), "dens_feats"),
                        (dict(pres_feats=True), "dens_feats"), (dict(dens_norm=True, window_dens="poly6"), "dens_feats"),
                        (dict(equivar=True), "equivar"), (dict(voxel_size=None), "farthest"), (dict(use_pre_adv=True), "use_pre_adv")):
        model = models.SymNet(**dict(base, **extra))
        with pytest.raises(NotImplementedError, match=what):
            model.step_batched([_item(), _item()])
    model = models.SymNet(**base)
    with pytest.raises(NotImplementedError, match="vel_corr"):
        model.step_batched([_item()], vel_corr=torch.zeros(4, 3))
    model.shard = object()
    with pytest.raises(NotImplementedError, match="sharded"):
        model.step_batched([_item()])
    for cfg in (configs.CCONV2D, configs.POINTNET2D):
        model = getattr(models, cfg["name"])(**cfg)
        with pytest.raises(NotImplementedError, match=cfg["name"]):
            model.step_batched([_item()])
    for cfg in (configs.WATERRAMPS, configs.WBC_SPH, configs.COLUMN_HRNET):  # the shipped 2-D configs pass the check
        getattr(models, cfg["name"])(**cfg)._check_batched_step()


class _NoModel:
    def requires_grad_(self, on):
        return self


def test_train_batched_defaults_to_off(tmp_path):
    """A pipeline built without the key takes the per-sample loop; with the key, the batched rows."""
    from dmcf_amd.pipelines.simulator import Simulator
    taken = []
    for kwargs, want in ((dict(), "looped"), (dict(train_batched=False), "looped"), (dict(train_batched=True), "batched")):
        sim = Simulator(_NoModel(), device="cuda", main_log_dir=str(tmp_path), **kwargs)
        assert bool(sim.cfg.get("train_batched", False)) is (want == "batched")
        sim.device = torch.device("cpu")  # (the rows below are stubs: nothing reaches a device)
        sim._window_rows = lambda *a: taken.append("looped") or [torch.ones(1)]
        sim._window_rows_batched = lambda *a: taken.append("batched") or [torch.ones(1)]
        loss = sim.window_loss(dict(pos=[None, None]), [1.0, 1.0], [], [], [])
        assert taken[-1] == want and float(loss) == 0.25
    with pytest.raises(NotImplementedError, match="iterations"):
        sim.window_loss(dict(pos=[None]), [1.0], [], [], [], it=2)
