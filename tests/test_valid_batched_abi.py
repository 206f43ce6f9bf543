"""CPU checks of the batched validation: the ragged nearest-neighbour entry point (ABI 2.23: dmcf_nn_distance_ragged), its
Python surface (ops.nn_distance and evaluation_helper.chamfer_distance with row splits), the pipeline key ``valid_batched``,
Simulator.run_rollout_batched on a host stub and the host bookkeeping of which scenes have a frame t.  No device is touched."""
import ctypes
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["dmcf_nn_distance_ragged_workspace_bytes", "dmcf_nn_distance_ragged"]
OK, EINVAL, EWORKSPACE = 0, -1, -2
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
    assert hip_lib.dmcf_version() >= 22300


def _i64(values):
    return (ctypes.c_int64 * len(values))(*values)


def test_workspace_bytes(hip_lib):
    ws = hip_lib.dmcf_nn_distance_ragged_workspace_bytes
    assert ws(-1, 4, 1) == 0 and ws(4, -1, 1) == 0 and ws(4, 4, 0) == 0 and ws(4, 4, -1) == 0 and ws(4, 4, (1 << 26) + 1) == 0
    # one 16-byte record per tile of 64 rows; every item adds at most one partial tile to each direction
    for n, m, b in ((1, 1, 1), (64, 64, 1), (1000, 30, 7), (2025 * 16, 2025 * 16, 16)):
        assert ws(n, m, b) >= 16 * (n // 64 + m // 64 + 2 * b)
        assert ws(n, m, b) % 256 == 0


def test_error_returns(hip_lib):
    L = hip_lib
    rs1, rs2 = [0, 70, 70, 100], [0, 5, 5, 80]
    n, m, B = rs1[-1], rs2[-1], 3
    nb = L.dmcf_nn_distance_ragged_workspace_bytes(n, m, B)
    assert nb > 0
    p = ctypes.c_void_p(FAKE)

    def call(n_=n, m_=m, rs1_=rs1, rs2_=rs2, batch=B, x1=p, x2=p, d1=p, i1=p, d2=p, i2=p, ws=p, nb_=nb):
        return L.dmcf_nn_distance_ragged(x1, n_, None if rs1_ is None else _i64(rs1_), x2, m_, None if rs2_ is None else _i64(rs2_),
                                         batch, d1, i1, d2, i2, ws, nb_, None)

    assert call(batch=-1) == EINVAL
    assert call(batch=(1 << 26) + 1) == EINVAL
    assert call(rs1_=None) == EINVAL and call(rs2_=None) == EINVAL
    assert call(d1=None, i1=None, d2=None, i2=None) == EINVAL  # both directions left out
    assert call(i1=None) == EINVAL and call(d1=None) == EINVAL and call(i2=None) == EINVAL and call(d2=None) == EINVAL
    assert call(n_=-1) == EINVAL and call(m_=-1) == EINVAL
    assert call(n_=(1 << 31) - 200) == EINVAL  # (int32 indices)
    # row splits are read and validated on the host: they start at 0, do not decrease, end at the row count
    assert call(rs1_=[1, 70, 70, 100]) == EINVAL
    assert call(rs1_=[0, 70, 60, 100]) == EINVAL
    assert call(rs1_=[0, 70, 70, 99]) == EINVAL and call(rs2_=[0, 5, 5, 81]) == EINVAL
    # an item with exactly one empty set has no nearest neighbour
    assert call(rs1_=[0, 70, 71, 100]) == EINVAL and call(rs2_=[0, 5, 6, 80]) == EINVAL
    assert call(rs1_=[0, 0, 70, 100]) == EINVAL
    assert call(x1=None) == EINVAL and call(x2=None) == EINVAL and call(ws=None) == EINVAL
    assert call(nb_=nb - 1) == EWORKSPACE and call(nb_=0) == EWORKSPACE
    # each one-direction form passes validation too: it goes on to the workspace check
    assert call(d1=None, i1=None, nb_=nb - 1) == EWORKSPACE and call(d2=None, i2=None, nb_=nb - 1) == EWORKSPACE
    # nothing to do: DMCF_OK with nothing enqueued (no device here to launch on)
    assert call(n_=0, m_=0, rs1_=[0, 0, 0, 0], rs2_=[0, 0, 0, 0], x1=None, x2=None, ws=None, nb_=0) == OK
    assert call(n_=0, m_=0, rs1_=None, rs2_=None, batch=0, x1=None, x2=None, ws=None, nb_=0) == OK
    assert call(batch=0, rs1_=None, rs2_=None) == EINVAL  # rows without an item


A5 = torch.zeros(5, 3)
B7 = torch.zeros(7, 3)
MALFORMED = [[1, 5], [0, 4], [0, 3, 2, 5], [5], [], [0, 1.5, 5]]  # (the list of tests/test_grid_pos_batched_abi.py)


def test_one_split_alone_raises():
    from dmcf_amd import ops
    from dmcf_amd.utils import evaluation_helper as eh
    from dmcf_amd.utils.tools import nn_distance as tool
    assert tool.nn_distance is ops.nn_distance
    for kw in (dict(row_splits1=[0, 5]), dict(row_splits2=[0, 7])):
        with pytest.raises(NotImplementedError, match="both"):
            ops.nn_distance(A5, B7, **kw)
    for kw in (dict(pred_row_splits=[0, 5]), dict(gt_row_splits=[0, 7])):
        with pytest.raises(NotImplementedError, match="both"):
            eh.chamfer_distance(A5, B7, **kw)
        with pytest.raises(NotImplementedError, match="both"):
            eh.chamfer_distance(A5.numpy(), B7.numpy(), **kw)


@pytest.mark.parametrize("bad", MALFORMED)
def test_malformed_row_splits_raise_before_the_device(bad):
    from dmcf_amd import ops
    from dmcf_amd.utils import evaluation_helper as eh
    forms = [bad] + ([torch.tensor(bad, dtype=torch.int64)] if all(isinstance(v, int) for v in bad) else [])
    for rs in forms:
        with pytest.raises(ValueError):
            ops.nn_distance(A5, B7, rs, [0, 2, 7])
        with pytest.raises(ValueError):
            ops.nn_distance(B7, A5, [0, 2, 7], rs)
        with pytest.raises(ValueError):
            eh.chamfer_distance(A5, B7, pred_row_splits=rs, gt_row_splits=[0, 2, 7])
        with pytest.raises(ValueError):
            eh.chamfer_distance(B7, A5, pred_row_splits=[0, 2, 7], gt_row_splits=rs)


def test_row_splits_types_batch_sizes_and_empty_sets():
    from dmcf_amd import ops, _lib
    from dmcf_amd.utils import evaluation_helper as eh
    with pytest.raises(TypeError):
        ops.nn_distance(A5, B7, torch.tensor([0, 5], dtype=torch.int32), [0, 7])
    with pytest.raises(ValueError, match="equal lengths"):
        ops.nn_distance(A5, B7, [0, 2, 5], [0, 7])
    with pytest.raises(ValueError, match="equal lengths"):
        eh.chamfer_distance(A5, B7, pred_row_splits=[0, 5], gt_row_splits=[0, 3, 7])
    # an item with exactly one empty set: the dense form rejects n == 0 or m == 0 too
    for rs1, rs2 in (([0, 2, 2, 5], [0, 3, 4, 7]), ([0, 2, 4, 5], [0, 3, 3, 7]), ([0, 0, 5], [0, 1, 7])):
        with pytest.raises(ValueError, match="non-empty"):
            ops.nn_distance(A5, B7, rs1, rs2)
        with pytest.raises(ValueError, match="non-empty"):
            eh.chamfer_distance(B7, A5, pred_row_splits=rs2, gt_row_splits=rs1)
    # the ragged form takes [n_total, 3] point sets
    with pytest.raises(ValueError, match="n_total"):
        ops.nn_distance(A5.unsqueeze(0), B7.unsqueeze(0), [0, 5], [0, 7])
    # no gradient
    with pytest.raises(NotImplementedError, match="backward"):
        ops.nn_distance(A5.clone().requires_grad_(True), B7, [0, 5], [0, 7])
    with pytest.raises(NotImplementedError, match="backward"):
        ops.nn_distance(A5, B7.clone().requires_grad_(True), [0, 2, 5], [0, 3, 7])
    with torch.no_grad(), pytest.raises(_lib.DmcfError):  # (under no_grad the call goes on to the device check)
        ops.nn_distance(A5.clone().requires_grad_(True), B7, [0, 5], [0, 7])
    # well-formed, an item with both sets empty included, in every form the splits may take: on to the device check
    for rs1, rs2 in (([0, 2, 2, 5], [0, 3, 3, 7]), (torch.tensor([0, 2, 5]), (0, 3, 7)), (ops.RowSplits([0, 5], None), np.array([0, 7]))):
        with pytest.raises(_lib.DmcfError, match="GPU only"):
            ops.nn_distance(A5, B7, rs1, rs2)


def test_the_unbatched_call_is_unchanged():
    """Without row splits: the dense form's own checks, in their order."""
    import inspect
    from dmcf_amd import ops, _lib
    assert list(inspect.signature(ops.nn_distance).parameters) == ["xyz1", "xyz2", "row_splits1", "row_splits2"]
    with pytest.raises(_lib.DmcfError, match="GPU only"):
        ops.nn_distance(A5, B7)
    with pytest.raises(_lib.DmcfError, match="GPU only"):
        ops.nn_distance(A5, B7, None, None)
    with pytest.raises(TypeError):
        ops.nn_distance(A5.numpy(), B7)


# ---- the pipeline key and the refusals ---------------------------------------------------------------------------------------
class _Counting:
    """The library with a counter on every entry point called (the pattern of tests/test_gpu_step_batched.py)."""

    def __init__(self, real):
        self._real, self.calls = real, {}

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("dmcf_"):
            return fn

        def counted(*a):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*a)
        return counted


def _scene(n, frames, drift, seed):
    rng = np.random.default_rng(seed)
    p0 = (rng.integers(0, 64, size=(n, 3)) / 8.0).astype(np.float32)
    step = np.array([drift, 0.0, drift], dtype=np.float32)
    return dict(pos=np.stack([p0 + np.float32(t) * step for t in range(frames)]),
                vel=np.broadcast_to(step, (frames, n, 3)).astype(np.float32).copy(), grav=[None] * frames,
                box=np.zeros((frames, 2, 3), dtype=np.float32), box_normals=np.zeros((frames, 2, 3), dtype=np.float32))


def test_valid_batched_defaults_to_off(tmp_path, monkeypatch):
    """A pipeline built without the key validates scene after scene -- with the other batched keys set too."""
    from dmcf_amd import datasets
    from dmcf_amd.pipelines.simulator import Simulator
    import types
    data = [_scene(3, 2, 0.5, 0)]
    monkeypatch.setattr(datasets, "get_rollout", lambda *a, **k: data)
    for kwargs, want in ((dict(), "looped"), (dict(train_batched=True, warm_up_batched=True), "looped"),
                         (dict(valid_batched=False), "looped"), (dict(valid_batched=True), "batched")):
        sim = Simulator(_Drift(), dataset=types.SimpleNamespace(valid=None), device="cuda", main_log_dir=str(tmp_path), **kwargs)
        assert bool(sim.cfg.get("valid_batched", False)) is (want == "batched")
        taken = []

        class Stop(Exception):
            pass

        def rollout(name):
            def run(*a):
                taken.append(name)
                raise Stop()
            return run
        sim.run_rollout, sim.run_rollout_batched = rollout("looped"), rollout("batched")
        with pytest.raises(Stop):
            sim.run_valid(epoch=0)
        assert taken == [want]


def test_a_model_without_a_batched_step_is_refused_before_any_launch(tmp_path, monkeypatch):
    from dmcf_amd import _lib, models
    from dmcf_amd.pipelines.simulator import Simulator
    from tools import configs
    counting = _Counting(_lib.lib())
    monkeypatch.setattr(_lib, "lib", lambda: counting)
    data = [_scene(3, 3, 0.5, 0), _scene(4, 3, 0.25, 1)]
    for cfg in (configs.CCONV2D, configs.POINTNET2D):
        model = getattr(models, cfg["name"])(**cfg)
        sim = Simulator(model, device="cuda", main_log_dir=str(tmp_path / cfg["name"]), valid_batched=True)
        sim.device = torch.device("cpu")  # (nothing may reach a device: the refusal comes first)
        with pytest.raises(NotImplementedError, match=cfg["name"]):
            sim.run_rollout_batched(data, 3)
        with pytest.raises(NotImplementedError, match=cfg["name"]):
            sim.run_valid(epoch=0)  # (before the split is read: this simulator has no dataset at all)
        assert not os.path.exists(sim.cfg.logs_dir)
    assert counting.calls == {}

    class _NoStep:
        pass
    sim = Simulator(_NoStep(), device="cuda", main_log_dir=str(tmp_path), valid_batched=True)
    with pytest.raises(NotImplementedError, match="_NoStep"):
        sim.run_rollout_batched(data, 3)


class _Drift:
    """A model on CPU tensors whose step moves every particle by the velocity it carries (the stub of
    tests/test_window_sum_batched_abi.py): ``__call__`` is the per-scene step, ``step_batched`` the same for a list of items."""

    def __init__(self):
        self.batches, self.calls = [], 0

    def __call__(self, inputs, training=False):
        self.calls += 1
        return inputs[0] + inputs[1], inputs[1]

    def step_batched(self, items, training=False):
        self.batches.append(len(items))
        rs = [0]
        for it in items:
            rs.append(rs[-1] + it[0].shape[0])
        pos, vel = torch.cat([it[0] for it in items]), torch.cat([it[1] for it in items])
        return pos + vel, vel, rs


def test_run_rollout_batched_on_the_host(tmp_path, monkeypatch, caplog):
    """On CPU tensors with a stub model: the structure of run_rollout, one batched step per time step, bit for bit."""
    import logging
    from dmcf_amd.pipelines.simulator import Simulator
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    data = [_scene(3, 5, 0.5, 0), _scene(1, 5, 0.125, 1), _scene(6, 5, 0.25, 2)]
    model = _Drift()
    sim = Simulator(model, device="cuda", main_log_dir=str(tmp_path))
    sim.device = torch.device("cpu")
    want = sim.run_rollout(data, 4)
    assert model.batches == [] and model.calls == 1 + 3 * 3 and len(sim.timing) == 3
    model.calls = 0
    with caplog.at_level(logging.INFO, logger="dmcf_amd.pipelines.simulator"):
        got = sim.run_rollout_batched(data, 4)
    assert model.batches == [3, 3, 3] and model.calls == 1  # (the "dummy init" on the first scene, as in run_rollout)
    assert len(sim.timing) == 3 and "Average runtime" in caplog.text
    assert len(got) == len(want) == 3
    for i in range(3):
        assert len(got[i]) == len(want[i]) == 4
        for t in range(4):
            assert len(got[i][t]) == len(want[i][t]) == 6 and got[i][t][3] is None and got[i][t][2] is None
            for k in (0, 1, 4, 5):
                assert torch.equal(got[i][t][k], want[i][t][k]), (i, t, k)
            assert got[i][t][4] is got[i][0][4] and got[i][t][5] is got[i][0][5]  # the boxes are carried through
            assert torch.equal(got[i][t][0], torch.from_numpy(data[i]["pos"][t]))


# ---- which scenes have a frame t ---------------------------------------------------------------------------------------------
def test_valid_frames_restates_the_loop():
    from dmcf_amd.pipelines.simulator import valid_frames

    def loop(lengths, eval_stride):  # run_valid's scene and frame loops, their (scene, frame) pairs only
        pairs = []
        for i, length in enumerate(lengths):
            for t in range(1, length):
                if t % eval_stride != 0:
                    continue
                pairs.append((i, t))
        return pairs

    assert valid_frames([3, 3]) == [(1, [0, 1]), (2, [0, 1])]
    assert valid_frames([5, 2, 4], 1) == [(1, [0, 1, 2]), (2, [0, 2]), (3, [0, 2]), (4, [0])]
    assert valid_frames([5, 2, 4], 2) == [(2, [0, 2]), (4, [0])]
    assert valid_frames([7, 1, 0, 7], 3) == [(3, [0, 3]), (6, [0, 3])]
    assert valid_frames([], 1) == [] and valid_frames([1, 1]) == [] and valid_frames([3], 5) == []
    with pytest.raises(ValueError):
        valid_frames([3], 0)
    rng = np.random.default_rng(5)
    for _ in range(200):
        lengths = rng.integers(0, 9, size=int(rng.integers(0, 6))).tolist()
        stride = int(rng.integers(1, 5))
        frames = valid_frames(lengths, stride)
        assert [t for t, _ in frames] == sorted({t for t, _ in frames}) and all(scenes for _, scenes in frames)
        assert sorted((i, t) for t, scenes in frames for i in scenes) == sorted(loop(lengths, stride))
