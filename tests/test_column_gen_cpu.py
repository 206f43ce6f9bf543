"""CPU checks of the generated datasets: the numpy restatement of the 1-D SPH step (tests/sph1d_ref.py) against the reference's
scenes (tests/golden/column_gen.npz) under the bar of tests/column_gen_bar.py, the host side of dmcf_amd/datasets/column_gen.py
(draws, frame dicts), free_fall_gen, DatasetGroup's generation branch with its cache, and the ABI of dmcf_sph1d_rollout
(ABI 2.17).  No device is touched: where DatasetGroup has to run the column solver, the restatement stands in for the kernel."""
import ctypes
import os
import re

import numpy as np
import pytest

import column_gen_bar as bar
import sph1d_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
FAKE = 1 << 20  # a non-NULL device address: validation returns before anything could dereference it


def _draw(name):
    from dmcf_amd.datasets import column_gen
    seed, sec = bar.CASES[name]
    np.random.seed(seed)
    return column_gen.draw_states(**{k: v for k, v in sec.items() if k != "timesteps"})


def _constants():
    from dmcf_amd.datasets import column_gen
    return column_gen.solver_constants(gravity=bar.DATASET["gravity"] * bar.DATASET["res"], dt=bar.DATASET["dt"])


def _ref_rollout(states, timesteps, **constants):
    """column_gen.rollout's contract on the host."""
    runs = [sph1d_ref.rollout(s, timesteps, **constants) for s in states]
    return [r[0] for r in runs], [r[2] for r in runs]


@pytest.mark.parametrize("name", sorted(bar.CASES))
def test_restatement_meets_the_bar(name):
    from dmcf_amd.datasets import column_gen
    fx = bar.fixture()
    _, states = _draw(name)
    seqs, iters = _ref_rollout(states, bar.CASES[name][1]["timesteps"], **_constants())
    assert len(states) == int(fx[f"{name}_scenes"])
    for s, seq in enumerate(seqs):
        scene = column_gen.gen_dict(np.ascontiguousarray(seq[:, ::-1]), s, bar.DATASET["res"], 2, -1000.0)
        bar.check_scene(name, s, np.stack([f["pos"] for f in scene]), np.stack([f["vel"] for f in scene]))
        ref = fx[f"{name}_s{s}_iters"]
        print(f"case {name} scene {s}: iterations sum {iters[s].sum()} (reference {ref.sum()})")
        assert iters[s].min() >= 1 and iters[s].max() <= 10000


@pytest.mark.parametrize("name", sorted(bar.CASES))
def test_draws_match_the_reference_bit_for_bit(name):
    """Same seed, same draws in the same order: the point counts and frame 0 of every scene are the reference's bits."""
    from dmcf_amd.datasets import column_gen
    fx = bar.fixture()
    counts, states = _draw(name)
    assert len(states) == int(fx[f"{name}_scenes"])
    for s, st in enumerate(states):
        assert st.dtype == np.float32 and st.shape == (int(counts[s]) + 2, 3)
        assert int(counts[s]) == fx[f"{name}_s{s}_pos"].shape[1]
        frame = column_gen.gen_dict(st[None, ::-1, :2].copy(), s, bar.DATASET["res"], 2, -1000.0)[0]
        for k in ("pos", "vel", "box", "box_normals"):
            ref = fx[f"{name}_s{s}_{k}"]
            np.testing.assert_array_equal(frame[k], ref[0] if k in ("pos", "vel") else ref)
        np.testing.assert_array_equal(frame["grav"].astype(np.float32), fx[f"{name}_s{s}_grav"][0])


def test_draw_paths():
    from dmcf_amd.datasets import column_gen
    np.random.seed(3)
    counts, states = column_gen.draw_states(5, min_pts=2, max_pts=9)  # choice without replacement, sorted
    assert list(counts) == sorted(set(counts)) and len(states) == 5 and all(2 <= c <= 9 for c in counts)
    np.testing.assert_array_equal(states[0][:, 0], np.arange(counts[0] + 2, dtype=np.float32) * 0.5)
    with pytest.raises(NotImplementedError):
        column_gen.draw_states(9, min_pts=1, max_pts=8)
    c = column_gen.solver_constants()
    assert c == dict(h=1.0, rest_dens=2.0, stiffness=20.0, visc=0.1, gravity=-10.0, dt=0.01, eps=0.01, max_iter=10000, bcnt=2)


def test_gen_dict_keys_dtypes_and_shapes():
    from dmcf_amd.datasets import column_gen
    data = np.arange(2 * 6 * 2, dtype=np.float32).reshape(2, 6, 2)  # 4 fluid points, 2 boundary points (last)
    frames = column_gen.gen_dict(data.copy(), 7, 100, 2, -1000.0)
    assert len(frames) == 2
    f = frames[1]
    assert list(f) == ["frame_id", "scene_id", "grav", "pos", "vel", "box", "box_normals"]
    assert f["frame_id"] == 1 and f["scene_id"] == "sim_0007"
    assert f["grav"].dtype == np.float64 and f["grav"].tolist() == [0.0, -10.0, 0.0]
    for k, shape in (("pos", (4, 3)), ("vel", (4, 3)), ("box", (2, 3)), ("box_normals", (2, 3))):
        assert f[k].dtype == np.float32 and f[k].shape == shape, k
    np.testing.assert_array_equal(f["pos"][:, 1], data[1, :4, 0] / np.float32(100))
    np.testing.assert_array_equal(f["vel"][:, 1], data[1, :4, 1] / np.float32(100))
    np.testing.assert_array_equal(f["box"][:, 1], data[1, 4:, 0] / np.float32(100))
    assert not f["pos"][:, [0, 2]].any() and f["box_normals"].tolist() == [[0, 1, 0]] * 2
    # width: every point repeated across x, 0.5 apart about 0 (pos and box become float64, as in the reference)
    w = column_gen.gen_dict(data.copy(), 0, 100, 2, -1000.0, width=3)[0]
    assert w["pos"].shape == (12, 3) and w["vel"].shape == (12, 3) and w["box"].shape == (6, 3) and w["box_normals"].shape == (6, 3)
    assert w["pos"].dtype == np.float64 and w["box"].dtype == np.float64 and w["vel"].dtype == np.float32
    np.testing.assert_allclose(w["pos"][:3, 0] * 100, [-0.5, 0.0, 0.5])
    np.testing.assert_array_equal(w["pos"][:3, 1], w["pos"][0, 1])
    # side walls: four columns of 50 points outside the column, normals pointing inwards
    sw = column_gen.gen_dict(data.copy(), 0, 100, 2, -1000.0, width=3, side_walls=True)[0]
    assert sw["box"].shape == (6 + 200, 3) and sw["box_normals"].shape == (206, 3) and sw["pos"].shape == (12, 3)
    np.testing.assert_allclose(sorted(set(np.round(sw["box"][6:, 0] * 100, 6))), [-1.5, -1.0, 1.0, 1.5])
    assert (sw["box_normals"][6:106, 0] == 1).all() and (sw["box_normals"][106:, 0] == -1).all()
    np.testing.assert_allclose(sw["box"][6:56, 1] * 100, np.arange(50) * 0.5)
    # side_walls without width > 1 changes nothing (the reference's nesting)
    assert column_gen.gen_dict(data.copy(), 0, 100, 2, -1000.0, side_walls=True)[0]["box"].shape == (2, 3)


@pytest.mark.parametrize("mode", [0, 1])
def test_free_fall_closed_form(mode):
    from dmcf_amd.datasets import free_fall_gen
    T, res, dt, g = 6, 20, 0.01, -10.0
    data = free_fall_gen.gen_data(data_cnt=2, timesteps=T, res=res, radius=4, dt=dt, gravity=g, mode=mode)
    assert len(data) == 2 and len(data[0]) == T + 1
    p0 = data[0][0]["pos"] * res
    rg = np.linspace(0.5, res - 0.5, int((res - 2) * 0.5))
    inside = [(x, y) for x in rg for y in rg if np.hypot(x - res / 2, y - res / 2) < 4]
    assert len(inside) > 4
    np.testing.assert_allclose(p0, [[x, y, 0.0] for x, y in inside], rtol=0, atol=1e-12)
    G = g * res
    for t, f in enumerate(data[1]):
        assert list(f) == ["frame_id", "scene_id", "grav", "pos", "vel", "box", "box_normals"]
        assert f["frame_id"] == t and f["scene_id"] == "sim_0001" and f["pos"].dtype == np.float64
        np.testing.assert_allclose(f["grav"], [0.0, g, 0.0])
        np.testing.assert_allclose(f["box"], [[2.0, 2.0, 2.0]])
        assert f["box_normals"].shape == (1, 3) and not f["box_normals"].any()
        vy = G * dt * t  # v_t = g dt t
        if mode == 0:  # x_t = x_0 + dt sum_{k<=t} v_k = x_0 + g dt^2 t (t + 1) / 2
            dy = G * dt * dt * t * (t + 1) / 2
        else:  # as written: x_{k+1} = x_k + dt v_k + (v_k + v_{k+1}) / 2  ->  x_0 + g dt^2 t (t - 1) / 2 + g dt t^2 / 2
            dy = G * dt * dt * t * (t - 1) / 2 + G * dt * t * t / 2
        np.testing.assert_allclose(f["vel"] * res, np.broadcast_to([0.0, vy, 0.0], p0.shape), rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(f["pos"] * res, p0 + [0.0, dy, 0.0], rtol=1e-12, atol=1e-9)
    assert free_fall_gen.gen_data(timesteps=1, res=12, dim=3, radius=3)[0][0]["pos"][:, 2].any()


def test_dataset_group_cache_write_hit_regen(tmp_path, monkeypatch):
    from dmcf_amd.datasets import DatasetGroup, free_fall_gen
    calls = []
    real = free_fall_gen.gen_data
    monkeypatch.setattr(free_fall_gen, "gen_data", lambda **kw: calls.append(kw) or real(**kw))
    cfg = dict(name="ff", type="free_fall", res=16, dt=0.01, cache_dir=str(tmp_path / "cache"),
               test=dict(seed=5, data_cnt=1, timesteps=3, radius=3), valid=dict(data_cnt=1, timesteps=2, radius=3))
    g = DatasetGroup(**cfg, split="test")
    assert len(calls) == 1 and calls[0] == dict(data_cnt=1, timesteps=3, radius=3, res=16, dt=0.01)  # seed and type are not passed on
    assert g.train is None and g.valid is g.test and len(g.test) == 1 and len(g.test[0]) == 4
    entries = os.listdir(tmp_path / "cache")
    assert len(entries) == 1 and os.listdir(tmp_path / "cache" / entries[0]) == ["data.msgpack.zst"]
    hit = DatasetGroup(**cfg, split="test")
    assert len(calls) == 1  # read from the cache
    for f, h in zip(g.test[0], hit.test[0]):
        assert list(f) == list(h) and f["frame_id"] == h["frame_id"] and f["scene_id"] == h["scene_id"]
        for k in ("pos", "vel", "grav", "box", "box_normals"):
            assert f[k].dtype == h[k].dtype
            np.testing.assert_array_equal(f[k], h[k])
    DatasetGroup(**cfg, split="test", regen=True)
    assert len(calls) == 2 and os.listdir(tmp_path / "cache") == entries  # generated again, stored again
    DatasetGroup(**dict(cfg, test=dict(cfg["test"], timesteps=4)), split="test")
    assert len(calls) == 3 and len(os.listdir(tmp_path / "cache")) == 2  # another section, another entry
    # a section without a seed is generated every time and never cached
    v = DatasetGroup(**cfg, split="valid")
    DatasetGroup(**cfg, split="valid")
    assert len(calls) == 5 and v.test is None and len(v.valid[0]) == 3 and len(os.listdir(tmp_path / "cache")) == 2


def test_dataset_group_generates_column_splits(tmp_path, monkeypatch):
    """type: column through DatasetGroup with the restatement in the kernel's place: seeded per section, the splits asked for."""
    from dmcf_amd.datasets import DatasetGroup, column_gen
    monkeypatch.setattr(column_gen, "rollout", _ref_rollout)
    sec = dict(seed=44, offset=10.0, pts_cnt=[1, 5], data_cnt=2, timesteps=3)
    cfg = dict(name="Column2", type="column", **bar.DATASET, cache_dir=str(tmp_path / "cache"), train=dict(sec, seed=1),
               valid=dict(sec, seed=2, timesteps=2), test=sec)
    fx = bar.fixture()
    g = DatasetGroup(**cfg, split="test")
    assert g.name == "Column2" and g.train is None and g.valid is g.test and len(g.test) == 2
    for s in (0, 1):
        for t in range(3):
            np.testing.assert_array_equal(g.test[s][t]["pos"], fx[f"a_s{s}_pos"][t])  # (free flight: the same bits)
            np.testing.assert_array_equal(g.test[s][t]["vel"], fx[f"a_s{s}_vel"][t])
    g = DatasetGroup(**cfg, split="train")
    assert [len(d) for d in (g.train, g.valid, g.test)] == [2, 2, 2] and len(g.valid[0]) == 2 and len(g.train[1]) == 3
    g = DatasetGroup(**cfg, split="valid")
    assert g.train is None and g.test is None and len(g.valid) == 2


def test_column_solver_has_no_host_fallback(monkeypatch):
    import torch
    from dmcf_amd import _lib
    from dmcf_amd.datasets import column_gen
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(_lib.DmcfError):
        column_gen.gen_data(data_cnt=1, timesteps=1, pts_cnt=[2])


def test_cases_that_still_raise(tmp_path):
    from dmcf_amd.datasets import DatasetGroup
    sec = dict(seed=1, data_cnt=1, timesteps=1)
    kw = dict(name="x", cache_dir=str(tmp_path / "cache"))
    with pytest.raises(NotImplementedError):
        DatasetGroup(**kw, type="tank", train=sec, valid=sec, test=sec, split="test")
    with pytest.raises(NotImplementedError):
        DatasetGroup(**kw, train=sec, valid=sec, test=sec, split="test")  # no type: the reference's default is tank
    with pytest.raises(NotImplementedError):
        DatasetGroup(**kw, type="pool", train=sec, valid=sec, test=sec, split="test")
    with pytest.raises(NotImplementedError):
        DatasetGroup(**kw, type="column", split="test")
    with pytest.raises(NotImplementedError):
        DatasetGroup(**kw, type="free_fall", train=sec, test=sec, split="valid")
    with pytest.raises(NotImplementedError):
        DatasetGroup(**kw, type="free_fall", valid=sec, test=sec, split="train")
    with pytest.raises(NotImplementedError):
        DatasetGroup(**kw, type="column", dataset_path=None, split="test")
    assert not os.path.exists(tmp_path / "cache")


# ---- ABI 2.17 ------------------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def hip_lib():
    from dmcf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dmcf_hip.h")).read(), flags=re.S)


def test_abi_symbol_declared_listed_exported(hip_lib):
    from dmcf_amd import _lib
    assert hip_lib.dmcf_version() >= 21700
    text = _header()
    assert re.search(r"\bdmcf_sph1d_rollout\s*\(", text) and "dmcf_sph1d_rollout" in _lib.SYMBOLS and hasattr(hip_lib, "dmcf_sph1d_rollout")
    c = ctypes
    fn = hip_lib.dmcf_sph1d_rollout
    assert fn.restype is c.c_int
    assert fn.argtypes == [c.c_void_p, c.c_void_p, c.c_int64, c.c_int32, c.POINTER(_lib.Sph1dParams), c.c_int32, c.c_void_p, c.c_void_p,
                           c.c_void_p, c.c_void_p]
    proto = re.search(r"int\s+dmcf_sph1d_rollout\s*\(([^)]*)\)", text).group(1)
    assert [p.split()[-1].lstrip("*") for p in proto.split(",")] == ["state", "n_tot", "n_scenes", "max_points", "params", "n_frames",
                                                                     "sequence", "state_out", "iterations", "stream"]
    ctype = {"int64_t": c.c_int64, "int32_t": c.c_int32}
    for p, a in zip(proto.split(","), fn.argtypes):
        if "*" not in p and "dmcf_stream_t" not in p:
            assert a is ctype[p.split()[-2]], p


def test_abi_struct_layout_matches_header():
    from dmcf_amd._lib import Sph1dParams
    text = _header()
    body = text[text.index("typedef struct dmcf_sph1d_params {"):text.index("} dmcf_sph1d_params;")]
    fields = re.findall(r"\b(uint32_t|int32_t|double)\s+([a-z_]+);", body)
    ctype = {"uint32_t": ctypes.c_uint32, "int32_t": ctypes.c_int32, "double": ctypes.c_double}
    assert [(n, ctype[t]) for t, n in fields] == list(Sph1dParams._fields_)
    assert ctypes.sizeof(Sph1dParams) == 16 + 7 * 8


def _params(**kw):
    from dmcf_amd._lib import Sph1dParams
    p = Sph1dParams()
    p.struct_size = ctypes.sizeof(p)
    p.bcnt, p.max_iter = 2, 10000
    p.h, p.rest_dens, p.stiffness, p.visc, p.gravity, p.dt, p.eps = 1.0, 2.0, 20.0, 0.1, -1000.0, 0.0025, 0.01
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_abi_host_validation(hip_lib):
    """Every argument error comes back before anything is enqueued."""
    def call(p=None, state=FAKE, n_tot=FAKE, scenes=1, points=42, frames=1, seq=FAKE, out=FAKE, iters=FAKE):
        p = _params() if p is None else p
        return hip_lib.dmcf_sph1d_rollout(state, n_tot, scenes, points, ctypes.byref(p), frames, seq, out, iters, None)

    assert call(points=65) == EINVAL  # one lane per point: at most 64
    assert call(points=0) == EINVAL
    assert call(scenes=-1) == EINVAL and call(frames=-1) == EINVAL
    assert call(state=None) == EINVAL and call(n_tot=None) == EINVAL and call(out=None) == EINVAL
    assert call(seq=None) == EINVAL and call(iters=None) == EINVAL
    assert call(p=_params(struct_size=8)) == EINVAL
    assert call(p=_params(bcnt=-1)) == EINVAL and call(p=_params(bcnt=42)) == EINVAL
    assert call(p=_params(max_iter=0)) == EINVAL
    assert call(p=_params(h=0.0)) == EINVAL and call(p=_params(rest_dens=0.0)) == EINVAL and call(p=_params(dt=float("nan"))) == EINVAL
    assert hip_lib.dmcf_sph1d_rollout(FAKE, FAKE, 1, 42, None, 1, FAKE, FAKE, FAKE, None) == EINVAL
    assert call(scenes=0, state=None, n_tot=None, seq=None, out=None, iters=None) == 0  # an empty batch enqueues nothing


def test_ops_refuses_cpu_tensors_and_large_scenes(hip_lib):
    import torch
    from dmcf_amd import _lib, ops
    with pytest.raises(_lib.DmcfError):
        ops.sph1d_rollout(torch.zeros(1, 3, 3), [3], 1, **_constants())
    assert ops.SPH1D_MAX_POINTS == 64 and ops.SPH1D_LAUNCH_ITERS <= 200_000
