"""CPU checks of the training loop: the tensor-bundle writer against the shipped Liquid3d checkpoint (tests/golden/
liquid3d_ckpt.npz), a synthetic model plus optimizer state through the writer and back, the training data flow and the loop's
schedules against restatements of the reference (datasets/dataset_reader_physics.py:210-357, pipelines/simulator.py:430-480),
and the C ABI of dmcf_adam_step (host-side validation only: no device is touched)."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
EINVAL = -1
FAKE = 1 << 20  # a non-NULL device address: validation returns before anything could dereference it
NEW = ["dmcf_adam_step_workspace_bytes", "dmcf_adam_step", "dmcf_adam_step_kernel_names"]


def _fixture(tmp_path):
    blob = np.load(os.path.join(GOLDEN, "liquid3d_ckpt.npz"))
    prefix = str(tmp_path / "ckpt")
    open(prefix + ".index", "wb").write(blob["index"].tobytes())
    open(prefix + ".data-00000-of-00001", "wb").write(blob["data"].tobytes())
    return prefix


def test_bundle_writer_reproduces_the_shipped_checkpoint(tmp_path):
    from dmcf_amd.utils import tf_checkpoint as tc
    src = _fixture(tmp_path)
    items = tc.read_bundle(src)
    assert len(items) == 154 and items[-1][0] == tc.OBJECT_GRAPH_KEY and isinstance(items[-1][1], bytes)
    out = str(tmp_path / "out" / "ckpt")
    tc.write_bundle(out, items)
    assert open(out + ".data-00000-of-00001", "rb").read() == open(src + ".data-00000-of-00001", "rb").read()
    orig, new = tc.read_index(src + ".index"), tc.read_index(out + ".index")
    assert set(orig) == set(new)
    for k in orig:
        assert {f: orig[k][f] for f in ("dtype", "shape", "shard", "offset", "size")} == \
            {f: new[k][f] for f in ("dtype", "shape", "shard", "offset", "size")}, k
    slot = [k for k in orig if ".OPTIMIZER_SLOT" in k]
    plain = [k for k in orig if ".OPTIMIZER_SLOT" not in k]
    assert len(slot) == 98 and len(plain) == 56
    assert all(orig[k]["crc32c"] == new[k]["crc32c"] for k in plain)
    # the fixture zeroed the slots' bytes but kept their checksums
    assert all(orig[k]["crc32c"] != new[k]["crc32c"] for k in slot)
    for k in slot:
        new[k]["crc32c"] = orig[k]["crc32c"]
    assert tc.encode_index(new) == open(src + ".index", "rb").read()  # the SSTable layout, byte for byte


def test_crc32c_known_values():
    from dmcf_amd.utils import tf_checkpoint as tc
    assert tc.crc32c(b"123456789") == 0xE3069283  # the CRC-32C check value
    assert tc.crc32c(bytes(32)) == 0x8A9136AA  # RFC 3720 B.4
    assert tc.crc32c(b"6789", tc.crc32c(b"12345")) == 0xE3069283


class _Opt:
    """What save_train_checkpoint reads of an optimizer (KerasAdam's state), on host tensors."""

    def __init__(self, params, rng):
        import torch
        self.params = params
        self.iterations, self.beta_1, self.beta_2, self.decay = 12345, 0.9, 0.999, 0.0
        self.m = [torch.from_numpy(rng.normal(size=p.shape).astype(np.float32)) if i % 3 else None for i, p in enumerate(params)]
        self.v = [torch.from_numpy(rng.uniform(size=p.shape).astype(np.float32)) if i % 3 else None for i, p in enumerate(params)]

    def slots_by_param(self):
        return {id(p): {"m": m, "v": v} for p, m, v in zip(self.params, self.m, self.v) if m is not None}


def test_synthetic_model_and_optimizer_state_round_trip(tmp_path):
    import torch
    from dmcf_amd.utils import tf_checkpoint as tc
    from dmcf_amd.models.base_model import Dense

    class Model(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.layers = [Dense(7), Dense(5, use_bias=False), Dense(3)]
            for i, (l, n) in enumerate(zip(self.layers, (4, 7, 5))):
                l.build(n, "cpu")

        def checkpoint_items(self):
            return [([f"model/dense/{i}", "model/other"], l) for i, l in enumerate(self.layers)]

    rng = np.random.default_rng(0)
    model = Model()
    variables = tc.model_variables(model)
    assert [k for k, _, _ in variables] == ["model/dense/0/kernel", "model/dense/0/bias", "model/dense/1/kernel",
                                            "model/dense/2/kernel", "model/dense/2/bias"]
    opt = _Opt([getattr(m, a) for _, m, a in variables], rng)
    graph = bytes(rng.integers(0, 256, size=300, dtype=np.uint8))
    mgr = tc.CheckpointManager(str(tmp_path / "checkpoint"), max_to_keep=2)
    for n in (1, 2, 3):
        mgr.save(model, opt, n, graph if n == 3 else None)
    assert sorted(f for f in os.listdir(tmp_path / "checkpoint") if f.endswith(".index")) == ["ckpt-2.index", "ckpt-3.index"]
    assert tc.CheckpointManager(str(tmp_path / "checkpoint")).latest_checkpoint == str(tmp_path / "checkpoint" / "ckpt-3")
    state = open(tmp_path / "checkpoint" / "checkpoint").read()
    assert state.startswith('model_checkpoint_path: "ckpt-3"\n') and 'all_model_checkpoint_paths: "ckpt-2"' in state
    weights, slots, o, g = tc.read_train_state(str(tmp_path / "checkpoint" / "ckpt-3"))
    assert g == graph and o["iter"] == 12345 and o["save_counter"] == 3
    assert o["beta_1"] == np.float32(0.9) and o["beta_2"] == np.float32(0.999) and o["decay"] == 0.0
    for i, (key, mod, attr) in enumerate(variables):
        p = getattr(mod, attr).detach().numpy()
        assert weights[key].dtype == np.float32 and np.array_equal(weights[key].view(np.uint32), p.view(np.uint32))
        if opt.m[i] is None:
            assert key not in slots
        else:
            assert np.array_equal(slots[key]["m"], opt.m[i].numpy()) and np.array_equal(slots[key]["v"], opt.v[i].numpy())
    e = tc.read_index(str(tmp_path / "checkpoint" / "ckpt-3.index"))
    assert e["step/.ATTRIBUTES/VARIABLE_VALUE"]["dtype"] == 3 and e["optimizer/iter/.ATTRIBUTES/VARIABLE_VALUE"]["dtype"] == 9
    assert tc.checkpoint_epoch(str(tmp_path / "checkpoint" / "ckpt-3"), 5) == 11


# ---- data flow and schedules -----------------------------------------------------------------------------------------------

def _scene(n_frames=9, n=20, m=6, grav=True, seed=0):
    rng = np.random.default_rng(seed)
    box, bn = rng.normal(size=(m, 3)).astype(np.float32), rng.normal(size=(m, 3)).astype(np.float32)
    frames = [dict(pos=rng.normal(size=(n, 3)).astype(np.float32), vel=rng.normal(size=(n, 3)).astype(np.float32), frame_id=t,
                   scene_id="s", box=box, box_normals=bn) for t in range(n_frames)]
    for f in frames if grav else []:
        f["grav"] = np.array([0.0, -9.81, 0.0], np.float32)
    return frames


def _restated_samples(scenes, window, pre_frames, stride, sample_cnt, augment, translate, scale, seed):
    """datasets/dataset_reader_physics.py:295-357 + :236-293, restated: the flow's rng shuffles and jitters, numpy's global
    generator draws pre and the rotation."""
    rng = np.random.RandomState(seed)
    shuffle = True
    files = np.arange(len(scenes))
    rng.shuffle(files)
    for fi in files:
        data = scenes[fi]
        idxs = np.arange(len(data) - (window + pre_frames) * stride)
        rng.shuffle(idxs)
        idxs = idxs[:sample_cnt] if sample_cnt is not None else idxs
        for i in idxs:
            pre = np.random.randint(pre_frames + 1)
            fr = [data[i + j * stride] for j in range(pre + window + 1)]
            s = {"pre": pre}
            for k in ("pos", "vel"):
                s[k] = np.stack([f[k] for f in fr]).astype(np.float32)
            s["grav"] = np.stack([f["grav"] for f in fr]).astype(np.float32) if "grav" in fr[0] else [None]
            if s["grav"][0] is not None:
                s["grav"] = np.full_like(s["vel"], s["grav"][:, None, :])
            for k in ("box", "box_normals"):
                s[k] = np.stack([data[0][k]] * len(fr)).astype(np.float32)
            s["frame_id"] = np.array([f["frame_id"] for f in fr])
            for mode, cfg in augment.items():
                if mode == "rotate":
                    th = np.random.rand(3)[0] * 2 * np.pi
                    R = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]]).astype(np.float32)
                    for k in ("box", "box_normals", "pos", "vel"):
                        s[k] = s[k] @ R
                    if s["grav"][0] is not None:
                        s["vel"] = s["grav"] @ R  # the reference's leaked loop variable: vel <- rotated gravity
                elif mode == "jitter":
                    for k, v in cfg["channels"].items():
                        s[k] += rng.normal(scale=v, size=s[k].shape)
                elif mode == "jitter_inp":
                    for k, v in cfg["channels"].items():
                        s[k][0] += rng.normal(scale=v, size=s[k][0].shape)
            if translate is not None:
                s["pos"] += translate
                s["box"] += translate
            if scale is not None:
                for k in ("pos", "box", "vel"):
                    s[k] *= scale
                if s["grav"][0] is not None:
                    s["grav"] *= scale
            yield s
    assert shuffle


@pytest.mark.parametrize("augment", [{}, {"jitter_inp": {"channels": {"pos": [0.001, 0.002, 0.0]}}, "rotate": {"rot_axis": 1}},
                                     {"jitter": {"channels": {"pos": 0.01, "vel": 0.001}}}])
def test_data_flow_against_restatement(augment):
    from dmcf_amd.datasets import Dataset, PhysicsSimDataFlow
    scenes = [_scene(seed=0), _scene(11, seed=1, grav=False)]
    kw = dict(window=2, pre_frames=2, stride=2, sample_cnt=3, augment=augment, translate=[0.5, 0.0, -0.5], scale=[1.0, 2.0, 1.0])
    np.random.seed(7)
    want = list(_restated_samples(scenes, seed=3, **kw))
    np.random.seed(7)
    got = list(PhysicsSimDataFlow(Dataset(data=scenes), shuffle=True, seed=3, **kw))
    assert len(got) == len(want) == 4  # one start frame in the 9-frame scene, three of the 11-frame one
    for g, w in zip(got, want):
        assert g["pre"] == w["pre"] and np.array_equal(g["frame_id"], w["frame_id"])
        assert g["pos"].shape[0] == w["pre"] + 3 and np.all(np.diff(g["frame_id"]) == 2)
        for k in ("pos", "vel", "box", "box_normals"):
            assert g[k].dtype == np.float32 and np.array_equal(g[k], w[k]), k
        if w["grav"][0] is None:
            assert g["grav"] == [None]
        else:
            assert np.array_equal(g["grav"], w["grav"])


def test_dataloader_batches_repeat_and_shuffle():
    from dmcf_amd.datasets import Dataset, get_dataloader
    scenes = [_scene(6)]
    np.random.seed(0)
    a = get_dataloader(Dataset(data=scenes), batch_size=3, window=1, repeat=True, shuffle_buffer=4, seed=5, num_workers=2)
    batches = [next(a) for _ in range(5)]  # (5 samples per pass: the flow repeats)
    assert all(len(b["pos"]) == 3 and b["pos"][0].shape == (2, 20, 3) for b in batches)
    starts = [int(f[0]) for b in batches for f in b["frame_id"]]
    assert sorted(set(starts)) == [0, 1, 2, 3, 4]
    np.random.seed(0)
    b = get_dataloader(Dataset(data=scenes), batch_size=3, window=1, repeat=True, shuffle_buffer=4, seed=5)
    again = [next(b) for _ in range(5)]
    assert [[f.tolist() for f in x["frame_id"]] for x in again] == [[f.tolist() for f in x["frame_id"]] for x in batches]
    finite = list(get_dataloader(Dataset(data=scenes), batch_size=3, window=1))
    assert len(finite) == 1  # 5 samples, batches of 3: the incomplete one is dropped
    assert [int(f[0]) for f in finite[0]["frame_id"]] == [0, 1, 2]


def test_dataset_group_train_split(tmp_path):
    from dmcf_amd.datasets import DatasetGroup, write_scene
    with pytest.raises(NotImplementedError):
        DatasetGroup(name="x", dataset_path=str(tmp_path), split="train")
    (tmp_path / "train").mkdir()
    write_scene(str(tmp_path / "train" / "a.msgpack.zst"), _scene(4))
    write_scene(str(tmp_path / "b.msgpack.zst"), _scene(3))
    g = DatasetGroup(name="x", dataset_path=str(tmp_path), split="train")
    assert len(g.train) == 1 and len(g.train[0]) == 4 and len(g.valid[0]) == 3 and len(g.test[0]) == 3
    d = DatasetGroup(name="x", data=[_scene(2)])
    assert d.train is d.valid and len(d.train) == 1


class _Cfg(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)


def _restated_schedule(cfg, steps, lengths_pres):
    """pipelines/simulator.py:430-480 restated: loader rebuilds, the window / warm-up / its indices and time_w per step."""
    window_it = warm_up_it = it_idx = 0
    out = []
    for step in steps:
        rebuilt = False
        while window_it < min(len(cfg.windows), len(cfg.window_bnds)) and step >= cfg.window_bnds[window_it]:
            window_it += 1
            rebuilt = True
        while warm_up_it < min(len(cfg.max_warm_up), len(cfg.warm_up_bnds)) and step >= cfg.warm_up_bnds[warm_up_it]:
            warm_up_it += 1
            rebuilt = True
        while it_idx < min(len(cfg.iterations), len(cfg.its_bnds)) and step >= cfg.its_bnds[it_idx]:
            it_idx += 1
        lengths, pres = lengths_pres(cfg.windows[window_it], cfg.max_warm_up[warm_up_it])
        time_w = np.ones((np.min([d - 1 - p for d, p in zip(lengths, pres)])), dtype=np.float32)
        if window_it > 0:
            a = (step - cfg.window_bnds[window_it - 1] + 1) / cfg.time_blend
            if a < 1.0 and len(time_w) >= cfg.windows[window_it]:
                diff = cfg.windows[window_it] - cfg.windows[window_it - 1]
                time_w[-diff:] = np.clip(a - np.arange(diff) / diff, 0.0, 1.0)
        out.append((rebuilt, cfg.windows[window_it], cfg.max_warm_up[warm_up_it], cfg.iterations[it_idx], time_w))
    return out


@pytest.mark.parametrize("cfg", [
    _Cfg(windows=[3, 5, 10, 20], window_bnds=[5000, 10000, 15000], time_blend=200, max_warm_up=[0, 5, 10, 20],
         warm_up_bnds=[20000, 25000, 30000], iterations=[0], its_bnds=[]),  # configs/WaterRamps.yml
    _Cfg(windows=[2, 3], window_bnds=[15000], time_blend=200, max_warm_up=[0], warm_up_bnds=[], iterations=[0, 1, 2],
         its_bnds=[100, 14990]),  # Liquid3d's windows
    _Cfg(windows=[1, 2], window_bnds=[1], time_blend=2, max_warm_up=[0, 1, 2, 3], warm_up_bnds=[3, 5, 7], iterations=[0, 1], its_bnds=[0]),
])
def test_schedules_against_restatement(cfg):
    from dmcf_amd.pipelines.simulator import TrainSchedule
    rng = np.random.default_rng(1)
    steps = sorted(set([0, 1, 2, 3, 4, 5, 6, 7, 99, 100, 101] + list(rng.integers(0, 32000, size=300))
                       + [b + d for b in cfg.window_bnds + cfg.warm_up_bnds for d in (-1, 0, 1, 2, 50, 150, 199, 200)]))
    steps = [s for s in steps if s >= 0]
    samples = {}

    def lengths_pres(window, warm):
        key = (window, warm)
        if key not in samples:
            pres = [int(p) for p in rng.integers(0, warm + 1, size=4)]
            samples[key] = ([p + window + 1 for p in pres], pres)
        return samples[key]

    want = _restated_schedule(cfg, steps, lengths_pres)
    sched = TrainSchedule(cfg)
    for step, (rebuilt, window, warm, its, time_w) in zip(steps, want):
        assert sched.advance(step) == rebuilt, step
        assert (sched.window, sched.pre_frames, sched.iterations) == (window, warm, its), step
        lengths, pres = lengths_pres(window, warm)
        tw = sched.time_weights(lengths, pres, step)
        assert tw.dtype == np.float32 and np.array_equal(tw, time_w), step


def test_keras_adam_coefficients_and_get_optimizer_docstring():
    from dmcf_amd.utils.tools import losses
    opt = losses.KerasAdam([], lr_boundaries=[20000, 25000], lr_values=[1e-3, 5e-4, 2.5e-4])
    assert opt.lr(0) == np.float32(1e-3) and opt.lr(20000) == np.float32(1e-3) and opt.lr(20001) == np.float32(5e-4)
    assert opt.lr(51000) == np.float32(2.5e-4)
    lr, b1p, b2p = opt.coefficients(0)
    assert b1p == np.float32(0.9) and b2p == np.float32(0.999)
    _, b1p, b2p = opt.coefficients(51000)
    assert b1p == np.power(np.float32(0.9), np.float32(51001)) and b2p == np.power(np.float32(0.999), np.float32(51001))
    opt.decay = 0.5
    assert opt.lr(2) == np.float32(np.float32(1e-3) / np.float32(2.0))
    opt.step()  # no parameters: the iteration still counts (Keras)
    assert opt.iterations == 1
    assert "KerasAdam" in losses.get_optimizer.__doc__


# ---- the C ABI -------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def hip_lib():
    from dmcf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_adam_symbols_and_version(hip_lib):
    from dmcf_amd import _lib
    assert hip_lib.dmcf_version() >= 21100
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dmcf_hip.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert name in _lib.SYMBOLS and hasattr(hip_lib, name)


@pytest.mark.parametrize("struct,cls,size", [("dmcf_adam_tensor", "AdamTensor", 40), ("dmcf_adam_args", "AdamArgs", 56)])
def test_adam_structs_mirror_header(struct, cls, size):
    from dmcf_amd import _lib
    C = getattr(_lib, cls)
    text = open(os.path.join(ROOT, "include", "dmcf_hip.h")).read()
    body = text[text.index(f"typedef struct {struct} {{"):text.index(f"}} {struct};")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"^\s*(?:const\s+)?([a-z0-9_]+\*?)\s+(\*?)([a-z_0-9]+);", body, flags=re.M)
    assert [f[2] for f in fields] == [f[0] for f in C._fields_]
    ctypes_of = {"uint32_t": ctypes.c_uint32, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float}
    for (typ, star, name), (_, ctyp) in zip(fields, C._fields_):
        assert ctyp is (ctypes.c_void_p if (typ.endswith("*") or star) else ctypes_of[typ]), name
    assert ctypes.sizeof(C) == size


def _args(sizes=(10, 3), **kw):
    from dmcf_amd._lib import AdamArgs, AdamTensor
    recs = (AdamTensor * max(len(sizes), 1))()
    for i, n in enumerate(sizes):
        recs[i].param = recs[i].grad = recs[i].m = recs[i].v = FAKE + 4096 * i
        recs[i].n = n
    a = AdamArgs()
    a.struct_size = ctypes.sizeof(AdamArgs)
    a.n_tensors = len(sizes)
    a.tensors = ctypes.cast(recs, ctypes.c_void_p).value
    a.device_tensors = FAKE
    a.lr, a.beta_1, a.beta_2, a.epsilon, a.beta_1_power, a.beta_2_power, a.clip_norm = 1e-3, 0.9, 0.999, 1e-6, 0.9, 0.999, -1.0
    for k, v in kw.items():
        setattr(a, k, v)
    return a, recs


def _names(L, a):
    buf = ctypes.create_string_buffer(64)
    rc = L.dmcf_adam_step_kernel_names(ctypes.byref(a), buf, 64)
    return rc, buf.value.decode()


def test_adam_kernel_names_and_workspace(hip_lib):
    a, keep = _args()
    assert _names(hip_lib, a) == (0, "adam_update")
    assert hip_lib.dmcf_adam_step_workspace_bytes(ctypes.byref(a)) == 0
    a, keep = _args(sizes=(5000, 3, 0), clip_norm=1.0)
    assert _names(hip_lib, a) == (0, "adam_sumsq;adam_update")
    assert hip_lib.dmcf_adam_step_workspace_bytes(ctypes.byref(a)) == 8 * 3 * 5  # a double per (tensor, block column)
    a, keep = _args(sizes=(0, 0), clip_norm=1.0)
    assert _names(hip_lib, a) == (0, "")
    a, keep = _args(sizes=())
    assert _names(hip_lib, a) == (0, "")
    assert hip_lib.dmcf_adam_step(ctypes.byref(a), None, 0, None) == 0  # nothing to do: nothing enqueued


@pytest.mark.parametrize("case", ["short", "count_neg", "n_neg", "param_null", "grad_null", "m_null", "v_null", "table_null",
                                  "device_table_null", "too_many", "clip_nan", "workspace"])
def test_adam_validation(hip_lib, case):
    kw = {}
    sizes = (10, 3)
    if case == "count_neg":
        kw["n_tensors"] = -1
    elif case == "too_many":
        kw["n_tensors"] = 65536
    elif case == "table_null":
        kw["tensors"] = None
    elif case == "device_table_null":
        kw["device_tensors"] = None
    elif case == "clip_nan":
        kw["clip_norm"] = float("nan")
    a, recs = _args(sizes, **kw)
    if case == "short":
        a.struct_size -= 4
    elif case == "n_neg":
        recs[1].n = -3
    elif case.endswith("_null") and case not in ("table_null", "device_table_null"):
        setattr(recs[1], case[:-5], None)
    if case == "workspace":
        a.clip_norm = 1.0
        assert hip_lib.dmcf_adam_step(ctypes.byref(a), None, 0, None) == -2  # DMCF_EWORKSPACE
        return
    assert hip_lib.dmcf_adam_step(ctypes.byref(a), None, 0, None) == EINVAL
    assert hip_lib.dmcf_adam_step_workspace_bytes(ctypes.byref(a)) == 0
    assert _names(hip_lib, a)[0] == EINVAL
