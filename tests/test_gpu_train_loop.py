"""The training loop on the GPU: dmcf_adam_step against a float64 restatement of TensorFlow's ApplyAdam, Simulator.train_step
against a composition of the model's own pieces, run_pipeline --split train end to end with checkpoints and resume, and one
2-D iteration."""
import glob
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ULP8 = 8 * 2.0 ** -24
LR_CFG = dict(lr_boundaries=[20000, 25000, 30000, 35000, 40000, 45000],
              lr_values=[0.001, 0.0005, 0.00025, 0.000125, 0.0000625, 0.00003125, 0.000015625])  # configs/Liquid3d.yml
LOSS = {"weighted_mse": dict(typ="weighted_mse", fac=128.0, gamma=0.5, neighbor_scale=0.025)}


def apply_adam64(p, g, m, v, lr, b1, b2, eps, b1p, b2p, clip):
    """TensorFlow's ApplyAdam (after tf.clip_by_norm when clip > 0) in float64 on float32 inputs."""
    p, g, m, v = (np.asarray(x, np.float64) for x in (p, g, m, v))
    lr, b1, b2, eps, b1p, b2p = (float(np.float32(x)) for x in (lr, b1, b2, eps, b1p, b2p))
    if clip and clip > 0:
        norm = np.sqrt(np.sum(g * g))
        g = g * clip / max(norm, clip)
    alpha = lr * np.sqrt(1 - b2p) / (1 - b1p)
    m = m + (1 - b1) * (g - m)
    v = v + (1 - b2) * (g * g - v)
    return p - alpha * m / (eps + np.sqrt(v)), m, v


def _adam_case(rng, sizes, it):
    ps, gs, ms, vs = [], [], [], []
    for i, n in enumerate(sizes):
        ps.append(rng.normal(size=n).astype(np.float32))
        scale = 10.0 ** rng.uniform(-8, 0, size=n)  # (gradients from 1e-8 to 1: epsilon matters for some, not for others)
        gs.append((rng.normal(size=n) * scale).astype(np.float32))
        if it == 0:
            ms.append(np.zeros(n, np.float32))
            vs.append(np.zeros(n, np.float32))
        else:
            ms.append((rng.normal(size=n) * scale).astype(np.float32))
            vs.append((rng.uniform(0, 1, size=n) * scale * scale).astype(np.float32))
    return ps, gs, ms, vs


@pytest.mark.parametrize("clip", [None, 0.01])
@pytest.mark.parametrize("it", [0, 1, 51000])
def test_adam_step_against_float64_apply_adam(it, clip):
    from dmcf_amd import ops
    from dmcf_amd.utils.tools.losses import KerasAdam
    rng = np.random.default_rng(100 + it)
    # 1001: a vector body and a tail; 262149 > 256 x 1024: the block columns are capped and stride over the tensor (and over
    # adam_sumsq's partials); the last tensor's param is a view one float into its buffer: the element-wise path
    sizes = [0, 1, 3, 1000, 4 * 4 * 4 * 24 * 16, 1001, 262149, 1003]
    misaligned = len(sizes) - 1
    ps, gs, ms, vs = _adam_case(rng, sizes, it)
    opt = KerasAdam([], **LR_CFG)
    lr, b1p, b2p = opt.coefficients(it)
    assert lr == np.float32(LR_CFG["lr_values"][0] if it < 20000 else LR_CFG["lr_values"][-1])
    dev = lambda a: torch.from_numpy(a.copy()).cuda()  # noqa: E731

    def dev_param(i, a):
        if i != misaligned:
            return dev(a)
        t = torch.from_numpy(np.concatenate([np.zeros(1, np.float32), a])).cuda()[1:]
        assert t.data_ptr() % 16 == 4 and t.is_contiguous()
        return t

    results = []
    for _ in range(2):
        P = [dev_param(i, a) for i, a in enumerate(ps)]
        G, M, V = ([dev(a) for a in arrs] for arrs in (gs, ms, vs))
        ops.adam_step(P, G, M, V, lr, 0.9, 0.999, 1e-6, b1p, b2p, clip)
        torch.cuda.synchronize()
        results.append([[t.cpu().numpy() for t in arrs] for arrs in (P, M, V)])
    assert ops.adam_step_kernel_names(P, G, M, V, clip) == ("adam_sumsq;adam_update" if clip else "adam_update")
    for a, b in zip(results[0], results[1]):  # identical bits over two calls
        for x, y in zip(a, b):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    P, M, V = results[0]
    for i in range(len(sizes)):
        p_ref, m_ref, v_ref = apply_adam64(ps[i], gs[i], ms[i], vs[i], lr, 0.9, 0.999, 1e-6, b1p, b2p, clip)
        for got, ref, old in ((P[i], p_ref, ps[i]), (M[i], m_ref, ms[i]), (V[i], v_ref, vs[i])):
            bar = ULP8 * (np.abs(ref) + np.abs(ref - old)) + 1e-45
            err = np.abs(got.astype(np.float64) - ref)
            assert np.all(err <= bar), (sizes[i], float(np.max(err / bar)))


def test_adam_step_is_not_torch_adam_and_skips_missing_gradients():
    """Iteration 0 with |g| ~ 1e-7: TensorFlow adds epsilon to sqrt(v), torch to the bias-corrected sqrt(v)."""
    from dmcf_amd.utils.tools.losses import KerasAdam
    rng = np.random.default_rng(5)
    p0 = (0.1 * rng.normal(size=4096)).astype(np.float32)
    g = (1e-7 * rng.choice([-1.0, 1.0], size=4096) * rng.uniform(0.5, 1.5, size=4096)).astype(np.float32)
    a = torch.nn.Parameter(torch.from_numpy(p0.copy()).cuda())
    unused = torch.nn.Parameter(torch.ones(7, device="cuda"))
    opt = KerasAdam([a, unused], **LR_CFG)
    a.grad = torch.from_numpy(g.copy()).cuda()
    opt.step()
    assert opt.iterations == 1 and opt.m[1] is None and opt.v[1] is None  # no gradient: no slots, no update
    assert torch.equal(unused.detach(), torch.ones(7, device="cuda"))
    lr, b1p, b2p = opt.coefficients(0)
    ref, _, _ = apply_adam64(p0, g, 0 * g, 0 * g, lr, 0.9, 0.999, 1e-6, b1p, b2p, None)
    got = a.detach().cpu().numpy().astype(np.float64)
    bar = ULP8 * (np.abs(ref) + np.abs(ref - p0))
    assert np.all(np.abs(got - ref) <= bar)
    b = torch.nn.Parameter(torch.from_numpy(p0.copy()).cuda())
    topt = torch.optim.Adam([b], lr=1e-3, eps=1e-6)
    b.grad = torch.from_numpy(g.copy()).cuda()
    topt.step()
    diff = np.abs(b.detach().cpu().numpy().astype(np.float64) - ref)
    assert np.median(diff / bar) > 100


# ---- the training step ---------------------------------------------------------------------------------------------------

def _canyon():
    return dict(np.load(os.path.join(GOLDEN, "canyon_frames.npz")))


def _liquid3d(weights=True):
    from dmcf_amd import models
    from dmcf_amd.utils import tf_checkpoint as tc
    from tools import configs
    cfg = dict(configs.LIQUID3D, loss=LOSS)
    model = getattr(models, cfg["name"])(**cfg)
    if weights:
        tc.load_into_model(model, dict(np.load(os.path.join(GOLDEN, "liquid3d_weights.npz"))), device="cuda:0")
    return model


def _batch(fx, samples):
    """A get_dataloader batch from (first frame, frame count, pre) per sample of the canyon frames."""
    out = {k: [] for k in ("pos", "vel", "grav", "box", "box_normals", "pre")}
    for f0, n, pre in samples:
        out["pos"].append(fx["pos"][f0:f0 + n].copy())
        out["vel"].append(fx["vel"][f0:f0 + n].copy())
        out["grav"].append([None])
        out["box"].append(np.stack([fx["box"]] * n))
        out["box_normals"].append(np.stack([fx["box_normals"]] * n))
        out["pre"].append(pre)
    return out


def _composition(model, data, time_w, max_dens_err, w_decay=0.0):
    """The reference's train() composed from the model's own calls: warm-up on the inference path with the max_dens_err exit
    (state after p + 1 steps against frame p; pre = the last loop index), the recorded window, model.loss, time_w, the
    w_decay term (w_decay times the sum of every weight's squares: a scalar), backward."""
    from dmcf_amd.utils.tools.losses import density_loss, get_window_func
    cuda = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()  # noqa: E731
    starts, pres = [], []
    for bi in range(len(data["pos"])):
        box = cuda(data["box"][bi][0])
        pos, vel = cuda(data["pos"][bi][0]), cuda(data["vel"][bi][0])
        p, prev = 0, 0.0
        with torch.no_grad():
            for p in range(data["pre"][bi]):
                pos2, vel2 = model([pos, vel, None, None, box, cuda(data["box_normals"][bi][0])], training=False)
                fr = cuda(data["pos"][bi][p])
                err = float(density_loss(pos2, fr, torch.cat([pos2, box]), torch.cat([fr, box]), radius=model.particle_radii[0],
                                         win=get_window_func(model.window_dens), use_max=True))
                if p > 0 and err > prev and err > max_dens_err:
                    break
                prev = err
                pos, vel = pos2, vel2
        starts.append((pos, vel))
        pres.append(p)
    model.requires_grad_(True)
    total = 0
    for bi, (pos, vel) in enumerate(starts):
        box, bn = cuda(data["box"][bi][0]), cuda(data["box_normals"][bi][0])
        for t in range(len(time_w)):
            inputs = [pos, vel, None, None, box, bn]
            pos, vel = model(inputs, training=True)
            pre = pres[bi]
            loss = model.loss([pos, vel], [inputs, cuda(data["pos"][bi][t + pre + 1]), cuda(data["pos"][bi][t + pre]), pre])
            total = total + loss["weighted_mse"] * float(time_w[t])
    total = total / (float(np.sum(time_w)) * len(starts))
    if w_decay > 0:
        from dmcf_amd.utils import tf_checkpoint as tc
        total = total + w_decay * sum(torch.sum(getattr(mod, attr) ** 2) for _, mod, attr in tc.model_variables(model))
    total.backward()
    return float(total.detach()), pres


@pytest.mark.parametrize("w_decay", [0.0, 1e-3])
def test_train_step_against_composition(tmp_path, w_decay):
    from dmcf_amd.pipelines import Simulator
    from dmcf_amd.utils import tf_checkpoint as tc
    from dmcf_amd.utils.tools.losses import KerasAdam
    fx = _canyon()
    data = _batch(fx, [(1, 4, 0), (0, 6, 2)])  # (the second sample warms up two steps: one max_dens_err comparison at p = 1)
    time_w = np.array([1.0, 1.0, 0.5], np.float32)
    max_dens_err = 0.1
    ref_model = _liquid3d()
    ref_loss, ref_pres = _composition(ref_model, data, time_w, max_dens_err, w_decay)
    model = _liquid3d()
    sim = Simulator(model, None, main_log_dir=str(tmp_path), device="cuda", optimizer=LR_CFG, w_decay=w_decay)
    before = {k: getattr(mod, attr).detach().clone() for k, mod, attr in tc.model_variables(model)}
    loss, pres = sim.train_step(data, time_w, 0, None, max_dens_err)
    assert pres == ref_pres and pres[0] == 0
    assert loss.shape == (len(model.loss_keys()),) == (1,)  # one entry per loss key, the w_decay term added to each
    assert float(loss[0]) == pytest.approx(ref_loss, rel=1e-5)
    assert isinstance(sim.optimizer, KerasAdam) and sim.optimizer.iterations == 1
    lr, b1p, b2p = sim.optimizer.coefficients(0)
    ref_vars = {k: getattr(mod, attr) for k, mod, attr in tc.model_variables(ref_model)}
    checked = 0
    for key, mod, attr in tc.model_variables(model):
        g = ref_vars[key].grad
        if g is None:
            assert sim.optimizer.slots_by_param().get(id(getattr(mod, attr))) is None, key
            continue
        p0 = before[key].cpu().numpy()
        want, _, _ = apply_adam64(p0, g.cpu().numpy(), 0 * p0, 0 * p0, lr, 0.9, 0.999, 1e-6, b1p, b2p, None)
        got = getattr(mod, attr).detach().cpu().numpy().astype(np.float64)
        d_ref, d_got = want - p0, got - p0
        assert np.linalg.norm(d_got - d_ref) <= 2e-3 * np.linalg.norm(d_ref) + 1e-12, key
        checked += 1
    assert checked >= 40


# ---- the loop ------------------------------------------------------------------------------------------------------------

def _scenes_from_canyon():
    fx = _canyon()
    return [[dict(pos=fx["pos"][t], vel=fx["vel"][t], frame_id=t, scene_id="canyon", box=fx["box"],
                  box_normals=fx["box_normals"]) for t in range(fx["pos"].shape[0])]]


def _yaml(path, model, pipeline):
    import yaml
    path.mkdir(parents=True, exist_ok=True)
    cfg = dict(dataset=dict(name="canyon"), model=dict(model, ckpt_path=None), pipeline=dict(dict(
        name="Simulator", version="train", main_log_dir=str(path / "logs"), output_dir=str(path / "out"), batch_size=2, iter=2,
        max_epoch=1, windows=[1, 2], window_bnds=[1], time_blend=2, max_warm_up=[0], warm_up_bnds=[], iterations=[0],
        its_bnds=[], max_dens_err=0.1, save_ckpt_freq=1, optimizer=LR_CFG,
        data_generator=dict(scale=[1.0, 1.0, 1.0],
                            train=dict(stride=1, repeat=True, shuffle_buffer=4, sample_cnt=3,
                                       augment=dict(jitter_inp=dict(channels=dict(pos=[0.001, 0.001, 0.001])),
                                                    rotate=dict(rot_axis=1))),
                            valid=dict(stride=1, time_end=3), test=dict(stride=1, time_start=0, time_end=3))), **pipeline))
    yml = path / "train.yml"
    yml.write_text(yaml.safe_dump(cfg))
    return str(yml)


def _state(sim):
    opt = sim.optimizer
    slots = opt.slots_by_param()
    out = {"iter": opt.iterations}
    from dmcf_amd.utils import tf_checkpoint as tc
    for key, mod, attr in tc.model_variables(sim.model):
        p = getattr(mod, attr)
        out[key] = p.detach().cpu().numpy().copy()
        if id(p) in slots:
            out[key + "/m"] = slots[id(p)]["m"].cpu().numpy().copy()
            out[key + "/v"] = slots[id(p)]["v"].cpu().numpy().copy()
    return out


def test_run_pipeline_train_checkpoints_and_resume(tmp_path, monkeypatch):
    from dmcf_amd import run_pipeline
    from dmcf_amd.pipelines import Simulator
    from dmcf_amd.utils import tf_checkpoint as tc
    from tools import configs
    scenes = _scenes_from_canyon()
    yml = _yaml(tmp_path, dict(configs.LIQUID3D, loss=LOSS), {})
    saved, calls, first_state = {}, [], {}
    real_save, real_step = Simulator.save_ckpt, Simulator.train_step

    def save_ckpt(self, epoch):
        path = real_save(self, epoch)
        saved[os.path.basename(path)] = _state(self)
        return path

    def train_step(self, *a, **kw):
        if not calls:
            first_state.update(_state(self))
        calls.append(self.optimizer.iterations)
        return real_step(self, *a, **kw)

    monkeypatch.setattr(Simulator, "save_ckpt", save_ckpt)
    monkeypatch.setattr(Simulator, "train_step", train_step)
    loss = run_pipeline.main(["-c", yml, "--split", "train"], data=scenes)
    assert loss and all(np.isfinite(v) for v in loss.values())
    assert calls == [0, 1, 2, 3]  # epochs 0 and 1, two iterations each
    logs = os.path.join(str(tmp_path), "logs", "SymNet_canyon_train")
    ck = os.path.join(logs, "checkpoint")
    assert os.path.exists(os.path.join(ck, "checkpoint")) and sorted(saved) == ["ckpt-1", "ckpt-2"]
    for name in saved:
        assert os.path.exists(os.path.join(ck, name + ".index")) and os.path.exists(os.path.join(ck, name + ".data-00000-of-00001"))
    weights, slots, opt, graph = tc.read_train_state(os.path.join(ck, "ckpt-2"))
    assert int(opt["iter"]) == 4 and opt["save_counter"] == 2 and graph is None
    assert any(not np.array_equal(first_state[k], weights[k]) for k in weights)  # the parameters changed
    for k, w in weights.items():  # the file holds the end state
        assert np.array_equal(w, saved["ckpt-2"][k])
        assert np.array_equal(slots[k]["m"], saved["ckpt-2"][k + "/m"]) and np.array_equal(slots[k]["v"], saved["ckpt-2"][k + "/v"])
    train_logs = glob.glob(os.path.join(logs, "log_train_*.txt"))
    assert len(train_logs) == 1 and "training - weighted_mse:" in open(train_logs[0]).read()
    valid = "".join(open(f).read() for f in glob.glob(os.path.join(logs, "log_valid_*.txt")))  # (one file per second)
    assert "validation of epoch 0" in valid and "validation of epoch 1" in valid
    out = os.path.join(str(tmp_path), "out", "SymNet_canyon_train", "visual", "0000")
    assert os.path.exists(os.path.join(out, "0001.hdf5"))

    # resume: the newest checkpoint, epoch 2 only
    calls.clear()
    first_state.clear()
    run_pipeline.main(["-c", yml, "--split", "train", "--pipeline.max_epoch", "2"], data=scenes)
    assert calls == [4, 5]
    end = saved["ckpt-2"]
    assert set(first_state) == set(end)
    for k in end:
        assert np.array_equal(np.asarray(first_state[k]), np.asarray(end[k])), k
    assert "ckpt-3" in saved and saved["ckpt-3"]["iter"] == 6
    assert int(tc.read_train_state(os.path.join(ck, "ckpt-3"))[2]["iter"]) == 6

    # an explicit checkpoint: the shipped Liquid3d one (Adam slots zeroed in the fixture), iteration 51000
    blob = np.load(os.path.join(GOLDEN, "liquid3d_ckpt.npz"))
    (tmp_path / "fixture").mkdir()
    prefix = str(tmp_path / "fixture" / "ckpt")
    open(prefix + ".index", "wb").write(blob["index"].tobytes())
    open(prefix + ".data-00000-of-00001", "wb").write(blob["data"].tobytes())
    calls.clear()
    lrs = []
    real_step2 = Simulator.train_step

    def train_step2(self, *a, **kw):
        lrs.append(float(self.optimizer.lr()))
        return real_step2(self, *a, **kw)

    monkeypatch.setattr(Simulator, "train_step", train_step2)
    yml2 = _yaml(tmp_path / "b", dict(configs.LIQUID3D, loss=LOSS), dict(max_epoch=0, iter=1))
    run_pipeline.main(["-c", yml2, "--split", "train", "--ckpt_path", prefix], data=scenes)
    assert calls == [51000] and lrs == [pytest.approx(0.000015625, rel=1e-6)]
    ck2 = os.path.join(str(tmp_path / "b"), "logs", "SymNet_canyon_train", "checkpoint")
    # save_counter is restored from the explicit checkpoint as well (51 in the shipped one): the first file is ckpt-52
    assert sorted(f for f in os.listdir(ck2) if f.endswith(".index")) == ["ckpt-52.index"]
    w2, s2, o2, g2 = tc.read_train_state(os.path.join(ck2, "ckpt-52"))
    assert int(o2["iter"]) == 51001 and o2["save_counter"] == 52
    assert g2 == tc.read_train_state(prefix)[3]  # the object graph is carried over


def test_waterramps_2d_iteration(tmp_path, monkeypatch):
    from dmcf_amd import run_pipeline
    from dmcf_amd.pipelines import Simulator
    from dmcf_amd.utils import tf_checkpoint as tc
    from tools import configs, scenes as sc
    s = sc.box_scene(16, h=0.01, dim=2)
    frames = []
    pos, vel = s["pos"].copy(), s["vel"].copy()
    for t in range(5):
        frames.append(dict(pos=pos.copy(), vel=vel.copy(), frame_id=t, scene_id="box", box=s["box"], box_normals=s["box_normals"]))
        vel = vel + np.float32(0.0025) * np.array([0, -9.81, 0], np.float32)
        pos = pos + np.float32(0.0025) * vel
    rollouts = []
    real = Simulator.run_rollout

    def run_rollout(self, *a, **kw):
        res = real(self, *a, **kw)
        rollouts.append(res)
        return res

    monkeypatch.setattr(Simulator, "run_rollout", run_rollout)
    model = dict(configs.WATERRAMPS, loss={"weighted_mse": dict(typ="weighted_mse", fac=1000.0, gamma=0.5, neighbor_scale=0.0625)})
    yml = _yaml(tmp_path, model, dict(max_epoch=0, iter=1, windows=[1], window_bnds=[], max_dens_err=0.1,
                                      data_generator=dict(scale=[1.0, 1.0, 0.0], train=dict(stride=1, repeat=True, sample_cnt=3),
                                                          valid=dict(stride=1, time_end=3),
                                                          test=dict(stride=1, time_start=0, time_end=3))))
    loss = run_pipeline.main(["-c", yml, "--split", "train"], data=[frames])
    assert np.isfinite(loss["loss"])
    assert rollouts and all(float(step[0][:, 2].abs().max()) == 0.0 for res in rollouts for scene in res for step in scene)
    ck = os.path.join(str(tmp_path), "logs", "SymNet_canyon_train", "checkpoint", "ckpt-1")
    keys = {k[:-len("/.ATTRIBUTES/VARIABLE_VALUE")] for k in tc.read_index(ck + ".index")}
    want = set(json.load(open(os.path.join(GOLDEN, "ckpt_shapes.json")))["WaterRamps"])
    slots = {f"{k}/.OPTIMIZER_SLOT/optimizer/{s}" for k in want for s in ("m", "v")}
    opt = {"step", "save_counter", "optimizer/iter", "optimizer/beta_1", "optimizer/beta_2", "optimizer/decay"}
    assert keys == want | slots | opt


def _family(name):
    """(model, batch) of a small scene for a model family the recording path covers, weights built."""
    from dmcf_amd import models
    from dmcf_amd.utils import tf_checkpoint as tc
    from tools import configs, scenes
    if name == "PointNet":
        cfg, sc = dict(configs.POINTNET2D), scenes.box_scene(30, h=0.005, dim=2, vel_std=0.05)
    else:
        cfg = dict(configs.BY_NAME[name])
        sc = scenes.box_scene(16, h=0.0125, dim=2) if name == "other/cconv" else scenes.box_scene(16, h=0.005, dim=2)
    cfg["loss"] = {"weighted_mse": dict(typ="weighted_mse", fac=128.0, gamma=0.5, neighbor_scale=0.025)}
    model = getattr(models, cfg["name"])(**cfg)
    if name != "PointNet":
        tc.load_into_model(model, scenes.random_weights(configs.BY_NAME[name], seed=0), device="cuda:0")
    use_acc = cfg.get("use_acc", True) is not False
    g = np.array([0.0, float(cfg["grav"]), 0.0], np.float32)
    pos, vel, frames = sc["pos"].copy(), sc["vel"].copy(), []
    for _ in range(6):
        frames.append((pos.copy(), vel.copy()))
        vel = vel + np.float32(cfg["timestep"]) * g
        pos = pos + np.float32(cfg["timestep"]) * vel
    data = {k: [] for k in ("pos", "vel", "grav", "box", "box_normals", "pre")}
    for f0, n, pre in ((1, 4, 0), (0, 6, 2)):
        data["pos"].append(np.stack([f[0] for f in frames[f0:f0 + n]]))
        data["vel"].append(np.stack([f[1] for f in frames[f0:f0 + n]]))
        data["grav"].append(np.broadcast_to(g, (n,) + sc["pos"].shape).copy() if use_acc else [None])
        data["box"].append(np.stack([sc["box"]] * n))
        data["box_normals"].append(np.stack([sc["box_normals"]] * n))
        data["pre"].append(pre)
    with torch.no_grad():  # (builds the lazily created weights, as run_train's first inference call does)
        grav0 = torch.from_numpy(data["grav"][0][0]).cuda() if use_acc else None
        model([torch.from_numpy(data["pos"][0][0]).cuda(), torch.from_numpy(data["vel"][0][0]).cuda(), grav0, None,
               torch.from_numpy(sc["box"]).cuda(), torch.from_numpy(sc["box_normals"]).cuda()], training=False)
    return model, data


@pytest.mark.parametrize("name", ["other/cconv", "column/hrnet", "PointNet"])
def test_train_step_other_families(tmp_path, name):
    """One train_step of the CConv, HRNet and PointNet families (warm-up with the max_dens_err exit, the recorded window, the
    update): every weight that gets a gradient is a checkpoint variable of the optimizer, gets slots and changes."""
    from dmcf_amd.pipelines import Simulator
    from dmcf_amd.utils import tf_checkpoint as tc
    model, data = _family(name)
    sim = Simulator(model, None, main_log_dir=str(tmp_path), device="cuda", optimizer=LR_CFG)
    variables = tc.model_variables(model)
    assert {id(getattr(m, a)) for _, m, a in variables} == {id(p) for p in model.parameters()}
    before = [getattr(m, a).detach().clone() for _, m, a in variables]
    loss, pres = sim.train_step(data, np.ones(3, np.float32), 0, None, 0.1)
    assert loss.shape == (1,) and np.isfinite(loss).all() and len(pres) == 2 and pres[0] == 0
    slots = sim.optimizer.slots_by_param()
    assert sim.optimizer.iterations == 1 and len(slots) > 0
    changed = 0
    for (key, m, a), b in zip(variables, before):
        p = getattr(m, a)
        if id(p) in slots:
            assert torch.isfinite(p).all(), key
            changed += int(not torch.equal(p.detach(), b))
        else:
            assert p.grad is None and torch.equal(p.detach(), b), key
    assert changed >= len(slots) // 2
