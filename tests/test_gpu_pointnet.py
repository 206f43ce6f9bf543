"""PointNet on the GPU: dmcf_neighbor_dense_forward / _backward against the float64 restatement (tests/pointnet_ref.py),
element by element with |err| <= 256 * 2^-24 * A (A the result summed from absolute terms), the inference path, the model
step and a 60-step rollout against the transliteration of models/pointnet.py, the training gradients of every Dense, and
run_pipeline --split test / valid.  The worst err / bar of each group is printed (run with -s to see it)."""
import os

import numpy as np
import pytest
import torch

import pointnet_ref as R

pytestmark = pytest.mark.gpu

EPS = 256 * 2.0 ** -24
WORST = {}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _record(group, err, bar):
    r = float(np.max(err / np.maximum(bar, 1e-30))) if err.size else 0.0
    WORST[group] = max(WORST.get(group, 0.0), r)
    print(f"[pointnet] {group}: worst err/bar so far {WORST[group]:.3g}")
    return r


def _check(group, got, ref, A):
    got = got.detach().double().cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == ref.shape
    err, bar = np.abs(got - ref), EPS * A
    r = _record(group, err, bar)
    assert np.all(err <= bar), (group, r)


def _scene_list(dev, dim, side):
    from dmcf_amd import ops
    from tools import scenes
    h = 0.005 if dim == 2 else 0.05
    sc = scenes.box_scene(side, h=h, dim=dim)
    P = torch.from_numpy(np.concatenate([sc["pos"], sc["box"]])).to(dev)
    nns = ops.fixed_radius_search(P, P, 2 * h, return_distances=False)
    return len(sc["pos"]), P.shape[0], nns.neighbors_index, nns.neighbors_row_splits


def _np(t):
    return t.detach().cpu().numpy()


SHAPES = [(7, 64, False), (64, 128, False), (128, 128, True), (128, 3, False)]


@pytest.mark.parametrize("dim,side", [(2, 30), (3, 10)])
@pytest.mark.parametrize("cin,cout,res", SHAPES)
@pytest.mark.parametrize("relu", [True, False])
def test_forward_against_float64(dev, dim, side, cin, cout, res, relu):
    from dmcf_amd import ops
    n_fluid, n_all, idx, rs = _scene_list(dev, dim, side)
    g = torch.Generator(device="cpu").manual_seed(cin * 1000 + cout)
    # layer-0 style (fluid-only rows addressed by indices over every point) for the 7-wide input, full rows otherwise
    n_x = n_fluid if cin == 7 else n_all
    x = torch.randn(n_x, cin, generator=g).to(dev)
    W = (torch.randn(cin, cout, generator=g) / cin ** 0.5).to(dev)
    b = torch.randn(cout, generator=g).to(dev)
    r = torch.randn(n_all, cout, generator=g).to(dev) if res else None
    y = ops.neighbor_dense(x, W, b, idx, rs, relu=relu, residual=r)
    y2 = ops.neighbor_dense(x, W, b, idx, rs, relu=relu, residual=r)
    assert torch.equal(y, y2)  # two calls, identical bits
    a = (_np(x), _np(W), _np(b), _np(idx), _np(rs))
    ref = R.layer_reference_order(*a, relu=relu, residual=None if r is None else _np(r))
    _check("op forward", y, ref, R.layer_abs(*a, relu=relu, residual=None if r is None else _np(r)))
    # the fused order restated gives the same numbers
    assert np.allclose(R.layer_fused_order(*a, relu=relu), R.layer_reference_order(*a, relu=relu), rtol=1e-10, atol=1e-10)


def test_forward_edge_cases(dev):
    from dmcf_amd import ops
    g = torch.Generator(device="cpu").manual_seed(5)
    x = torch.randn(20, 16, generator=g).to(dev)
    W = torch.randn(16, 24, generator=g).to(dev)
    b = torch.randn(24, generator=g).to(dev)
    # empty rows, out-of-range and negative indices, a row made only of out-of-range indices
    rs = torch.tensor([0, 0, 3, 3, 7, 9, 9, 12], dtype=torch.int64, device=dev)
    idx = torch.tensor([1, 25, 4, -1, 19, 20, 2, 30, 31, 0, 5, 19], dtype=torch.int32, device=dev)
    for relu in (True, False):
        y = ops.neighbor_dense(x, W, b, idx, rs, relu=relu)
        a = (_np(x), _np(W), _np(b), _np(idx), _np(rs))
        ref = R.layer_reference_order(*a, relu=relu)
        _check("op forward", y, ref, R.layer_abs(*a, relu=relu))
        assert torch.all(y[[0, 2, 5]] == 0)  # empty rows and a row of out-of-range pairs: no bias either
    # n_in below the rows of x: indices >= n_in read nothing
    y = ops.neighbor_dense(x, W, b, idx, rs, n_in=10)
    ref = R.layer_reference_order(_np(x), _np(W), _np(b), _np(idx), _np(rs), n_in=10)
    _check("op forward", y, ref, R.layer_abs(_np(x), _np(W), _np(b), _np(idx), _np(rs), n_in=10))
    # n_out = 0
    y = ops.neighbor_dense(x, W, b, idx[:0], torch.zeros(1, dtype=torch.int64, device=dev))
    assert y.shape == (0, 24)
    # n_in = 0: every pair out of range -> zeros, or the residual
    res = torch.randn(7, 24, generator=g).to(dev)
    y = ops.neighbor_dense(x[:0], W, b, idx, rs, residual=res)
    assert torch.equal(y, res)
    # a padded list (a row begin and a row length per row) gives the bits of the CSR list
    from dmcf_amd import ops as O
    P = torch.rand(500, 3, generator=g).to(dev)
    P[:, 2] = 0
    csr = O.fixed_radius_search(P, P, 0.08, return_distances=False)
    pad = O.fixed_radius_search(P, P, 0.08, return_distances=False, row_stride=64)
    assert int(pad.max_count.item()) <= 64
    xi = torch.randn(500, 16, generator=g).to(dev)
    y_csr = ops.neighbor_dense(xi, W, b, csr.neighbors_index, csr.neighbors_row_splits)
    index, begin, _ = pad.raw()
    y_pad = ops.neighbor_dense(xi, W, b, index, begin, neighbors_row_count=pad.row_count)
    assert torch.equal(y_csr, y_pad)


@pytest.mark.parametrize("dim,side", [(2, 30), (3, 10)])
@pytest.mark.parametrize("cin,cout,res", SHAPES)
def test_backward_against_float64(dev, dim, side, cin, cout, res):
    from dmcf_amd import ops
    n_fluid, n_all, idx, rs = _scene_list(dev, dim, side)
    g = torch.Generator(device="cpu").manual_seed(cin + 7 * cout)
    n_x = n_fluid if cin == 7 else n_all
    x = torch.randn(n_x, cin, generator=g).to(dev).requires_grad_(True)
    W = (torch.randn(cin, cout, generator=g) / cin ** 0.5).to(dev).requires_grad_(True)
    b = torch.randn(cout, generator=g).to(dev).requires_grad_(True)
    r = torch.randn(n_all, cout, generator=g).to(dev).requires_grad_(True) if res else None
    G = torch.randn(n_all, cout, generator=g).to(dev)
    grads = []
    for _ in range(2):
        y = ops.neighbor_dense(x, W, b, idx, rs, residual=r)
        assert y.grad_fn is not None
        gs = torch.autograd.grad(y, [x, W, b] + ([r] if res else []), G)
        grads.append(gs)
    for a, c in zip(*grads):
        assert torch.equal(a, c)  # two calls, identical bits
    gx, gW, gb = grads[0][:3]
    xs, Ws, Gs, ii, rr = _np(x), _np(W), _np(G), _np(idx), _np(rs)
    dx, dW, db = R.layer_backward(xs, Ws, Gs, ii, rr)
    Ax, AW, Ab = R.layer_backward(xs, Ws, Gs, ii, rr, absolute=True)
    _check("op backward", gx, dx, Ax)
    _check("op backward", gW, dW, AW)
    _check("op backward", gb, db, Ab)
    if res:
        assert torch.equal(grads[0][3], G)
    # the inference path: same kernel, same bits, no grad_fn
    with torch.no_grad():
        y0 = ops.neighbor_dense(x, W, b, idx, rs, residual=r)
    y1 = ops.neighbor_dense(x.detach(), W.detach(), b.detach(), idx, rs, residual=None if r is None else r.detach())
    assert y0.grad_fn is None and y1.grad_fn is None
    assert torch.equal(y0, y1) and torch.equal(y0, ops.neighbor_dense(x, W, b, idx, rs, residual=r).detach())


def test_backward_out_of_range_pairs_get_no_gradient(dev):
    from dmcf_amd import ops
    g = torch.Generator(device="cpu").manual_seed(9)
    n_fluid, n_all, idx, rs = _scene_list(dev, 2, 20)
    x = torch.randn(n_all, 7, generator=g).to(dev).requires_grad_(True)
    W = torch.randn(7, 64, generator=g).to(dev)
    b = torch.randn(64, generator=g).to(dev)
    G = torch.randn(n_all, 64, generator=g).to(dev)
    shared = ops.SharedInverse(n_all, idx, rs)
    y = ops.neighbor_dense(x, W, b, idx, rs, n_in=n_fluid, inverted=shared)
    (gx,) = torch.autograd.grad(y, [x], G)
    assert torch.all(gx[n_fluid:] == 0)
    dx, _, _ = R.layer_backward(_np(x), _np(W), _np(G), _np(idx), _np(rs), n_in=n_fluid)
    Ax, _, _ = R.layer_backward(_np(x), _np(W), _np(G), _np(idx), _np(rs), n_in=n_fluid, absolute=True)
    _check("op backward", gx, dx, Ax)
    # the shared inversion (over every point) and a layer's own (over its n_in rows) give the same bits
    y = ops.neighbor_dense(x, W, b, idx, rs, n_in=n_fluid)
    (gx2,) = torch.autograd.grad(y, [x], G)
    assert torch.equal(gx, gx2)


# ---- the model ----
def _seeded_weights(model, seed=0):
    rng = np.random.default_rng(seed)
    widths = [7] + list(model.layer_channels)
    w, pairs = {}, []
    for i in range(len(model.layer_channels)):
        k = (rng.normal(size=(widths[i], widths[i + 1])) / np.sqrt(widths[i])).astype(np.float32)
        bb = rng.normal(scale=0.1, size=widths[i + 1]).astype(np.float32)
        w[f"model/denses/{i}/kernel"], w[f"model/denses/{i}/bias"] = k, bb
        pairs.append((k, bb))
    return w, pairs


def _model(dev, **over):
    from dmcf_amd import models
    from dmcf_amd.utils import tf_checkpoint as tc
    from tools import configs
    cfg = dict(configs.POINTNET2D, **over)
    m = models.PointNet(**cfg)
    w, pairs = _seeded_weights(m)
    tc.load_into_model(m, w, device=dev)
    return m, cfg, pairs


def _model_search(model):
    def search(points, radius):
        return _np(model.neighbors_index), _np(model.neighbors_row_splits)
    return search


def _compare_step(tag, model, cfg, pairs, data_np):
    ref = R.PointNetRef(cfg, pairs, _model_search(model))
    pos_ref, _ = ref.step(data_np)
    pc = _np(model.pos_correction).astype(np.float64)
    err = np.abs(pc - ref.pos_correction)
    bar = 1e-5 * np.abs(ref.pos_correction).max() + 1e-5 * np.abs(ref.pos_correction)
    _record(tag, err, bar)
    assert np.all(err <= bar), tag
    assert np.array_equal(_np(model.num_fluid_neighbors), ref.num_fluid_neighbors)


@pytest.mark.parametrize("over", [{}, {"use_bnds": False}, {"out_activation": "tanh"}])
def test_model_step_against_transliteration(dev, over):
    from tools import scenes
    model, cfg, pairs = _model(dev, **over)
    sc = scenes.box_scene(40, h=0.005, dim=2, vel_std=0.05)
    data_np = scenes.model_inputs(sc, grav=[0.0, -9.81, 0.0])
    data = scenes.model_inputs(sc, device=dev, grav=[0.0, -9.81, 0.0])
    with torch.no_grad():
        model(data, training=False)
    nn_mean = float(np.diff(_np(model.neighbors_row_splits)).mean())
    assert 8 < nn_mean < 16
    _compare_step("model step", model, cfg, pairs, data_np)


def test_inference_step_is_five_launches(dev):
    from dmcf_amd import ops
    from tools import scenes
    model, _, _ = _model(dev)
    data = scenes.model_inputs(scenes.box_scene(60, h=0.005, dim=2), device=dev, grav=[0.0, -9.81, 0.0])
    ops.timer = ops.LaunchTimer()
    try:
        with torch.no_grad():
            model(data, training=False)
        torch.cuda.synchronize()
        kinds = [m for k, m, _ in ops.timer.results() if k == "neighbor_dense"]
    finally:
        ops.timer = None
    assert len(kinds) == 5
    assert all(m["kernel"].count(";") == 0 for m in kinds)


def test_rollout_60_steps(dev):
    from dmcf_amd.pipelines import Simulator
    from tools import scenes
    model, cfg, pairs = _model(dev)
    sc = scenes.box_scene(30, h=0.005, dim=2, vel_std=0.05)
    n = len(sc["pos"])
    inp = dict(pos=sc["pos"][None], vel=sc["vel"][None], grav=np.broadcast_to(np.float32([0, -9.81, 0]), (1, n, 3)).copy(),
               box=sc["box"][None], box_normals=sc["box_normals"][None])
    sim = Simulator(model, device="cuda")
    res = sim.run_rollout([inp], timesteps=61)[0]
    assert len(res) == 61
    for t in (0, 30, 59):
        state = [None if a is None else a for a in res[t]]
        data_np = [None if a is None else _np(a) for a in state]
        with torch.no_grad():
            pos, _ = model(state, training=False)
        assert torch.equal(pos, res[t + 1][0])  # the step is deterministic: the rollout's own step again
        _compare_step("rollout", model, cfg, pairs, data_np)


def test_training_gradients_of_every_dense(dev):
    """weighted_mse of one step; every dense{i} gradient against the same step restated in float64 torch (Dense then
    gather, index_add in the reference's order, on the model's own list), then one Adam step changes the output."""
    from tools import scenes
    model, cfg, pairs = _model(dev, loss={"weighted_mse": dict(typ="weighted_mse", fac=1000.0, gamma=0.5, neighbor_scale=0.0625)})
    sc = scenes.box_scene(30, h=0.005, dim=2, vel_std=0.05)
    data = scenes.model_inputs(sc, device=dev, grav=[0.0, -9.81, 0.0])
    target = data[0] + 0.0025 * data[1] + 1e-5
    model.requires_grad_(True)
    out = model(data, training=True)
    loss = model.loss(out, (data, target, None, 0))["weighted_mse"]
    loss.backward()
    # float64 restatement
    idx = model.neighbors_index.long()
    rs = model.neighbors_row_splits
    n_out = rs.shape[0] - 1
    row = torch.repeat_interleave(torch.arange(n_out, device=dev), torch.diff(rs))
    pos, vel, acc = (t.double() for t in data[:3])
    dt = 0.0025
    vel2 = vel + dt * acc
    pos2 = pos + dt * vel2
    x = torch.cat([torch.ones_like(pos2[:, :1]), vel2, acc], dim=-1)
    ws = [(torch.from_numpy(k).double().to(dev).requires_grad_(True), torch.from_numpy(b).double().to(dev).requires_grad_(True))
          for k, b in pairs]
    ans = x
    for W, b in ws:
        d = torch.relu(ans) @ W + b
        ok = idx < d.shape[0]
        s = torch.zeros(n_out, W.shape[1], dtype=torch.float64, device=dev).index_add_(0, row[ok], d[idx[ok]])
        ans = s + ans if s.shape == ans.shape else s
    pc = torch.tensor(cfg["out_scale"], dtype=torch.float64, device=dev) * ans[:pos.shape[0]]
    pred = pos2 + pc
    loss64 = model.loss_fn["weighted_mse"](target.double(), pred, num_fluid_neighbors=model.num_fluid_neighbors)
    gs = torch.autograd.grad(loss64, [t for wb in ws for t in wb])
    for i, dense in enumerate(model.denses):
        for got, want in ((dense.kernel.grad, gs[2 * i]), (dense.bias.grad, gs[2 * i + 1])):
            w = _np(want)
            err = np.abs(_np(got).astype(np.float64) - w)
            bar = 1e-4 * np.abs(w).max() + 1e-4 * np.abs(w)
            _record("training grads", err, bar)
            assert np.all(err <= bar), i
    opt, _ = model.get_optimizer({"lr_boundaries": [1000], "lr_values": [1e-3, 1e-4]})
    before = model(data, training=False)[0].detach().clone()
    opt.step()
    with torch.no_grad():
        after = model(data, training=False)[0]
    assert not torch.equal(before, after)
    model.requires_grad_(False)


def _scene_dir(tmp_path):
    from dmcf_amd.datasets.dataset_reader_physics import write_scene
    from tools import scenes
    sc = scenes.box_scene(20, h=0.005, dim=2, vel_std=0.05)
    frames, pos, vel = [], sc["pos"].copy(), sc["vel"].copy()
    for t in range(4):
        f = dict(frame_id=t, scene_id="box2d", pos=pos.copy(), vel=vel.copy(), grav=np.float32([0, -9.81, 0]),
                 m=np.ones(len(pos), np.float32), viscosity=np.zeros(len(pos), np.float32))
        if t == 0:
            f.update(box=sc["box"], box_normals=sc["box_normals"])
        frames.append(f)
        vel = (vel + np.float32(0.0025) * np.float32([0, -9.81, 0])).astype(np.float32)
        pos = (pos + np.float32(0.0025) * vel).astype(np.float32)
    d = tmp_path / "data"
    d.mkdir()
    write_scene(str(d / "box2d.msgpack.zst"), frames)
    return str(d)


@pytest.mark.parametrize("split", ["test", "valid"])
def test_run_pipeline(dev, tmp_path, monkeypatch, split):
    import glob
    import yaml
    from dmcf_amd import pipelines, run_pipeline
    from dmcf_amd.utils import tf_checkpoint as tc
    from tools import configs

    def load_ckpt(self, path):
        tc.load_into_model(self.model, _seeded_weights(self.model)[0], device=dev)
        return 0

    monkeypatch.setattr(pipelines.Simulator, "load_ckpt", load_ckpt)
    model = dict(configs.POINTNET2D, ckpt_path=None, window_dens="poly6",
                 loss={"weighted_mse": dict(typ="weighted_mse", fac=1000.0, gamma=0.5, neighbor_scale=0.0625)})
    cfg = dict(dataset=dict(name="ComplexData"), model=model,
               pipeline=dict(name="Simulator", version="2d", main_log_dir=str(tmp_path / "logs"), output_dir=str(tmp_path / "out"),
                             data_generator=dict(translate=[-0.5, -0.5, 0.0], scale=[1.0, 1.0, 0.0], train=dict(stride=1),
                                                 valid=dict(stride=1, time_end=3), test=dict(stride=1, time_start=0, time_end=3))))
    yml = tmp_path / "pointnet.yml"
    yml.write_text(yaml.safe_dump(cfg))
    got = run_pipeline.main(["-c", str(yml), "--split", split, "--dataset_path", _scene_dir(tmp_path)])
    if split == "valid":
        for k in ("mse_val", "chamfer_val", "chamfer_val_2", "emd", "loss"):
            assert k in got and np.isfinite(got[k]), k
    else:
        assert len(got) == 1 and os.path.exists(got[0])
        assert glob.glob(os.path.join(str(tmp_path / "out"), "**", "*"), recursive=True)
