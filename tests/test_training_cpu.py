"""CPU checks of the training surface: the losses (utils/tools/losses.py:47-110 of the reference), the optimizer's learning-rate
schedule, PBFNet.loss on a SymNet config, and the float64 backward reference the GPU tests compare against
(tests/cconv_backward_ref.py) -- its forward against the oracle, its gradients against the adjoint identities."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")


def _np_losses(typ, target, pred, kw, **cfg):
    """numpy restatement of losses.py:47-110."""
    gamma = cfg.get("gamma", 0.5)
    pre_f = np.exp(-cfg.get("pre_scale", 0.0) * float(kw["pre_steps"]))
    if typ in ("mse", "weighted_mse"):
        diff = (np.sum((target - pred) ** 2, axis=-1) + 1e-9) ** gamma
        imp = np.exp(-cfg.get("neighbor_scale", 1.0) * kw["num_fluid_neighbors"]) if typ == "weighted_mse" else 1.0
        return cfg.get("fac", 1.0) * np.mean(pre_f * imp * diff)
    if typ in ("vel", "weighted_vel"):
        inp, prev = kw["input"][0], kw["target_prev"]
        diff = (np.sum(((target - prev) - (pred - inp)) ** 2, axis=-1) + 1e-9) ** gamma
        imp = np.exp(-cfg.get("neighbor_scale", 1.0) * kw["num_fluid_neighbors"]) if typ == "weighted_vel" else 1.0
        return cfg.get("fac", 1.0) * np.mean(imp * diff)
    if typ == "momentum":
        return cfg.get("fac", 1.0) * np.mean(kw["pos_correction"])
    raise AssertionError(typ)


@pytest.mark.parametrize("typ,cfg", [
    ("mse", {}), ("mse", dict(fac=2.0, gamma=1.0, pre_scale=0.3)),
    ("weighted_mse", dict(fac=128.0, neighbor_scale=0.025, pre_scale=0.025, gamma=0.5)),
    ("vel", dict(gamma=0.75)), ("weighted_vel", dict(neighbor_scale=0.1)), ("momentum", dict(fac=3.0)),
])
def test_get_loss_matches_numpy(typ, cfg):
    from dmcf_amd.utils.tools.losses import get_loss
    rng = np.random.default_rng(0)
    n = 500
    target, pred, inp, prev, corr = (rng.normal(size=(n, 3)) for _ in range(5))
    nfn = rng.integers(0, 40, size=n).astype(np.float64)
    kw = dict(num_fluid_neighbors=nfn, input=[inp], target_prev=prev, pre_steps=3, pos_correction=corr)
    f = get_loss(typ, **cfg)
    tkw = dict(num_fluid_neighbors=torch.from_numpy(nfn).float(), input=[torch.from_numpy(inp).float()],
               target_prev=torch.from_numpy(prev).float(), pre_steps=3, pos_correction=torch.from_numpy(corr).float())
    got = float(f(torch.from_numpy(target).float(), torch.from_numpy(pred).float(), **tkw))
    assert got == pytest.approx(_np_losses(typ, target, pred, kw, **cfg), rel=1e-5)


@pytest.mark.parametrize("typ", ["dense", "chamfer", "emd", "hist"])
def test_unimplemented_losses_raise(typ):
    from dmcf_amd.utils.tools.losses import get_loss
    f = get_loss(typ)
    with pytest.raises(NotImplementedError):
        f(torch.zeros(3, 3), torch.zeros(3, 3))


def test_optimizer_schedule():
    from dmcf_amd.utils.tools.losses import get_optimizer
    w = torch.nn.Parameter(torch.zeros(3))
    opt, sched = get_optimizer([w], {"lr_boundaries": [2, 4], "lr_values": [1e-3, 5e-4, 1e-4]})
    assert isinstance(opt, torch.optim.Adam) and opt.defaults["eps"] == 1e-6
    lrs = []
    for _ in range(7):
        lrs.append(opt.param_groups[0]["lr"])
        w.grad = torch.ones(3)
        opt.step()
        sched.step()
    # Keras PiecewiseConstantDecay: values[0] up to and including step boundaries[0], values[1] up to boundaries[1], ...
    assert lrs == pytest.approx([1e-3, 1e-3, 1e-3, 5e-4, 5e-4, 1e-4, 1e-4], rel=1e-12)
    with pytest.raises(ValueError):
        get_optimizer([w], {"lr_boundaries": [2, 4], "lr_values": [1e-3]})


def test_symnet_loss_from_config():
    from dmcf_amd import models
    from tools import configs
    cfg = dict(configs.BY_NAME["Liquid3d"])
    cfg["loss"] = {"weighted_mse": dict(typ="weighted_mse", fac=128.0, gamma=0.5, neighbor_scale=0.025, pre_scale=0.025),
                   "momentum": dict(typ="momentum", fac=1.0)}
    model = getattr(models, cfg["name"])(**cfg)
    assert list(model.loss_keys()) == ["weighted_mse", "momentum"]
    rng = np.random.default_rng(1)
    n = 64
    pred, target, prev, inp = (torch.from_numpy(rng.normal(size=(n, 3)).astype(np.float32)) for _ in range(4))
    model.num_fluid_neighbors = torch.from_numpy(rng.integers(0, 30, size=n).astype(np.float32))
    model.pos_correction = torch.from_numpy(rng.normal(size=(n, 3)).astype(np.float32))
    loss = model.loss([pred, None], ([inp], target, prev, 2))
    kw = dict(num_fluid_neighbors=model.num_fluid_neighbors.numpy(), input=[inp.numpy()], target_prev=prev.numpy(), pre_steps=2,
              pos_correction=model.pos_correction.numpy())
    assert float(loss["weighted_mse"]) == pytest.approx(
        _np_losses("weighted_mse", target.numpy(), pred.numpy(), kw, fac=128.0, neighbor_scale=0.025, pre_scale=0.025), rel=1e-5)
    assert float(loss["momentum"]) == pytest.approx(_np_losses("momentum", target.numpy(), pred.numpy(), kw), rel=1e-5)
    assert model.recording() is False  # weights are built with requires_grad=False


def _brute_list(pos, radius, ignore_query_point=False):
    d2 = ((pos[:, None, :] - pos[None, :, :]) ** 2).sum(-1)
    n = len(pos)
    rows = [np.nonzero((d2[i] <= radius * radius) & ~((np.arange(n) == i) & ignore_query_point))[0] for i in range(n)]
    rs = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return np.concatenate(rows).astype(np.int32), rs


@pytest.mark.parametrize("case", [
    dict(), dict(window="cubic", normalize=True),
    dict(mapping="ball_to_cube_radial", interpolation="linear_border", align_corners=False),
    dict(interpolation="nearest_neighbor"), dict(imp=True), dict(shape=(1, 8, 8), dims=2),
    dict(symmetric=True, sym_axis=1), dict(symmetric=True, sym_axis=2, shape=(1, 8, 4), dims=2),
])
def test_float64_reference_forward_and_adjoint(oracle, case):
    import cconv_backward_ref as ref
    rng = np.random.default_rng(2)
    n, radius, cin, cout = 150, 0.25, 3, 4
    pos = rng.uniform(0, 1, size=(n, 3)).astype(np.float32)
    if case.get("dims") == 2:
        pos[:, 2] = 0
    sym = case.get("symmetric", False)
    shape = case.get("shape", (6, 3, 6) if sym else (4, 4, 4))
    full = list(shape)
    if sym:
        full[case["sym_axis"]] *= 2
    feat = rng.normal(size=(n, cin)).astype(np.float32)
    filt = rng.uniform(-1, 1, size=(*shape, cin, cout)).astype(np.float32)
    imp = rng.uniform(0.5, 1.5, size=n).astype(np.float32) if case.get("imp") else None
    idx, rs = _brute_list(pos, radius, ignore_query_point=sym)
    window = case.get("window", "poly6")
    mapping = case.get("mapping", "ball_to_cube_volume_preserving")
    interp = case.get("interpolation", "linear")
    align = case.get("align_corners", True)
    normalize = case.get("normalize", False)
    extent = 2 * radius
    pw = ref.PairWeights(pos, pos, idx, rs, extent, full, window=window, inp_importance=imp, align_corners=align,
                         mapping=mapping, interpolation=interp)
    kw = dict(normalize=normalize, symmetric=sym, sym_axis=case.get("sym_axis", 2))
    G = rng.normal(size=(n, cout))
    dW, dF, out = ref.grads(pw, filt, feat, G, **kw)
    # forward == the oracle's float64 restatement
    d2 = ((pos[idx] - np.repeat(pos, np.diff(rs), axis=0)) ** 2).sum(-1).astype(np.float32)
    nimp = oracle.window(window, d2 / np.float32(radius) ** 2)
    W_full = oracle.mirror_kernel(filt, case["sym_axis"]) if sym else filt
    okw = dict(inp_importance=imp, align_corners=align, coordinate_mapping=mapping, interpolation=interp, f64=True)
    want = oracle.continuous_conv(W_full, pos, extent, pos, feat, idx, rs, nimp, normalize=normalize, **okw)
    if sym:
        # ASCC: out_i = sum_p a_p g(r_p) (f_j + f_i): the centre part, channel by channel, from calls on features of ones
        for c in range(cin):
            gc = oracle.continuous_conv(np.ascontiguousarray(W_full[..., c:c + 1, :]), pos, extent, pos,
                                        np.ones((n, 1), np.float32), idx, rs, nimp, **okw)
            want = want + feat[:, c:c + 1] * gc
    assert np.abs(out - want).max() <= 1e-5 * np.abs(want).max()
    # adjoint identities: <G, conv(f)> = <dF, f>, <G, conv_W(f)> = <dW, W>
    lhs = float((G * out).sum())
    assert float((dF * feat).sum()) == pytest.approx(lhs, rel=1e-10)
    assert float((dW * filt).sum()) == pytest.approx(lhs, rel=1e-10)
