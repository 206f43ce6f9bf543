"""One training step of the shipped model families on the GPU: loss.backward() through every layer, each parameter's gradient
against the same model whose ops.cconv_forward is a float64 torch restatement on the constant pair weights
(tests/cconv_backward_ref.py; the pattern of tests/shims.py), then an Adam step and a two-step unrolled loss."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import cconv_backward_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model(name, weights=None, seed=0):
    from dmcf_amd import models
    from dmcf_amd.utils import tf_checkpoint as tc
    from tools import configs, scenes
    cfg = dict(configs.BY_NAME[name])
    cfg["loss"] = {"weighted_mse": dict(typ="weighted_mse", fac=128.0, gamma=0.5, neighbor_scale=0.025, pre_scale=0.025)}
    model = getattr(models, cfg["name"])(**cfg)
    w = dict(np.load(weights)) if weights else scenes.random_weights(cfg, seed=seed)
    tc.load_into_model(model, w, device="cuda:0")
    return model


def _scene(name):
    from tools import configs, scenes
    if name == "Liquid3d":
        sc = scenes.box_scene(8, h=0.05)
    elif name == "other/cconv":
        sc = scenes.box_scene(16, h=0.0125, dim=2)
    else:
        sc = scenes.box_scene(16, h=0.005, dim=2) if name == "column/hrnet" else scenes.box_scene(16, h=0.01, dim=2)
    # (the configs with use_acc take the per-particle accelerations: gravity)
    grav = None if configs.BY_NAME[name].get("use_acc", True) is False else (0.0, float(configs.BY_NAME[name]["grav"]), 0.0)
    return scenes.model_inputs(sc, device="cuda:0", grav=grav)


def _loss(model, data):
    pos2, vel2 = model(data)
    target = data[0] + 0.5 * model.timestep * data[1] + 1e-3
    loss = model.loss([pos2, vel2], ([data[0]], target, data[0], 0))["weighted_mse"]
    return loss, pos2, vel2


CASES = [("Liquid3d", os.path.join(ROOT, "tests", "golden", "liquid3d_weights.npz")), ("WaterRamps", None),
         ("column/hrnet", None), ("other/cconv", None)]


@pytest.mark.parametrize("name,weights", CASES, ids=[c[0] for c in CASES])
def test_gradients_against_float64_restatement(name, weights, monkeypatch):
    from dmcf_amd import ops
    data = _scene(name)
    model = _model(name, weights)
    with torch.no_grad():
        model(data)  # (builds every lazy weight)
    model.requires_grad_(True)
    assert model.recording()
    loss, _, _ = _loss(model, data)
    assert loss.grad_fn is not None
    model.zero_grad()
    loss.backward()
    got = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    assert got, "no gradients"
    monkeypatch.setattr(ops, "cconv_forward", ref.float64_cconv(ops.cconv_forward))
    model.zero_grad()
    loss_ref, _, _ = _loss(model, data)
    loss_ref.backward()
    assert float(loss) == pytest.approx(float(loss_ref), rel=1e-4)
    for n, p in model.named_parameters():
        if p.grad is None:
            assert n not in got
            continue
        g, r = got[n].double(), p.grad.double()
        assert torch.isfinite(g).all(), n
        assert float((g - r).norm()) <= 2e-3 * float(r.norm()) + 1e-12, (n, float((g - r).norm()), float(r.norm()))


def test_adam_step_and_two_step_unroll():
    data = _scene("Liquid3d")
    model = _model("Liquid3d", os.path.join(ROOT, "tests", "golden", "liquid3d_weights.npz"))
    with torch.no_grad():
        before = model(data)[0].clone()
    model.requires_grad_(True)
    opt, sched = model.get_optimizer({"lr_boundaries": [10], "lr_values": [1e-3, 1e-4]})
    loss, _, _ = _loss(model, data)
    opt.zero_grad()
    loss.backward()
    opt.step()
    sched.step()
    with torch.no_grad():
        after = model(data)[0]
    assert not torch.equal(after, before)
    # two steps unrolled: the second step's inputs are the first step's outputs (gradients through both)
    opt.zero_grad()
    pos2, vel2 = model(data)
    data2 = [pos2, vel2, None, None, data[4], data[5]]
    loss2, _, _ = _loss(model, data2)
    loss2.backward()
    grads = [p.grad for p in model.parameters() if p.grad is not None]
    assert grads and all(torch.isfinite(g).all() for g in grads)
    assert any(float(g.abs().max()) > 0 for g in grads)
    # inference afterwards records nothing
    model.requires_grad_(False)
    out = model(data)[0]
    assert out.grad_fn is None
