"""Training through the particles -> lattice layers: ContinuousConv(record_scatter_form=True) from a particle cloud onto a
grid_pos lattice with 4 or 8 output channels, and a Liquid3d training step with model.record_scatter_form(True), against the same
layer / model with the flag off (the neighbour-list route with its list inversion, whose gradients
tests/test_gpu_cconv_backward.py and tests/test_gpu_training.py pin).

Layer bar: the operator bar of tests/test_gpu_cconv_scatter_backward.py without its fixed-point term (a stricter bar),
|err| <= 256 * 2^-24 * A per element against the float64 restatement on the explicit forward list; the two HIP routes each meet
it, so they differ by at most twice the bar.  Model bar: that of tests/test_gpu_training.py, |g - r| <= 2e-3 |r| per parameter,
losses equal to 1e-4."""
import copy
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import cconv_backward_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

K_BAR = 256
SIDE = 12  # fluid particles per edge of the model test's box: enough for an inference step to take splat S at SCATTER_MIN_INPUTS = 256


def _dev():
    return torch.device("cuda:0")


def _count_calls(monkeypatch, name):
    from dmcf_amd import ops
    calls = []
    real = getattr(ops, name)

    def counted(*a, **kw):
        calls.append(1)
        return real(*a, **kw)
    monkeypatch.setattr(ops, name, counted)
    return calls


def _cloud(seed=0):
    """A body of 3000 points in a cube of edge 1 and one stray 0.22 away from it."""
    rng = np.random.default_rng(seed)
    pos = rng.uniform(-0.5, 0.5, size=(3000, 3)).astype(np.float32)
    stray = np.float32([[0.72, 0.1, -0.2]])
    return torch.from_numpy(np.concatenate([pos, stray])).to(_dev())


def _layer(cout, scatter_form):
    from dmcf_amd.utils.convolutions import ContinuousConv
    from dmcf_amd.utils.tools.losses import get_window_func
    return ContinuousConv(name="t", filters=cout, kernel_size=[4, 4, 4], activation=None, align_corners=True,
                          interpolation="linear", coordinate_mapping="ball_to_cube_volume_preserving", normalize=False,
                          window_function=get_window_func("poly6"), use_bias=True, record_scatter_form=scatter_form)


def _layer_grads(conv, F, A, B, extent, G):
    F = F.clone().requires_grad_()
    conv.zero_grad()
    out = conv(F, A, B, extent)
    assert out.grad_fn is not None
    (out * G).sum().backward()
    return out.detach(), conv.kernel.grad.clone(), conv.bias.grad.clone(), F.grad.clone()


def _pair(cin, cout, seed=7):
    from dmcf_amd import ops
    P = _cloud()
    B = ops.grid_pos(P, np.float32([0.2] * 3), centralize=True)
    rng = np.random.default_rng(seed)
    F = torch.from_numpy(rng.normal(size=(P.shape[0], cin)).astype(np.float32)).to(_dev())
    G = torch.from_numpy(rng.normal(size=(B.shape[0], cout)).astype(np.float32)).to(_dev())
    on = _layer(cout, True)
    with torch.no_grad():
        on(F, P, B, 0.8)  # (builds the weights)
        on.kernel.uniform_(-1, 1)
        on.bias.uniform_(-1, 1)
    off = copy.deepcopy(on)
    off.record_scatter_form = False
    for conv in (on, off):
        conv.requires_grad_(True)
    return P, B, F, G, on, off


@pytest.mark.parametrize("cin,cout", [(24, 4), (16, 8)], ids=["24to4", "16to8"])
def test_layer_against_the_list_route(cin, cout, monkeypatch):
    from dmcf_amd import ops
    from dmcf_amd.utils import convolutions
    monkeypatch.setattr(convolutions, "SCATTER_MIN_INPUTS", 256)
    extent = 0.8  # radius 0.4: reach 2 on the 0.2 lattice
    P, B, F, G, on, off = _pair(cin, cout)
    assert B.shape[0] * 4 <= P.shape[0]
    # what the forward inside the node is: splat S where inference takes it (4 output channels), else the list form
    with torch.no_grad():
        assert (on._scatter_form(F, P, B, None, None, 0.4) is not None) == (cout == 4)
    new, inv = _count_calls(monkeypatch, "cconv_scatter_backward"), _count_calls(monkeypatch, "invert_neighbors_list")
    out_off, w_off, b_off, f_off = _layer_grads(off, F, P, B, extent, G)
    assert not new and len(inv) == 1  # a layer without the flag never takes the new backward
    del inv[:]
    ops.timer = ops.LaunchTimer()
    try:
        out_on, w_on, b_on, f_on = _layer_grads(on, F, P, B, extent, G)
        torch.cuda.synchronize()
        fwd = [m.get("kernel", "") for k, m, _ in ops.timer.results() if k == "cconv"]
        bwd = [m.get("kernel", "") for k, m, _ in ops.timer.results() if k == "cconv_backward"]
    finally:
        ops.timer = None
    assert len(new) == 1 and not inv
    assert bwd == ["cconv_sct_bwd"] and len(fwd) == 1 and fwd[0].startswith("cconv_sct_kernel") == (cout == 4), (fwd, bwd)
    # float64 on the explicit forward list
    nns = ops.fixed_radius_search(P, B, 0.4, return_distances=True)
    pw = ref.PairWeights(B.cpu().numpy(), P.cpu().numpy(), nns.neighbors_index.cpu().numpy(), nns.neighbors_row_splits.cpu().numpy(),
                         extent, [4, 4, 4], window="poly6")
    Wn, Fn, Gn = on.kernel.detach().cpu().numpy(), F.cpu().numpy(), G.cpu().numpy()
    rw, rf, _ = ref.grads(pw, Wn, Fn, Gn)
    aw, af, _ = ref.grads(pw, Wn, Fn, Gn, abs_mode=True)
    tag = f"{cin}to{cout}"
    assert torch.allclose(out_on, out_off, rtol=0, atol=1e-4 * float(out_off.abs().max()))
    ref.check(f"scatter-layer:{tag}:filters", w_on.cpu().numpy(), rw, aw, K_BAR)
    ref.check(f"scatter-layer:{tag}:features", f_on.cpu().numpy(), rf, af, K_BAR)
    ref.check(f"scatter-layer-vs-list:{tag}:filters", w_on.cpu().numpy(), w_off.double().cpu().numpy(), 2.0 * aw, K_BAR)
    ref.check(f"scatter-layer-vs-list:{tag}:features", f_on.cpu().numpy(), f_off.double().cpu().numpy(), 2.0 * af, K_BAR)
    assert torch.equal(b_on, b_off)  # (both: torch's column sum of the same grad_out)
    for k in sorted(k for k in ref.WORST if k.startswith("scatter-layer") and f":{tag}:" in k):
        print(f"{k}: worst err/bar {ref.WORST[k]:.3g}")


def test_ineligible_layer_keeps_the_list_route(monkeypatch):
    """16 output channels: the flag changes nothing, bit for bit."""
    from dmcf_amd.utils import convolutions
    monkeypatch.setattr(convolutions, "SCATTER_MIN_INPUTS", 256)
    P, B, F, G, on, off = _pair(24, 16)
    new = _count_calls(monkeypatch, "cconv_scatter_backward")
    res_off = _layer_grads(off, F, P, B, 0.8, G)
    res_on = _layer_grads(on, F, P, B, 0.8, G)
    assert not new
    for a, b in zip(res_on, res_off):
        assert torch.equal(a, b)


def test_user_supplied_list_keeps_the_list_route(monkeypatch):
    from dmcf_amd import ops
    P, B, F, G, on, off = _pair(24, 4)
    new = _count_calls(monkeypatch, "cconv_scatter_backward")
    nns = ops.fixed_radius_search(P, B, 0.4, return_distances=False)
    Fg = F.clone().requires_grad_()
    out = on(Fg, P, B, 0.8, user_neighbors_index=nns.neighbors_index, user_neighbors_row_splits=nns.neighbors_row_splits)
    (out * G).sum().backward()
    assert not new and Fg.grad is not None


@pytest.fixture(scope="module")
def liquid3d():
    """The Liquid3d model of tests/test_gpu_training.py on a box big enough for splat S, recorded once with the flag never set
    and once with it."""
    from dmcf_amd import ops
    from dmcf_amd.utils import convolutions
    from test_gpu_training import ROOT, _loss, _model
    from tools import configs, scenes
    mp = pytest.MonkeyPatch()
    mp.setattr(convolutions, "SCATTER_MIN_INPUTS", 256)
    calls, inv = _count_calls(mp, "cconv_scatter_backward"), _count_calls(mp, "invert_neighbors_list")
    try:
        grav = (0.0, float(configs.BY_NAME["Liquid3d"]["grav"]), 0.0)
        data = scenes.model_inputs(scenes.box_scene(SIDE, h=0.05), device="cuda:0", grav=grav)
        model = _model("Liquid3d", os.path.join(ROOT, "tests", "golden", "liquid3d_weights.npz"))
        ops.timer = ops.LaunchTimer()
        try:
            with torch.no_grad():
                model(data)
            torch.cuda.synchronize()
            infer = [m.get("kernel", "") for k, m, _ in ops.timer.results() if k == "cconv"]
        finally:
            ops.timer = None
        model.requires_grad_(True)
        res = {"infer": infer}
        for flag in (None, True):
            if flag is not None:
                assert model.record_scatter_form(flag) > 0
            model.zero_grad()
            del calls[:], inv[:]
            loss, _, _ = _loss(model, data)
            loss.backward()
            res[flag] = dict(loss=float(loss.detach()), calls=len(calls), inversions=len(inv),
                             grads={n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None})
        return res
    finally:
        mp.undo()


def test_the_box_is_big_enough_for_the_scatter_form(liquid3d):
    """Otherwise the cases below would compare the list route with itself."""
    assert any(k.startswith("cconv_sct_kernel") for k in liquid3d["infer"]), sorted(set(liquid3d["infer"]))


def test_model_without_the_flag_never_calls_the_new_entry_point(liquid3d):
    assert liquid3d[None]["calls"] == 0
    assert liquid3d[None]["grads"]


def test_liquid3d_step_takes_the_scatter_backward(liquid3d):
    off, on = liquid3d[None], liquid3d[True]
    assert on["calls"] >= 1, "no layer took dmcf_cconv_scatter_backward"
    assert on["inversions"] < off["inversions"], (on["inversions"], off["inversions"])  # the new route inverts no list
    assert on["loss"] == pytest.approx(off["loss"], rel=1e-4)
    assert set(on["grads"]) == set(off["grads"])
    for n, r in off["grads"].items():
        g, r = on["grads"][n].double(), r.double()
        assert torch.isfinite(g).all(), n
        assert float((g - r).norm()) <= 2e-3 * float(r.norm()) + 1e-12, (n, float((g - r).norm()), float(r.norm()))
