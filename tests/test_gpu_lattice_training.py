"""Training through the lattice form: ContinuousConv(record_lattice_form=True) between two grid_pos lattices, and a Liquid3d
training step with model.record_lattice_form(True), against the same layer / model with the flag off (the neighbour-list
form, whose gradients tests/test_gpu_cconv_backward.py and tests/test_gpu_training.py pin).

Layer bar: the operator bar of tests/test_gpu_lattice_backward.py, |err| <= 256 * 2^-24 * A per element against the float64
restatement on the explicit neighbour list.  The stencil form uses the nominal offsets d * voxel where the list form subtracts
rounded positions: dmcf_amd/lattice.py puts that deviation at about 0.6e-6 * |x| / extent of the output; the clouds here keep
|x| / extent <= 2, i.e. 1.2e-6 against a bar of 1.5e-5 of A.  The two HIP forms each meet the bar, so they differ by at most
twice the bar.  Model bar: that of tests/test_gpu_training.py, |g - r| <= 2e-3 |r| per parameter, losses equal to 1e-4."""
import copy
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import cconv_backward_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

K_BAR = 256


def _dev():
    return torch.device("cuda:0")


def _count_calls(monkeypatch):
    from dmcf_amd import ops
    calls = []
    real = ops.lattice_conv_backward

    def counted(*a, **kw):
        calls.append(1)
        return real(*a, **kw)
    monkeypatch.setattr(ops, "lattice_conv_backward", counted)
    return calls


def _cloud(seed=0):
    """A body of 3000 points in a cube of edge 1 and one stray 0.22 away from it: every lattice point has |x| < 1."""
    rng = np.random.default_rng(seed)
    pos = rng.uniform(-0.5, 0.5, size=(3000, 3)).astype(np.float32)
    stray = np.float32([[0.72, 0.1, -0.2]])
    return torch.from_numpy(np.concatenate([pos, stray])).to(_dev())


def _layer(cin, cout, lattice_form):
    from dmcf_amd.utils.convolutions import ContinuousConv
    from dmcf_amd.utils.tools.losses import get_window_func
    return ContinuousConv(name="t", filters=cout, kernel_size=[4, 4, 4], activation=None, align_corners=True,
                          interpolation="linear", coordinate_mapping="ball_to_cube_volume_preserving", normalize=False,
                          window_function=get_window_func("poly6"), use_bias=True, record_lattice_form=lattice_form)


def _layer_grads(conv, F, A, B, extent, G):
    F = F.clone().requires_grad_()
    conv.zero_grad()
    out = conv(F, A, B, extent)
    assert out.grad_fn is not None
    (out * G).sum().backward()
    return out.detach(), conv.kernel.grad.clone(), conv.bias.grad.clone(), F.grad.clone()


PAIRS = [("same", 0.1, 0.1, 0.5, 8, 16), ("coarser", 0.1, 0.2, 0.5, 4, 20), ("finer", 0.2, 0.1, 1.0, 8, 32)]


@pytest.mark.parametrize("tag,v_in,v_out,extent,cin,cout", PAIRS, ids=[p[0] for p in PAIRS])
def test_layer_against_the_list_form(tag, v_in, v_out, extent, cin, cout, monkeypatch):
    from dmcf_amd import lattice, ops
    P = _cloud()
    A = ops.grid_pos(P, np.float32([v_in] * 3), centralize=True)
    B = A if v_in == v_out else ops.grid_pos(P, np.float32([v_out] * 3), centralize=True)
    assert float((torch.cat([A, B]).abs().max())) <= 2.0 * extent  # (|x| / extent <= 2: see the module docstring)
    rng = np.random.default_rng(7)
    F = torch.from_numpy(rng.normal(size=(A.shape[0], cin)).astype(np.float32)).to(_dev())
    G = torch.from_numpy(rng.normal(size=(B.shape[0], cout)).astype(np.float32)).to(_dev())
    on = _layer(cin, cout, True)
    with torch.no_grad():
        on(F, A, B, extent)  # (builds the weights)
        on.kernel.uniform_(-1, 1)
        on.bias.uniform_(-1, 1)
    off = copy.deepcopy(on)
    off.record_lattice_form = False
    for conv in (on, off):
        conv.requires_grad_(True)
    calls = _count_calls(monkeypatch)
    out_off, w_off, b_off, f_off = _layer_grads(off, F, A, B, extent, G)
    assert not calls  # a layer without the flag never takes the new backward
    out_on, w_on, b_on, f_on = _layer_grads(on, F, A, B, extent, G)
    assert len(calls) == 1
    # float64 on the explicit list
    radius = float(np.float32(0.5) * np.float32(extent))
    nns = ops.fixed_radius_search(A, B, radius, return_distances=True)
    pw = ref.PairWeights(B.cpu().numpy(), A.cpu().numpy(), nns.neighbors_index.cpu().numpy(), nns.neighbors_row_splits.cpu().numpy(),
                         extent, [4, 4, 4], window="poly6")
    Wn, Fn, Gn = on.kernel.detach().cpu().numpy(), F.cpu().numpy(), G.cpu().numpy()
    rw, rf, _ = ref.grads(pw, Wn, Fn, Gn)
    aw, af, _ = ref.grads(pw, Wn, Fn, Gn, abs_mode=True)
    ref.check(f"lattice-layer:{tag}:filters", w_on.cpu().numpy(), rw, aw, K_BAR)
    ref.check(f"lattice-layer:{tag}:features", f_on.cpu().numpy(), rf, af, K_BAR)
    ref.check(f"lattice-layer-vs-list:{tag}:filters", w_on.cpu().numpy(), w_off.double().cpu().numpy(), 2.0 * aw, K_BAR)
    ref.check(f"lattice-layer-vs-list:{tag}:features", f_on.cpu().numpy(), f_off.double().cpu().numpy(), 2.0 * af, K_BAR)
    assert torch.equal(b_on, b_off)  # (both: torch's column sum of the same grad_out)
    for k in sorted(k for k in ref.WORST if k.startswith("lattice-layer") and f":{tag}:" in k):
        print(f"{k}: worst err/bar {ref.WORST[k]:.3g}")
    # strays forced (DMCF_LATTICE_CORE_FILL above any fill: every lattice is split into a core and stray rows; the core keeps the
    # slabs with at least half the points of the fullest one, which leaves the stray's out): the layer falls back to the list
    # form as a whole
    monkeypatch.setattr(lattice, "CORE_MIN_FILL", 2.0)
    monkeypatch.setattr(lattice, "CORE_SLAB_FRACTION", 0.5)
    lattice.clear()
    A2 = ops.grid_pos(P, np.float32([v_in] * 3), centralize=True)
    B2 = A2 if v_in == v_out else ops.grid_pos(P, np.float32([v_out] * 3), centralize=True)
    assert torch.equal(A2, A) and torch.equal(B2, B)
    del calls[:]
    out_s, w_s, b_s, f_s = _layer_grads(on, F, A2, B2, extent, G)
    assert not calls
    assert torch.equal(w_s, w_off) and torch.equal(f_s, f_off) and torch.equal(out_s, out_off)


@pytest.fixture(scope="module")
def liquid3d():
    """The Liquid3d case of tests/test_gpu_training.py, recorded once with the flag never set and once with it."""
    from test_gpu_training import ROOT, _loss, _model, _scene
    mp = pytest.MonkeyPatch()
    calls = _count_calls(mp)
    try:
        data = _scene("Liquid3d")
        model = _model("Liquid3d", os.path.join(ROOT, "tests", "golden", "liquid3d_weights.npz"))
        with torch.no_grad():
            model(data)
        model.requires_grad_(True)
        res = {}
        for flag in (None, True):
            if flag is not None:
                assert model.record_lattice_form(flag) > 0
            model.zero_grad()
            del calls[:]
            loss, _, _ = _loss(model, data)
            loss.backward()
            res[flag] = dict(loss=float(loss.detach()), calls=len(calls),
                             grads={n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None})
        return res
    finally:
        mp.undo()


def test_model_without_the_flag_never_calls_the_new_entry_point(liquid3d):
    assert liquid3d[None]["calls"] == 0
    assert liquid3d[None]["grads"]


def test_liquid3d_step_keeps_the_stencil_form(liquid3d):
    off, on = liquid3d[None], liquid3d[True]
    assert on["calls"] >= 1, "no layer took dmcf_lattice_conv_backward"
    assert on["loss"] == pytest.approx(off["loss"], rel=1e-4)
    assert set(on["grads"]) == set(off["grads"])
    for n, r in off["grads"].items():
        g, r = on["grads"][n].double(), r.double()
        assert torch.isfinite(g).all(), n
        assert float((g - r).norm()) <= 2e-3 * float(r.norm()) + 1e-12, (n, float((g - r).norm()), float(r.norm()))
