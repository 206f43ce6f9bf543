"""The batched warm-up (Simulator.warm_up_batched, pipeline key warm_up_batched) against the per-sample loop
(Simulator.warm_up) on the GPU: the same exits, the same states up to the order of float32 additions in the batched kernels,
and the density check through dmcf_frs_window_sum_batched alone.

Fixture: the ``waterramps`` model, items and data of tests/test_gpu_step_batched.py (180, 1 and 260 fluid points over a boundary
slab, random weights), pre = [3, 0, 3], frames p0 + k dt v0.  Item 2's frames are squeezed towards their centroid by SQUEEZE^k
from frame 1 on: the frame's largest density grows away from the prediction's, its density error passes MAX_DENS_ERR and the
sample leaves early, while item 0 runs all its steps.

Chosen on an MI355X from the per-sample loop alone: SQUEEZE = 0.8, MAX_DENS_ERR = 0.25.  The loop's density errors there:
sample 0: 0.07597 (p = 0), 0.20780 (p = 1: above its predecessor, 17 % under the limit), 0.17637 (p = 2: 15 % under its
predecessor) -- it runs all three steps and records pre = 2; sample 2: 0.08496 (p = 0), 0.27255 (p = 1: above its predecessor
and 9 % over the limit) -- it leaves at p = 1 with the state of one step.  (Unsqueezed, sample 2's errors are 0.085, 0.076,
0.122; at 0.85^k 0.085, 0.173, 0.307, which would leave at p = 2 = pre - 1 and record what a whole run records.)  Measured
distance of the batched warm-up's states from the loop's on this fixture: 0 for every sample (bar k * 1e-5 for k steps), and
the batched density errors equal the loop's to the last digit; after 20 steps on 16 WaterRamps-sized scenes
(tools/bench_batched_warm_up.py) the worst distances are 1.3e-6 (positions) and 2.4e-5 (velocities), bar 2e-4."""
import tempfile

import numpy as np
import pytest

import batched_scene as scene

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
R = scene.VOXEL  # particle radius and voxel of the scaled network
DT = 0.0025
PRE = [3, 0, 3]
SQUEEZE = 0.8
MAX_DENS_ERR = 0.25


def _rel(a, b):  # as tests/test_gpu_model.py defines it
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def _model(loss=False):
    from dmcf_amd import models
    from dmcf_amd.utils import tf_checkpoint as tc
    from tools import configs, scenes
    cfg = dict(configs.WATERRAMPS, particle_radii=[R, 2 * R, 4 * R], voxel_size=[R, R, 0.0], window_dens="poly6")
    if loss:
        cfg["loss"] = {"weighted_mse": dict(typ="weighted_mse", fac=128.0, gamma=0.5, neighbor_scale=0.025, pre_scale=0.025)}
    model = getattr(models, cfg["name"])(**cfg)
    tc.load_into_model(model, scenes.random_weights(cfg, seed=4), device=DEV)
    return model


def _data(squeeze=SQUEEZE, frames=7, seed=1):
    """One batch of the data loader's form: per sample ``frames`` frames p0 + k dt v0 (item 2's squeezed from frame 1 on)."""
    rng = np.random.RandomState(seed)
    box, nrm = scene.slab()
    data = dict(pos=[], vel=[], grav=[], box=[], box_normals=[], pre=list(PRE))
    for b, p0 in enumerate(scene.fluid_items()):
        v0 = rng.uniform(-5.0, 5.0, size=p0.shape).astype(np.float32)
        v0[:, 2] = 0.0
        pos = [(p0 + np.float32(k * DT) * v0).astype(np.float32) for k in range(frames)]
        if b == 2:
            pos = [f if k == 0 else (f.mean(0) + np.float32(squeeze ** k) * (f - f.mean(0))).astype(np.float32)
                   for k, f in enumerate(pos)]
        data["pos"].append(pos)
        data["vel"].append([v0] * frames)
        data["grav"].append([None] * frames)
        data["box"].append([box])
        data["box_normals"].append([nrm])
    return data


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


def _recorded(sim, batched, data, max_dens_err):
    """One warm-up with every density error it read (as host floats, in the order of the reads) and the library calls."""
    from dmcf_amd import _lib
    from dmcf_amd.utils.tools import losses
    errors = []
    real = losses.density_loss

    def recording(*a, **k):
        out = real(*a, **k)
        errors.append(out.reshape(-1).tolist())
        return out

    counting = _Counting(_lib.lib())
    mp = pytest.MonkeyPatch()
    try:
        mp.setattr(losses, "density_loss", recording)
        mp.setattr(_lib, "lib", lambda: counting)
        res = (sim.warm_up_batched if batched else sim.warm_up)(data, None, max_dens_err)
    finally:
        mp.undo()
    torch.cuda.synchronize()
    return res, errors, counting.calls


@pytest.fixture(scope="module")
def warm_ups():
    from dmcf_amd.pipelines.simulator import Simulator
    model = _model()
    data = _data()
    sim = Simulator(model, device="cuda", main_log_dir=tempfile.mkdtemp())
    return {batched: _recorded(sim, batched, data, MAX_DENS_ERR) for batched in (False, True)}


def _decisions(errors, pres):
    """The per-sample loop's reads, sample after sample -> ([(sample, p, err, prev)] for every read with p > 0 (a decision),
    the number of steps each sample took: the reads, less the one that made it leave)."""
    out, steps, at = [], [], 0
    for bi, pre in enumerate(PRE):
        reads = min(pre, pres[bi] + 1)
        prev, took = None, 0
        for p in range(reads):
            (err,) = errors[at]
            at += 1
            if p > 0:
                out.append((bi, p, err, prev))
            if not (p > 0 and err > prev and err > MAX_DENS_ERR):
                took += 1
            prev = err
        steps.append(took)
    assert at == len(errors)
    return out, steps


def test_fixture_is_not_borderline(warm_ups):
    """The per-sample loop alone: one sample left early, one ran all its steps, and no decision hangs on a rounding."""
    (_, _, pres), errors, _ = warm_ups[False]
    print("per-sample pre", pres, "density errors", errors)
    left = [bi for bi, pre in enumerate(PRE) if pre and pres[bi] < pre - 1]
    ran = [bi for bi, pre in enumerate(PRE) if pre and pres[bi] == pre - 1]
    assert left and ran, f"fixture is borderline: left {left}, ran all {ran}"
    for bi, p, err, prev in _decisions(errors, pres)[0]:
        print(f"sample {bi} p {p}: err {err:.6g} prev {prev:.6g} limit {MAX_DENS_ERR}")
        assert abs(err - MAX_DENS_ERR) > 1e-3 * MAX_DENS_ERR and abs(err - prev) > 1e-3 * max(abs(prev), abs(err)), \
            f"fixture is borderline: sample {bi} p {p} err {err} prev {prev} limit {MAX_DENS_ERR}"


def test_same_exits_and_states(warm_ups):
    test_fixture_is_not_borderline(warm_ups)
    (want_pos, want_vel, want_pre), want_err, _ = warm_ups[False]
    (got_pos, got_vel, got_pre), got_err, _ = warm_ups[True]
    print("pre looped", want_pre, "batched", got_pre)
    print("density errors looped", want_err, "batched", got_err)
    assert got_pre == want_pre
    worst = 0.0
    steps = _decisions(want_err, want_pre)[1]
    assert steps[1] == 0 and max(steps) == 3
    for bi, k in enumerate(steps):
        assert got_pos[bi].shape == want_pos[bi].shape and got_vel[bi].shape == want_vel[bi].shape
        ep = _rel(got_pos[bi].cpu().numpy(), want_pos[bi].cpu().numpy())
        ev = _rel(got_vel[bi].cpu().numpy(), want_vel[bi].cpu().numpy())
        print(f"sample {bi}: {k} steps, pos rel {ep:.2e}, vel rel {ev:.2e} (bar {k}e-5)")
        worst = max(worst, ep / max(k, 1), ev / max(k, 1))
        assert ep <= k * 1e-5 and ev <= k * 1e-5, (bi, k, ep, ev)  # (no step: frame 0's state, bit for bit)
    print(f"worst rel / steps {worst:.2e}")


def test_density_check_goes_through_the_batched_entry_points(warm_ups):
    _, errors, calls = warm_ups[True]
    _, _, looped = warm_ups[False]
    iterations = len(errors)
    print("iterations", iterations, "batched calls", {k: v for k, v in calls.items() if "frs" in k},
          "looped", {k: v for k, v in looped.items() if "window_sum" in k or k == "dmcf_frs_build"})
    assert 1 <= iterations <= max(PRE)
    assert calls.get("dmcf_frs_window_sum_batched", 0) == 2 * iterations
    assert calls.get("dmcf_frs_window_sum", 0) == 0 and calls.get("dmcf_frs_build", 0) == 0
    # the step's eight structures (tests/test_gpu_step_batched.py) and at most two for the density check
    assert calls.get("dmcf_frs_build_batched", 0) <= (8 + 2) * iterations
    assert looped.get("dmcf_frs_window_sum", 0) >= 2 * iterations and looped.get("dmcf_frs_window_sum_batched", 0) == 0


def test_one_train_step():
    """train_batched + warm_up_batched against train_batched alone: the same pre, the same loss vector."""
    from dmcf_amd.pipelines.simulator import Simulator
    data = _data()
    res = {}
    for batched in (False, True):
        model = _model(loss=True)
        with torch.no_grad():  # builds the lazily created weights before the optimizer takes them
            model.step_batched([[torch.from_numpy(data["pos"][b][0]).to(DEV), torch.from_numpy(data["vel"][b][0]).to(DEV), None,
                                 None, torch.from_numpy(data["box"][b][0]).to(DEV),
                                 torch.from_numpy(data["box_normals"][b][0]).to(DEV)] for b in range(3)], training=False)
        sim = Simulator(model, device="cuda", main_log_dir=tempfile.mkdtemp(), train_batched=True, warm_up_batched=batched,
                        optimizer=dict(lr_boundaries=[20000], lr_values=[0.001, 0.0005]))
        loss, pre = sim.train_step(data, [1.0, 0.5], max_dens_err=MAX_DENS_ERR)
        res[batched] = (loss, list(pre))
        print("warm_up_batched", batched, "loss", loss, "pre", pre, "timing", sim.train_timing)
    assert res[True][1] == res[False][1]
    assert np.isfinite(res[True][0]).all()
    assert res[True][0] == pytest.approx(res[False][0], rel=1e-4)
