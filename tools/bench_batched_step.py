"""Time the forward and backward of ONE recorded window step of a training batch, sample by sample (the loop of
pipelines/simulator.py: Simulator.window_loss) against the same batch in one pass of the network (PBFNet.step_batched, the
pipeline key train_batched):

  the WaterRamps network (tools/configs.py, random weights) on 16 scenes of 2,025 particles -- a 45 x 45 jittered lattice of
  spacing 0.01, the scene of tools/bench_batched_search.py -- each over a boundary of two rows of 0.005-spaced points

HIP events around each variant, a warm-up, the two variants alternating in one process; medians of 15.  Both variants include
what they cost the host.  Beside the times: the library entry points each variant calls per step, and the device kernels it
dispatches (torch.profiler; left out if the profiler is not available).  Prints one JSON line and writes the table to
``--out`` (default profiles/batched_step.md)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dmcf_amd import _lib, models, ops  # noqa: E402,F401
from dmcf_amd.utils import tf_checkpoint as tc  # noqa: E402
from tools import configs, scenes  # noqa: E402
from tools.bench_batched_search import timed_pair  # noqa: E402


def scene_items(dev, n_items=16):
    rng = np.random.default_rng(0)
    g = (np.stack(np.meshgrid(np.arange(45), np.arange(45), indexing="ij"), -1).reshape(-1, 2) + 0.5) * 0.01
    x = np.arange(-4, 95, dtype=np.float32) * 0.005
    box = np.concatenate([np.stack([x, np.full_like(x, y), np.zeros_like(x)], -1) for y in (-0.005, -0.010)]).astype(np.float32)
    nrm = np.tile(np.float32([[0.0, 1.0, 0.0]]), (box.shape[0], 1))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)  # noqa: E731
    items = []
    for _ in range(n_items):
        p = np.zeros((2025, 3), np.float32)
        p[:, :2] = g + rng.uniform(-0.003, 0.003, size=g.shape)
        v = np.zeros_like(p)
        v[:, :2] = rng.uniform(-0.5, 0.5, size=g.shape)
        items.append([t(p), t(v), None, None, t(box), t(nrm)])
    return items


class Counting:
    def __init__(self, real):
        self._real, self.calls = real, 0

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("dmcf_") or name in ("dmcf_error_string", "dmcf_last_hip_error") or name.endswith("_bytes"):
            return fn

        def counted(*a):
            self.calls += 1
            return fn(*a)
        return counted


def library_calls(fn):
    real = _lib.lib
    counting = Counting(real())
    _lib.lib = lambda: counting
    try:
        fn()
    finally:
        _lib.lib = real
    return counting.calls


def kernel_dispatches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")
                   and not e.name.startswith(("Memcpy", "Memset")))
    except Exception as err:  # noqa: BLE001  (a figure beside the result, not the result)
        print(f"kernel count left out: {type(err).__name__}: {err}", file=sys.stderr)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batched_step.md"))
    ap.add_argument("--items", type=int, default=16)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = dict(configs.WATERRAMPS)
    cfg["loss"] = {"weighted_mse": dict(typ="weighted_mse", fac=128.0, gamma=0.5, neighbor_scale=0.025, pre_scale=0.025)}
    model = getattr(models, cfg["name"])(**cfg)
    tc.load_into_model(model, scenes.random_weights(cfg, seed=0), device=dev)
    items = scene_items(dev, args.items)
    targets = [it[0] + 0.5 * model.timestep * it[1] + 1e-4 for it in items]
    model.requires_grad_(True)

    def item_loss(pos2, vel2, it, target):
        return model.loss([pos2, vel2], [it, target, it[0], 0])["weighted_mse"]

    def looped():
        model.zero_grad()
        total = 0.0
        for it, target in zip(items, targets):
            pos2, vel2 = model(it, training=True)
            total = total + item_loss(pos2, vel2, it, target)
        total.backward()
        return total

    def batched():
        model.zero_grad()
        pos2, vel2, rs = model.step_batched(items, training=True)
        correction, neighbors = model.pos_correction, model.num_fluid_neighbors
        total = 0.0
        for b, (it, target) in enumerate(zip(items, targets)):
            a, e = rs[b], rs[b + 1]
            model.pos_correction, model.num_fluid_neighbors = correction[a:e], neighbors[a:e]
            total = total + item_loss(pos2[a:e], vel2[a:e], it, target)
        model.pos_correction, model.num_fluid_neighbors = correction, neighbors
        total.backward()
        return total

    loss_l = float(looped())
    grads_l = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    loss_b = float(batched())
    worst = max(float((p.grad - grads_l[n]).norm() / grads_l[n].norm().clamp(min=1e-30))
                for n, p in model.named_parameters() if p.grad is not None)
    t_l, t_b = timed_pair(looped, batched)
    res = dict(items=len(items), points_per_item=2025, boundary_points_per_item=int(items[0][4].shape[0]),
               step_fwd_bwd_looped_ms=t_l, step_fwd_bwd_batched_ms=t_b, loss_looped=loss_l, loss_batched=loss_b,
               worst_gradient_rel_distance=worst,
               library_calls_looped=library_calls(looped), library_calls_batched=library_calls(batched),
               kernels_looped=kernel_dispatches(looped), kernels_batched=kernel_dispatches(batched))
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("# One recorded window step: looped over the samples against one batched step\n\n"
                "`python tools/bench_batched_step.py` on one MI355X: the WaterRamps network (random weights) on "
                f"{res['items']} scenes of {res['points_per_item']} particles over {res['boundary_points_per_item']} boundary "
                "points each; forward, weighted_mse loss and backward of one step; HIP events, medians of 15, the two variants "
                "alternating in one process.\n\n"
                "| | looped | batched |\n|---|---|---|\n"
                f"| forward + backward (ms) | {t_l} | {t_b} |\n"
                f"| library entry points called per step | {res['library_calls_looped']} | {res['library_calls_batched']} |\n"
                f"| device kernels dispatched per step | {res['kernels_looped']} | {res['kernels_batched']} |\n"
                f"| loss | {loss_l:.6g} | {loss_b:.6g} |\n\n"
                f"Worst distance of a parameter gradient between the two, relative to its norm: {worst:.2e}.\n")


if __name__ == "__main__":
    main()
