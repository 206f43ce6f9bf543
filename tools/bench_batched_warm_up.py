"""Time the warm-up of one training batch, sample by sample (Simulator.warm_up, the reference's loop) against the batched
warm-up (Simulator.warm_up_batched, the pipeline key warm_up_batched):

  the WaterRamps network (tools/configs.py, random weights, window_dens poly6) on 16 scenes of 2,025 particles over 198
  boundary points -- the scenes of tools/bench_batched_step.py -- with pre = 20 for every sample and max_dens_err so high
  that no sample leaves early: both variants take 20 steps per sample and 20 density checks per sample

HIP events around each variant, a warm-up, the two variants alternating in one process; medians of 15, device-synchronised.
Both variants include what they cost the host.  Beside the times: the library entry points each variant calls per warm-up and
the host's reads of device tensors (counted at the Python level).  Prints one JSON line and writes the
table to ``--out`` (default profiles/batched_warm_up.md)."""
import argparse
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dmcf_amd import _lib, models  # noqa: E402
from dmcf_amd.pipelines.simulator import Simulator  # noqa: E402
from dmcf_amd.utils import tf_checkpoint as tc  # noqa: E402
from tools import configs, scenes  # noqa: E402
from tools.bench_batched_search import timed_pair  # noqa: E402
from tools.bench_batched_step import scene_items  # noqa: E402


class Counting:
    def __init__(self, real):
        self._real, self.calls = real, {}

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("dmcf_") or name in ("dmcf_error_string", "dmcf_last_hip_error") or name.endswith("_bytes"):
            return fn

        def counted(*a):
            self.calls[name] = self.calls.get(name, 0) + 1
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


def host_copies(fn):
    """Reads of a device tensor by the host during one call: ``item`` / ``tolist`` / ``float()`` / ``int()`` / ``bool()`` /
    ``cpu`` / ``numpy`` on a device tensor, counted at the Python level (each is one synchronising device -> host copy; the
    implicit one inside ``nonzero`` is not seen here)."""
    names = ("item", "tolist", "__float__", "__int__", "__bool__", "__index__", "cpu", "numpy")
    real = {n: getattr(torch.Tensor, n) for n in names}
    count, depth = [0], [0]

    def wrap(f):
        def counted(t, *a, **k):
            outer = depth[0] == 0 and t.is_cuda
            if outer:
                count[0] += 1
            depth[0] += 1  # (tolist and float() may call item underneath: one copy, counted once)
            try:
                return f(t, *a, **k)
            finally:
                depth[0] -= 1
        return counted

    for n, f in real.items():
        setattr(torch.Tensor, n, wrap(f))
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        for n, f in real.items():
            setattr(torch.Tensor, n, f)
    return count[0]


def batch_data(items, pre, dt):
    """The data loader's form of the batch: frames p0 + k dt v0, pre + 1 of them per sample."""
    data = dict(pos=[], vel=[], grav=[], box=[], box_normals=[], pre=[pre] * len(items))
    for it in items:
        p0, v0 = it[0].cpu().numpy(), it[1].cpu().numpy()
        data["pos"].append([(p0 + np.float32(k * dt) * v0).astype(np.float32) for k in range(pre + 1)])
        data["vel"].append([v0])
        data["grav"].append([None])
        data["box"].append([it[4].cpu().numpy()])
        data["box_normals"].append([it[5].cpu().numpy()])
    return data


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batched_warm_up.md"))
    ap.add_argument("--items", type=int, default=16)
    ap.add_argument("--pre", type=int, default=20)
    ap.add_argument("--reps", type=int, default=15)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = dict(configs.WATERRAMPS, window_dens="poly6")
    model = getattr(models, cfg["name"])(**cfg)
    tc.load_into_model(model, scenes.random_weights(cfg, seed=0), device=dev)
    items = scene_items(dev, args.items)
    data = batch_data(items, args.pre, model.timestep)
    sim = Simulator(model, device="cuda", main_log_dir=tempfile.mkdtemp())
    limit = 1e9  # (no sample leaves: identical work in both variants)

    looped = lambda: sim.warm_up(data, None, limit)  # noqa: E731
    batched = lambda: sim.warm_up_batched(data, None, limit)  # noqa: E731

    (lp, lv, lpre), (bp, bv, bpre) = looped(), batched()
    assert lpre == bpre == [args.pre - 1] * len(items), (lpre, bpre)
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max().clamp(min=1e-30))  # noqa: E731
    worst_pos = max(rel(a, b) for a, b in zip(bp, lp))
    worst_vel = max(rel(a, b) for a, b in zip(bv, lv))
    t_l, t_b = timed_pair(looped, batched, n=args.reps, warmup=2)
    calls_l, calls_b = library_calls(looped), library_calls(batched)
    keys = ("dmcf_frs_build", "dmcf_frs_window_sum", "dmcf_frs_build_batched", "dmcf_frs_window_sum_batched")
    res = dict(items=len(items), points_per_item=2025, boundary_points_per_item=int(items[0][4].shape[0]), pre=args.pre,
               warm_up_looped_ms=t_l, warm_up_batched_ms=t_b, worst_pos_rel=worst_pos, worst_vel_rel=worst_vel,
               library_calls_looped=sum(calls_l.values()), library_calls_batched=sum(calls_b.values()),
               entry_points_looped={k: calls_l.get(k, 0) for k in keys}, entry_points_batched={k: calls_b.get(k, 0) for k in keys},
               host_copies_looped=host_copies(looped), host_copies_batched=host_copies(batched))
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("# The warm-up of one training batch: looped over the samples against the batched warm-up\n\n"
                "`python tools/bench_batched_warm_up.py` on one MI355X: the WaterRamps network (random weights, window_dens "
                f"poly6) on {res['items']} scenes of {res['points_per_item']} particles over {res['boundary_points_per_item']} "
                f"boundary points each; pre = {args.pre} for every sample, max_dens_err so high that no sample leaves; HIP "
                f"events, device-synchronised medians of {args.reps}, the two variants alternating in one process.\n\n"
                "| | looped (`warm_up`) | batched (`warm_up_batched`) |\n|---|---|---|\n"
                f"| one warm-up (ms) | {t_l} | {t_b} |\n"
                f"| library entry points called | {res['library_calls_looped']} | {res['library_calls_batched']} |\n"
                + "".join(f"| `{k}` | {calls_l.get(k, 0)} | {calls_b.get(k, 0)} |\n" for k in keys)
                + f"| host reads of a device tensor (`item`, `tolist`, `float()`, `cpu`, ...) | {res['host_copies_looped']} | "
                  f"{res['host_copies_batched']} |\n\n"
                f"Worst distance of a sample's final state between the two after {args.pre} steps, relative to its largest "
                f"entry: positions {worst_pos:.2e}, velocities {worst_vel:.2e}.\n")


if __name__ == "__main__":
    main()
