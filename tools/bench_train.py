"""Milliseconds per training iteration (Simulator.train_step), split into data, warm-up, recorded forward, backward, optimizer
and checkpoint, for two cases:

  liquid3d    Liquid3d SymNet (tests/golden weights) on the canyon frames: batch 8, window 3
  waterramps  WaterRamps SymNet (random weights) on a synthetic 2-D box of ~2k particles: batch 16, window 3

    python tools/bench_train.py [--case liquid3d|waterramps|both] [--iters 5] [--warmup 2]

Prints one JSON line per case.  The checkpoint column is one CheckpointManager.save per iteration (the loop saves once per
epoch).  Each phase is timed between device synchronisations (Simulator.train_step)."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LR = dict(lr_boundaries=[20000, 25000, 30000, 35000, 40000, 45000],
          lr_values=[0.001, 0.0005, 0.00025, 0.000125, 0.0000625, 0.00003125, 0.000015625])


def _case(name):
    from tools import configs, scenes
    if name == "liquid3d":
        fx = dict(np.load(os.path.join(ROOT, "tests", "golden", "canyon_frames.npz")))
        frames = [dict(pos=fx["pos"][t], vel=fx["vel"][t], frame_id=t, scene_id="canyon", box=fx["box"],
                       box_normals=fx["box_normals"]) for t in range(fx["pos"].shape[0])]
        model = dict(configs.LIQUID3D, loss={"weighted_mse": dict(typ="weighted_mse", fac=128.0, gamma=0.5, neighbor_scale=0.025)})
        weights = dict(np.load(os.path.join(ROOT, "tests", "golden", "liquid3d_weights.npz")))
        return frames, model, weights, 8, dict(scale=[1.0, 1.0, 1.0])
    s = scenes.box_scene(45, h=0.01, dim=2)  # 2025 particles
    frames, pos, vel = [], s["pos"].copy(), s["vel"].copy()
    for t in range(8):
        frames.append(dict(pos=pos.copy(), vel=vel.copy(), frame_id=t, scene_id="box", box=s["box"], box_normals=s["box_normals"]))
        vel = vel + np.float32(0.0025) * np.array([0, -9.81, 0], np.float32)
        pos = pos + np.float32(0.0025) * vel
    model = dict(configs.WATERRAMPS, loss={"weighted_mse": dict(typ="weighted_mse", fac=1000.0, gamma=0.5, neighbor_scale=0.0625)})
    return frames, model, scenes.random_weights(configs.WATERRAMPS, seed=0), 16, dict(scale=[1.0, 1.0, 0.0])


def run(name, iters, warmup, window=3):
    import torch
    from dmcf_amd import models
    from dmcf_amd.datasets import Dataset, get_dataloader
    from dmcf_amd.pipelines import Simulator
    from dmcf_amd.pipelines.simulator import TrainSchedule
    from dmcf_amd.utils import tf_checkpoint as tc
    from dmcf_amd.utils.config import Config
    frames, mcfg, weights, batch, gen = _case(name)
    model = getattr(models, mcfg["name"])(**mcfg)
    tc.load_into_model(model, weights, device="cuda")
    with tempfile.TemporaryDirectory() as tmp:
        sim = Simulator(model, None, main_log_dir=tmp, device="cuda", optimizer=LR, max_dens_err=0.1)
        np.random.seed(42)
        loader = get_dataloader(Dataset(data=[frames]), batch_size=batch, window=window, repeat=True, shuffle_buffer=64, **gen)
        sched = TrainSchedule(Config(dict(windows=[window], window_bnds=[], time_blend=1, max_warm_up=[0], warm_up_bnds=[],
                                          iterations=[0], its_bnds=[])))
        mgr = tc.CheckpointManager(os.path.join(tmp, "checkpoint"))
        rows = []
        for i in range(warmup + iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            data = next(loader)
            time_w = sched.time_weights([d.shape[0] for d in data["pos"]], data["pre"], i)
            t_data = time.perf_counter() - t0
            sim.train_step(data, time_w, 0, None, 0.1)
            t1 = time.perf_counter()
            mgr.save(model, sim.optimizer, i + 1)
            t_ckpt = time.perf_counter() - t1
            if i >= warmup:
                rows.append(dict(sim.train_timing, data=t_data, checkpoint=t_ckpt))
        ms = {k: round(1e3 * float(np.median([r[k] for r in rows])), 3) for k in rows[0]}
        n_params = sum(int(p.numel()) for p in sim.optimizer.params)
        n_points = int(frames[0]["pos"].shape[0])
        return dict(case=name, batch=batch, window=window, particles=n_points, parameters=n_params, iters=iters,
                    ms_per_iteration=round(sum(v for k, v in ms.items() if k != "checkpoint"), 3), ms=ms)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--case", default="both", choices=["liquid3d", "waterramps", "both"])
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args(argv)
    for name in (["liquid3d", "waterramps"] if args.case == "both" else [args.case]):
        print(json.dumps(run(name, args.iters, args.warmup)), flush=True)


if __name__ == "__main__":
    main()
