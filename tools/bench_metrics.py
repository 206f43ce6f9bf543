"""Validation-metric cost (dmcf_amd/csrc/metrics.hip): DESIGN.md section 4.7.

  python tools/bench_metrics.py [--sizes 1280,10000,100000] [--reps 5] [--out bench_metrics.json]

Reports, for n = m in --sizes (1 280 = the canyon crop), 3-D and 2-D (z = 0) point sets uniform in a cube / square holding
the particles at the spacing of the shipped scenes:
  * nn_distance: both directions (ops.nn_distance), ms from HIP events, median of --reps after one warm-up;
  * emd: the fused approximate-match EMD (ops.emd, 10 levels x 3 all-pairs passes, no match formed);
  * pairs_per_s: n m / time (nn_distance: 2 n m);
and one whole Simulator.run_valid (rollout + every metric) on a generated Liquid3d box scene (--valid-side^3 particles,
--valid-frames frames), ms wall time, median of --reps."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dmcf_amd import models, ops  # noqa: E402
from dmcf_amd.datasets.dataset_reader_physics import Dataset  # noqa: E402
from dmcf_amd.pipelines import Simulator  # noqa: E402
from dmcf_amd.utils import tf_checkpoint as tc  # noqa: E402
from tools import configs, scenes  # noqa: E402


def timed(fn, n=5):
    fn()
    ts = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return dict(ms_median=float(np.median(ts)), ms_min=float(np.min(ts)), ms_max=float(np.max(ts)))


def points(n, dim, seed, dev):
    side = (n * 0.025 ** dim) ** (1.0 / dim)  # particle spacing 0.025 (Liquid3d)
    p = np.random.default_rng(seed).uniform(0, side, (1, n, 3)).astype(np.float32)
    if dim == 2:
        p[..., 2] = 0
    return torch.from_numpy(p).to(dev)


def bench_pairs(n, dim, reps, dev):
    a, b = points(n, dim, 1, dev), points(n, dim, 2, dev)
    nn = timed(lambda: ops.nn_distance(a, b), reps)
    emd = timed(lambda: ops.emd(a, b), max(1, reps if n < 50000 else 3))
    return dict(n=n, m=n, dim=dim, nn_distance=dict(nn, pairs_per_s=2 * n * n / (nn["ms_median"] * 1e-3)),
                emd=dict(emd, pairs_per_s_per_pass=30 * n * n / (emd["ms_median"] * 1e-3)))


def bench_run_valid(side, frames, reps, dev, tmp):
    cfg = dict(configs.LIQUID3D)
    sc = scenes.box_scene(side)
    rng = np.random.default_rng(0)
    fr = []
    for t in range(frames):  # a drifting, jittered copy of the box as the "target" frames
        pos = sc["pos"] + (0.02 * t) * sc["vel"] + rng.normal(0, 1e-3, sc["pos"].shape).astype(np.float32)
        fr.append(dict(pos=pos.astype(np.float32), vel=sc["vel"], frame_id=t, scene_id="box", box=sc["box"],
                       box_normals=sc["box_normals"], grav=np.float32([0, -9.81, 0])))
    model = getattr(models, cfg["name"])(**cfg)
    tc.load_into_model(model, scenes.random_weights(cfg, seed=0), device=dev)
    sim = Simulator(model, dataset=None, main_log_dir=tmp, split="valid", device="cuda",
                    data_generator=dict(valid=dict(stride=1, time_end=frames)))
    sim.dataset = type("D", (), {"valid": Dataset(data=[fr]), "name": "box"})()
    ts = []
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = sim.run_valid(epoch=0)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts = ts[1:]
    return dict(particles=int(sc["pos"].shape[0]), boundary=int(sc["box"].shape[0]), frames=frames,
                ms_median=float(np.median(ts)), ms_min=float(np.min(ts)), metrics=res)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1280,10000,100000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--valid-side", type=int, default=20)
    ap.add_argument("--valid-frames", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    out = dict(device=torch.cuda.get_device_name(0), pairs=[])
    for n in [int(s) for s in args.sizes.split(",")]:
        for dim in (3, 2):
            r = bench_pairs(n, dim, args.reps, dev)
            out["pairs"].append(r)
            print(json.dumps(r), flush=True)
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        out["run_valid"] = bench_run_valid(args.valid_side, args.valid_frames, args.reps, dev, tmp)
    print(json.dumps(out["run_valid"]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    return out


if __name__ == "__main__":
    main()
