"""Time the validation of a split of many small scenes, scene after scene (Simulator.run_valid, the reference's loops) against
the batched validation (the pipeline key valid_batched: run_rollout_batched + valid_losses_batched):

  the WaterRamps network (tools/configs.py, random weights, window_dens poly6) on 16 scenes of 2,025 particles over 198
  boundary points -- the scenes of tools/bench_batched_step.py -- with 4 frames each, so 3 evaluated frames per scene;
  once with split "train" (what run_train's validation after every epoch computes: mse_val, chamfer_val, mse_single_val) and
  once with split "valid" (all nine metrics; the batched variant computes emd for all scenes in one dmcf_emd_ragged call per
  frame and the two vel_diff_val in one dmcf_hist_pair_ragged call per frame, where the loop calls the host compare_dist
  twice per scene);
  and, at the operator level, ops.emd called scene after scene on the split's first and last target frames against one
  ops.emd_ragged call for all scenes (no host copy in either; the costs are checked to be bit-identical)

A host clock around each run_valid, which ends device-synchronised; a warm-up, then the two variants alternating in one
process; the median and the range of ``--reps`` runs, divided by the evaluated frames: the wall time per evaluated frame, its
rollout step and its metrics.  Beside the times: the library entry points each variant calls per evaluated frame.  Prints one
JSON line and writes the tables to ``--out`` (default profiles/batched_valid.md).  ``--baseline FILE``: the JSON line of a run
of this tool on another commit in the same session; its batched times are quoted in a table of their own."""
import argparse
import json
import os
import sys
import tempfile
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dmcf_amd import datasets, models, ops  # noqa: E402
from dmcf_amd.pipelines.simulator import Simulator  # noqa: E402
from dmcf_amd.utils import tf_checkpoint as tc  # noqa: E402
from tools import configs, scenes  # noqa: E402
from tools.bench_batched_step import scene_items  # noqa: E402
from tools.bench_batched_warm_up import library_calls  # noqa: E402


def split_data(items, frames, dt):
    """get_rollout's form of the split: [T, N, 3] arrays per scene; the targets are p0 + k dt v0."""
    data = []
    for it in items:
        p0, v0, box, nrm = (it[k].cpu().numpy() for k in (0, 1, 4, 5))
        rep = lambda x: np.broadcast_to(x, (frames,) + x.shape).copy()  # noqa: E731
        data.append(dict(pos=np.stack([(p0 + np.float32(k * dt) * v0).astype(np.float32) for k in range(frames)]), vel=rep(v0),
                         grav=None, box=rep(box), box_normals=rep(nrm)))
    return data


def timed_pair(a, b, n, warmup):
    """Wall times (ms) of a() and b(), measured alternately, each ending device-synchronised -> two lists."""
    for _ in range(warmup):
        a()
        b()
    ts = ([], [])
    for _ in range(n):
        for k, fn in enumerate((a, b)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts[k].append((time.perf_counter() - t0) * 1e3)
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batched_valid.md"))
    ap.add_argument("--items", type=int, default=16)
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--baseline", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = dict(configs.WATERRAMPS, window_dens="poly6")
    model = getattr(models, cfg["name"])(**cfg)
    tc.load_into_model(model, scenes.random_weights(cfg, seed=0), device=dev)
    items = scene_items(dev, args.items)
    data = split_data(items, args.frames, model.timestep)
    datasets.get_rollout = lambda *a, **k: data  # (run_valid reads its split through dmcf_amd.datasets.get_rollout)
    evaluated = args.frames - 1
    res = dict(items=len(items), points_per_item=2025, boundary_points_per_item=int(items[0][4].shape[0]), frames=args.frames,
               evaluated_frames=evaluated, reps=args.reps, splits={})
    rows = []
    stat = lambda t: dict(median=round(float(np.median(t)), 3), min=round(float(t.min()), 3), max=round(float(t.max()), 3))  # noqa: E731
    fmt = lambda s: f"{s['median']} ({s['min']} - {s['max']})"  # noqa: E731
    for split in ("train", "valid"):
        sims = [Simulator(model, dataset=types.SimpleNamespace(valid=None), device="cuda", main_log_dir=tempfile.mkdtemp(),
                          split=split, valid_batched=batched) for batched in (False, True)]
        looped, batched = (lambda s=s: s.run_valid(epoch=0) for s in sims)
        want, got = looped(), batched()
        assert list(want) == list(got)
        worst = max(abs(got[k] - want[k]) / max(abs(want[k]), 1e-30) for k in want)
        t_l, t_b = (np.asarray(t) / evaluated for t in timed_pair(looped, batched, args.reps, warmup=2))
        calls_l, calls_b = library_calls(looped), library_calls(batched)
        r = dict(looped_ms_per_frame=stat(t_l), batched_ms_per_frame=stat(t_b),
                 library_calls_per_frame_looped=round(sum(calls_l.values()) / evaluated, 1),
                 library_calls_per_frame_batched=round(sum(calls_b.values()) / evaluated, 1),
                 nn_distance_calls_per_frame_looped=calls_l.get("dmcf_nn_distance", 0) / evaluated,
                 nn_distance_ragged_calls_per_frame_batched=calls_b.get("dmcf_nn_distance_ragged", 0) / evaluated,
                 emd_calls_per_frame_looped=calls_l.get("dmcf_emd", 0) / evaluated,
                 emd_calls_per_frame_batched=calls_b.get("dmcf_emd", 0) / evaluated,
                 emd_ragged_calls_per_frame_batched=calls_b.get("dmcf_emd_ragged", 0) / evaluated,
                 hist_pair_ragged_calls_per_frame_batched=calls_b.get("dmcf_hist_pair_ragged", 0) / evaluated,
                 worst_metric_rel_diff=worst, metrics=list(want))
        res["splits"][split] = r
        rows.append(f"| {split} | {fmt(r['looped_ms_per_frame'])} | {fmt(r['batched_ms_per_frame'])} | "
                    f"{r['library_calls_per_frame_looped']} | {r['library_calls_per_frame_batched']} | "
                    f"{r['nn_distance_calls_per_frame_looped']:g} | {r['nn_distance_ragged_calls_per_frame_batched']:g} | "
                    f"{r['emd_calls_per_frame_looped']:g} | {r['emd_calls_per_frame_batched']:g} | "
                    f"{r['emd_ragged_calls_per_frame_batched']:g} | {worst:.1e} |\n")
    # the operator alone: every scene's last target frame against its first, scene after scene and in one ragged call
    x1 = [torch.from_numpy(d["pos"][-1]).to(dev) for d in data]
    x2 = [torch.from_numpy(d["pos"][0]).to(dev) for d in data]
    X1, X2 = torch.cat(x1), torch.cat(x2)
    rs1, rs2 = (np.concatenate([[0], np.cumsum([x.shape[0] for x in xs])]).tolist() for xs in (x1, x2))
    emd_looped = lambda: [ops.emd(a.unsqueeze(0), b.unsqueeze(0)) for a, b in zip(x1, x2)]  # noqa: E731
    emd_ragged = lambda: ops.emd_ragged(X1, X2, rs1, rs2)  # noqa: E731
    assert torch.equal(torch.cat(emd_looped()), emd_ragged())
    t_l, t_b = (np.asarray(t) for t in timed_pair(emd_looped, emd_ragged, args.reps, warmup=2))
    res["emd_operator"] = dict(looped_ms=stat(t_l), ragged_ms=stat(t_b), library_calls_looped=sum(library_calls(emd_looped).values()),
                               library_calls_ragged=sum(library_calls(emd_ragged).values()), bit_identical=True)
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("# Validating a split of small scenes: looped over the scenes against `valid_batched`\n\n"
                "`python tools/bench_batched_valid.py` on one MI355X: the WaterRamps network (random weights, window_dens poly6) "
                f"on {res['items']} scenes of {res['points_per_item']} particles over {res['boundary_points_per_item']} boundary "
                f"points each, {args.frames} frames per scene ({evaluated} evaluated).  Wall time of `run_valid` per evaluated "
                f"frame (all scenes: the rollout step and the metrics), device-synchronised; median (min - max) of {args.reps} "
                "runs, the two variants alternating in one process after a warm-up.  Split \"train\" is the validation "
                "`run_train` runs after every epoch (mse_val, chamfer_val, mse_single_val); split \"valid\" computes all nine "
                "metrics; the batched variant computes emd in one `dmcf_emd_ragged` call per frame and the two vel_diff_val in "
                f"one `dmcf_hist_pair_ragged` call per frame ({res['splits']['valid']['hist_pair_ragged_calls_per_frame_batched']:g} "
                "counted), where the loop calls the host `compare_dist` twice per scene.\n\n"
                "| split | looped, ms per frame | batched, ms per frame | library calls per frame, looped | batched | "
                "`dmcf_nn_distance` per frame, looped | `dmcf_nn_distance_ragged` per frame, batched | `dmcf_emd` per frame, "
                "looped | batched | `dmcf_emd_ragged` per frame, batched | worst relative difference of a metric |\n"
                "|---|---|---|---|---|---|---|---|---|---|---|\n" + "".join(rows))
        e = res["emd_operator"]
        f.write(f"\nThe operator alone, on the {res['items']} scenes' last target frame against their first "
                f"({res['points_per_item']} points each side): `ops.emd` called scene after scene against one `ops.emd_ragged` "
                "call, no host copy in either, the costs bit-identical; wall time of all scenes, device-synchronised, measured "
                "the same way.\n\n| | looped `ops.emd`, ms | one `ops.emd_ragged`, ms | library calls, looped | ragged |\n"
                f"|---|---|---|---|---|\n| emd, {res['items']} x {res['points_per_item']} | {fmt(e['looped_ms'])} | "
                f"{fmt(e['ragged_ms'])} | {e['library_calls_looped']} | {e['library_calls_ragged']} |\n")
        if args.baseline:
            with open(args.baseline) as g:
                base = json.loads(g.read().strip().splitlines()[-1])
            f.write("\nThe same command on the parent commit in the same session (its batched validation calls the host "
                    "`compare_dist` twice per scene and frame, each call with its device-to-host copy), against this commit:\n\n"
                    "| split | parent, batched ms per frame | this commit, batched ms per frame |\n|---|---|---|\n")
            for split in ("train", "valid"):
                f.write(f"| {split} | {fmt(base['splits'][split]['batched_ms_per_frame'])} | "
                        f"{fmt(res['splits'][split]['batched_ms_per_frame'])} |\n")


if __name__ == "__main__":
    main()
