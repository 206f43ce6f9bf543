"""Time both directions of the velocity-histogram KL of run_valid (vel_diff_val, vel_diff_val_2) for a batch of scenes:

  looped   evaluation_helper.compare_dist(x_b, y_b) and compare_dist(y_b, x_b) scene after scene on device tensors -- 2 x
           ``--items`` host calls, each with its device-to-host copies, two np.percentile partitions and two bincounts;
  ragged   evaluation_helper.compare_dist_pair(X, Y, row_splits): ONE dmcf_hist_pair_ragged call (9 launches, one memset and
           one table copy whatever the batch), one host copy of the integer counts, then _kl_from_counts per scene and direction

on ``--items`` scenes of ``--points`` velocities (default 16 x 2,025: the split of tools/bench_batched_valid.py) and on one
item of ``--large`` rows (default 1,000,000).  The values are checked to be bit-identical first.  A host clock around ``inner``
calls that end device-synchronised (both variants end on the host); a warm-up, then the two variants alternating in one
process; the median and the range of ``--reps`` samples, per call.  Prints one JSON line and writes the table to ``--out``
(default profiles/hist_pair.md)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dmcf_amd.utils.evaluation_helper import compare_dist, compare_dist_pair  # noqa: E402
from tools.bench_batched_warm_up import library_calls  # noqa: E402

LAUNCHES_PER_CALL = 9  # dmcf_hist_pair_ragged: four digit passes, four picks, one count (csrc/hist.hip), whatever the batch


def timed_pair(a, b, n, warmup, inner):
    """Wall times (ms per call) of a() and b(), ``inner`` calls per sample, measured alternately -> two lists."""
    for _ in range(warmup):
        a()
        b()
    ts = ([], [])
    for _ in range(n):
        for k, fn in enumerate((a, b)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(inner):
                fn()
            torch.cuda.synchronize()
            ts[k].append((time.perf_counter() - t0) * 1e3 / inner)
    return ts


def case(items, points, reps, inner, dev, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    xs = [torch.randn(points, 3, generator=g).to(dev) for _ in range(items)]
    ys = [(x.cpu() + 0.3 * torch.randn(points, 3, generator=g)).to(dev) for x in xs]
    X, Y = torch.cat(xs), torch.cat(ys)
    rs = [k * points for k in range(items + 1)]
    looped = lambda: [(compare_dist(x, y), compare_dist(y, x)) for x, y in zip(xs, ys)]  # noqa: E731
    ragged = lambda: compare_dist_pair(X, Y, row_splits=rs)  # noqa: E731
    want, (kl_xy, kl_yx) = looped(), ragged()
    assert [w[0] for w in want] == list(kl_xy) and [w[1] for w in want] == list(kl_yx), "the two variants differ"
    t_l, t_r = (np.asarray(t) for t in timed_pair(looped, ragged, reps, warmup=2, inner=inner))
    stat = lambda t: dict(median=round(float(np.median(t)), 3), min=round(float(t.min()), 3), max=round(float(t.max()), 3))  # noqa: E731
    return dict(items=items, points_per_item=points, inner=inner, looped_ms=stat(t_l), ragged_ms=stat(t_r), bit_identical=True,
                host_compare_dist_calls_looped=2 * items, library_calls_ragged=library_calls(ragged),
                launches_ragged=LAUNCHES_PER_CALL)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hist_pair.md"))
    ap.add_argument("--items", type=int, default=16)
    ap.add_argument("--points", type=int, default=2025)
    ap.add_argument("--large", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = dict(reps=args.reps, cases=[case(args.items, args.points, args.reps, 20, dev, 0), case(1, args.large, args.reps, 3, dev, 1)])
    print(json.dumps(res), flush=True)
    fmt = lambda s: f"{s['median']} ({s['min']} - {s['max']})"  # noqa: E731
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("# Both directions of the velocity-histogram KL: host `compare_dist` per scene against one `dmcf_hist_pair_ragged` call\n\n"
                "`python tools/bench_hist_pair.py` on one MI355X.  Looped: `compare_dist(x, y)` and `compare_dist(y, x)` scene after "
                "scene on device tensors (their device-to-host copies included).  Ragged: `compare_dist_pair` -- one "
                "`dmcf_hist_pair_ragged` call, one host copy of the counts, `_kl_from_counts` per scene and direction.  The values "
                f"are bit-identical.  Wall time per call of the whole batch, device-synchronised; median (min - max) of {args.reps} "
                "samples, the two variants alternating in one process after a warm-up.\n\n"
                "| batch | looped host `compare_dist`, ms | one ragged call, ms | host `compare_dist` calls, looped | "
                "kernel launches, ragged |\n|---|---|---|---|---|\n")
        for c in res["cases"]:
            f.write(f"| {c['items']} x {c['points_per_item']:,} | {fmt(c['looped_ms'])} | {fmt(c['ragged_ms'])} | "
                    f"{c['host_compare_dist_calls_looped']} | {c['launches_ragged']} |\n")


if __name__ == "__main__":
    main()
