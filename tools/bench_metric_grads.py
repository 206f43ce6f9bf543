"""Cost of the point-cloud op gradients (dmcf_amd/csrc/metrics_bwd.hip): DESIGN.md section 4.11.

  python tools/bench_metric_grads.py [--sizes 1280,10000,100000] [--reps 5] [--out bench_metric_grads.json]

For n = m in --sizes, 3-D and 2-D (z = 0) point sets uniform in a cube / square at the particle spacing of the shipped scenes
(as tools/bench_metrics.py), ms from HIP events, median of --reps after one warm-up, of each backward alone (its forward state
made once, outside the timing):
  * nn_distance_backward: both distance gradients given (two index inversions + two gathers);
  * emd: the forward (dmcf_emd) next to the recording forward (dmcf_emd_with_levels) and the match-free backward
    (dmcf_emd_backward, both gradients), with pairs_per_s = 2 n m / backward time;
  * match_cost_backward: dense match, only where [n, n] floats fit (n <= 10 000);
  * gather_point_backward: n rows gathered by n random indices (repeats) onto n rows, 3 channels;
  * the degenerate cases of the inversion: nn_distance_backward_collapsed (the second set moved 1000 away, so all its points
    share one nearest point and vice versa) and gather_point_backward_one_target (every index 0)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dmcf_amd import ops  # noqa: E402
from tools.bench_metrics import points, timed  # noqa: E402


def bench(n, dim, reps, dev):
    a, b = points(n, dim, 1, dev), points(n, dim, 2, dev)
    r = dict(n=n, m=n, dim=dim)
    d1, i1, d2, i2 = ops.nn_distance(a, b)
    g1, g2 = torch.ones_like(d1), torch.ones_like(d2)
    r["nn_distance_backward"] = timed(lambda: ops.nn_distance_backward(a, b, i1, i2, g1, g2), reps)
    far = b + 1000.0  # a distant cloud: every point of each set has the same nearest point in the other (one long segment)
    _, j1, _, j2 = ops.nn_distance(a, far)
    r["nn_distance_backward_collapsed"] = dict(timed(lambda: ops.nn_distance_backward(a, far, j1, j2, g1, g2), reps),
                                               largest_segment=int(torch.bincount(j2[0].long()).max()))
    big = n >= 50000
    gc = torch.ones(1, dtype=torch.float32, device=dev)
    _, levels = ops.emd_with_levels(a, b)
    r["emd_forward"] = timed(lambda: ops.emd(a, b), 3 if big else reps)
    r["emd_with_levels"] = timed(lambda: ops.emd_with_levels(a, b), 3 if big else reps)
    bw = timed(lambda: ops.emd_backward(a, b, levels, gc), 3 if big else reps)
    r["emd_backward"] = dict(bw, pairs_per_s=2 * n * n / (bw["ms_median"] * 1e-3))
    if n <= 10000:
        match = ops.approx_match(a, b)
        r["match_cost_backward"] = timed(lambda: ops.match_cost_backward(a, b, match, gc), reps)
        del match
    x = torch.from_numpy(np.random.default_rng(3).normal(size=(n, 3)).astype(np.float32)).to(dev)
    idx = torch.from_numpy(np.random.default_rng(4).integers(0, n, size=n).astype(np.int32)).to(dev)
    r["gather_point_backward"] = timed(lambda: ops.gather_point_backward(x, idx, n), reps)
    one = torch.zeros_like(idx)  # every row gathered from row 0
    r["gather_point_backward_one_target"] = timed(lambda: ops.gather_point_backward(x, one, n), reps)
    return r


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1280,10000,100000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    out = dict(device=torch.cuda.get_device_name(0), sizes=[])
    for n in [int(s) for s in args.sizes.split(",")]:
        for dim in (3, 2):
            r = bench(n, dim, args.reps, dev)
            out["sizes"].append(r)
            print(json.dumps(r), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
