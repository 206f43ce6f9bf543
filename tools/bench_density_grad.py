"""Cost of the density gradient (dmcf_frs_window_sum_backward, dmcf_amd/csrc/frs.hip): DESIGN.md section 4.12.

  python tools/bench_density_grad.py [--side 100] [--reps 5] [--out bench_density_grad.json]

On bench.py's box (--side^3 fluid particles of spacing 0.05 plus the boundary shell, all positions in ONE set as the models
call compute_density), window poly6, R = the model's dens_radius[0] (Liquid3d: particle_radii[0]); ms from HIP events, median of
--reps after one warm-up, each on the search structure built once outside the timing:
  * window_sum_forward:   the fused scan dmcf_frs_window_sum;
  * window_sum_backward:  dmcf_frs_window_sum_backward, same set (coef_queries = coef_points = the incoming gradient);
  * torch_pair_list:      forward + backward of the torch composition on the explicit pair list (what the open3d readings take;
                          the search that makes the list is outside the timing), with its peak memory above the list itself."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dmcf_amd import ops  # noqa: E402
from tools import configs, scenes  # noqa: E402
from tools.bench_metrics import timed  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    radius = float(configs.LIQUID3D["particle_radii"][0])
    sc = scenes.box_scene(args.side)
    pos = torch.from_numpy(np.concatenate([sc["pos"], sc["box"]])).to(dev)
    n = pos.shape[0]
    G = torch.from_numpy(np.random.default_rng(1).normal(size=n).astype(np.float32)).to(dev)
    table = ops.build_spatial_hash_table(pos, radius, n_queries=n)
    r = dict(device=torch.cuda.get_device_name(0), n=n, radius=radius, window="poly6")
    r["window_sum_forward"] = timed(lambda: ops.window_sum(pos, pos, radius, "poly6", hash_table=table), args.reps)
    r["window_sum_backward"] = timed(lambda: ops.window_sum_backward(pos, table, radius, "poly6", G, G), args.reps)
    r["backward_over_forward"] = r["window_sum_backward"]["ms_median"] / r["window_sum_forward"]["ms_median"]

    nns = ops.fixed_radius_search(pos, pos, radius, return_distances=False, hash_table=table)
    idx, rs = nns.neighbors_index.long(), nns.neighbors_row_splits
    row = torch.repeat_interleave(torch.arange(n, device=dev), torch.diff(rs), output_size=idx.shape[0])
    r["pairs"] = int(idx.shape[0])

    def composition():
        p = pos.detach().requires_grad_(True)
        d2 = ((p[idx] - p[row]) ** 2).sum(-1)
        w = torch.clamp((1 - d2 / (radius * radius)) ** 3, 0, 1)
        out = torch.zeros(n, dtype=torch.float32, device=dev).index_add(0, row, w)
        return torch.autograd.grad(out, [p], G)[0]

    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    r["torch_pair_list"] = dict(timed(composition, args.reps),
                                peak_bytes_above_list=int(torch.cuda.max_memory_allocated(dev) - base))
    # the two must agree (a coarse check: the timing is of the right thing)
    a = ops.window_sum_backward(pos, table, radius, "poly6", G, G)
    b = composition()
    r["max_abs_difference"] = float((a - b).abs().max())
    r["max_abs_gradient"] = float(b.abs().max())
    print(json.dumps(r), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(r, f, indent=1)


if __name__ == "__main__":
    main()
