"""Per-point extents on the 1M-particle bench box (config 5, side 100): the radius search with radii spread over [0.5, 1] x R
and the individual-extent CConv on its list, next to the scalar search and CConv at R on the same scene.

  python tools/bench_extents.py [--side 100] [--radius 0.1] [--out bench_extents.json]

Every time is the median of 5 runs between device events, after one warm-up run; the searches include the grid build and
their host round trips (the pair count; the radius search also reads max_radius), as a layer pays them.  The CConv is one
8 -> 16 channel layer with a 4x4x4 filter and the poly6 window formed in the kernel (the flagship's flags)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dmcf_amd import ops  # noqa: E402
from tools import scenes  # noqa: E402


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
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=100)
    ap.add_argument("--radius", type=float, default=0.1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_extents needs a GPU")
    dev = torch.device("cuda:0")
    sc = scenes.box_scene(args.side)
    pos = torch.from_numpy(np.concatenate([sc["pos"], sc["box"]])).to(dev)
    n = pos.shape[0]
    R = float(np.float32(args.radius))
    rng = np.random.default_rng(0)
    radii = torch.from_numpy(rng.uniform(0.5 * R, R, size=n).astype(np.float32)).to(dev)
    feat = torch.from_numpy(rng.normal(size=(n, 8)).astype(np.float32)).to(dev)
    filt = torch.from_numpy(rng.uniform(-0.1, 0.1, size=(4, 4, 4, 8, 16)).astype(np.float32)).to(dev)
    kw = dict(window="poly6", align_corners=True, coordinate_mapping="ball_to_cube_volume_preserving", interpolation="linear")

    scalar = ops.fixed_radius_search(pos, pos, R, return_distances=False)
    per_point = ops.radius_search(pos, pos, radii, return_distances=False)
    rows = {}

    def report(name, t, pairs, **extra):
        rows[name] = dict(ms_median=t[0], ms_min=t[1], ms_max=t[2], pairs=int(pairs), **extra)
        print(json.dumps({name: rows[name]}), flush=True)

    report("search_scalar", timed(lambda: ops.fixed_radius_search(pos, pos, R, return_distances=False)),
           scalar.neighbors_row_splits[-1].item())
    report("search_radii", timed(lambda: ops.radius_search(pos, pos, radii, return_distances=False)),
           per_point.neighbors_row_splits[-1].item())
    si, srs, _ = scalar.raw()
    pi, prs, _ = per_point.raw()
    ext = 2.0 * radii
    const = torch.full_like(radii, 2.0 * R)
    out = torch.empty((n, 16), dtype=torch.float32, device=dev)
    report("cconv_scalar", timed(lambda: ops.cconv_forward(filt, pos, 2.0 * R, pos, feat, si, srs, out=out, **kw)),
           scalar.neighbors_row_splits[-1].item(),
           kernel=ops.cconv_forward(filt, pos, 2.0 * R, pos, feat, si, srs, name_only=True, **kw))
    report("cconv_extents_scalar_list", timed(lambda: ops.cconv_forward(filt, pos, const, pos, feat, si, srs, out=out, **kw)),
           scalar.neighbors_row_splits[-1].item(),
           kernel=ops.cconv_forward(filt, pos, const, pos, feat, si, srs, name_only=True, **kw))
    report("cconv_extents", timed(lambda: ops.cconv_forward(filt, pos, ext, pos, feat, pi, prs, out=out, **kw)),
           per_point.neighbors_row_splits[-1].item(),
           kernel=ops.cconv_forward(filt, pos, ext, pos, feat, pi, prs, name_only=True, **kw))
    result = dict(points=n, radius=R, radii="uniform [0.5, 1] x radius", layer="4x4x4, 8 -> 16, poly6", rows=rows)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
