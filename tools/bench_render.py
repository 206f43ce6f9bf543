"""Times the disc rasterizer (ops.raster_discs: dmcf_raster_count, the host read of the bin size, dmcf_raster_discs) on the
renderer's flagship input: the 2-D 1000 x 1000 box of tools/scenes.box_scene(1000, dim=2) with its shell (~1M points), laid
out as utils/draw_sim2d.py lays it out, at heights 360, 1080 and 2160, with F = 1 and F = 5 frames per call.  Radius: half the
particle spacing.  Medians of HIP events over --reps calls after --warmup; counts of binned (disc, tile) entries and of
pixel-disc evaluations (256 per entry and frame); host PNG encoding of one frame (Pillow) timed separately.

    python tools/bench_render.py [--reps 20] [--warmup 3]      -> one JSON line per case
"""
import argparse
import io
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--heights", type=int, nargs="+", default=[360, 1080, 2160])
    ap.add_argument("--frames", type=int, nargs="+", default=[1, 5])
    args = ap.parse_args()
    import torch
    from PIL import Image

    from dmcf_amd import _lib, ops
    from dmcf_amd.utils.draw_sim2d import canvas_layout
    from tools.scenes import box_scene
    if not torch.cuda.is_available():
        raise SystemExit("bench_render needs a GPU")
    dev = torch.device("cuda:0")
    sc = box_scene(1000, dim=2)
    mirror = np.float32([1, -1])
    bnd = sc["box"][:, :2] * mirror
    pts = np.concatenate([sc["pos"][:, :2] * mirror, bnd])
    L = _lib.lib()
    for H in args.heights:
        W, H, scale, shift = canvas_layout(bnd, 0.1, H)
        r = float(0.025 * scale)
        base = (scale * (pts + shift)).astype(np.float32)
        for F in args.frames:
            # F distinct frames: the scene moved by a fraction of a pixel per frame
            xy = torch.from_numpy(np.stack([base + np.float32(0.37 * f) for f in range(F)])).to(dev)
            out = torch.ones((F, H, W, 3), dtype=torch.float32, device=dev)
            for _ in range(args.warmup):
                ops.raster_discs(xy, r, 0xff0071c5, W, H, out=out)
            times = []
            for _ in range(args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                ops.raster_discs(xy, r, 0xff0071c5, W, H, out=out)
                e1.record()
                torch.cuda.synchronize()
                times.append(e0.elapsed_time(e1))
            # the bin size of this input (the count the call reads back)
            n = xy.shape[1]
            nbytes = int(L.dmcf_raster_workspace_bytes(n, F, n, W, H))
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            total = torch.empty(1, dtype=torch.int64, device=dev)
            _lib.check(L.dmcf_raster_count(ops._ptr(xy), n, F, n, r, W, H, ops._ptr(ws), nbytes, ops._ptr(total), ops._stream()),
                       "dmcf_raster_count")
            entries = int(total.item())
            frame = ops.rgba8(out[0]).cpu().numpy()
            t0 = time.perf_counter()
            Image.fromarray(frame, "RGBA").save(io.BytesIO(), format="PNG")
            png_ms = 1e3 * (time.perf_counter() - t0)
            ms = float(np.median(times))
            print(json.dumps(dict(height=H, width=W, frames=F, discs=n, radius_px=round(r, 4), call_ms=round(ms, 4),
                                  ms_per_frame=round(ms / F, 4), call_ms_min=round(float(np.min(times)), 4), entries=entries,
                                  pixel_disc_evals=entries * 256, png_encode_ms_per_frame=round(png_ms, 2))), flush=True)


if __name__ == "__main__":
    main()
