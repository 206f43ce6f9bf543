"""Times the sphere splat of the 3-D renderer (ops.splat_depth, ops.splat_shade: dmcf_amd/csrc/splat.hip) on the flagship scene:
the 1M-particle box of tools/scenes.box_scene(100) with its shell, at 1920 x 1080 through draw_sim3d's default camera with the
boundary as a FARTHEST layer (--bnd far).  Radius: half the particle spacing.  Per sample one frame is rendered as draw_sim3d
renders it -- two key fills, the fluid's depth call, the boundary's depth call, the image fill, the shade call -- and every
step is bracketed by HIP events (each depth / shade call is one kernel, so its events time that kernel and its launch).
Reported: median (min - max) of --samples samples per step, the launches per frame, the histogram of the spheres' clipped
bounding boxes (the depth kernel walks boxes of up to 256 pixels on one lane and hands larger ones to the wavefront), and, as a
yardstick only, ops.raster_discs on the same points' projected centres at the median pixel radius.

    python tools/bench_splat.py [--samples 7] [--warmup 2] [--side 100] [--width 1920] [--height 1080]     -> one JSON line
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _stats(v):
    return dict(median=round(float(np.median(v)), 4), min=round(float(np.min(v)), 4), max=round(float(np.max(v)), 4))


def footprints(cam, pts, radius, width, height, min_px=0.75):
    """(clipped bounding-box areas in pixels [n] -- 0 for spheres that are skipped or off the image --, pixel radii [n],
    projected centres [n, 2]) by the depth kernel's arithmetic, in float64."""
    v = np.float64(cam.view).reshape(3, 4)
    c = pts.astype(np.float64) @ v[:, :3].T + v[:, 3]
    live = c[:, 2] > cam.near
    z = np.where(live, c[:, 2], 1.0)
    m = np.full_like(z, cam.focal) if cam.orthographic else cam.focal / z
    sx, sy = cam.cx + m * c[:, 0], cam.cy + m * c[:, 1]
    R = np.maximum(m * radius, min_px)
    x0, x1 = np.maximum(np.floor(sx - R - 0.5), 0), np.minimum(np.ceil(sx + R - 0.5), width - 1)
    y0, y1 = np.maximum(np.floor(sy - R - 0.5), 0), np.minimum(np.ceil(sy + R - 0.5), height - 1)
    area = np.where(live & (x0 <= x1) & (y0 <= y1), (x1 - x0 + 1) * (y1 - y0 + 1), 0)
    return area.astype(np.int64), R, np.stack([sx, sy], axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--side", type=int, default=100, help="fluid particles per edge of the box (100: the 1M-particle scene)")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    args = ap.parse_args()
    import torch

    from dmcf_amd import ops
    from dmcf_amd.utils.draw_sim3d import default_pose
    from tools.scenes import box_scene
    if not torch.cuda.is_available():
        raise SystemExit("bench_splat needs a GPU")
    dev = torch.device("cuda:0")
    sc = box_scene(args.side)
    W, H, r = args.width, args.height, 0.025
    eye, target = default_pose(sc["box"], sc["pos"])
    cam = ops.look_at(eye, target, (0, 1, 0), W, H)
    fluid, bnd = torch.from_numpy(sc["pos"]).to(dev), torch.from_numpy(sc["box"]).to(dev)

    steps = ["fill_keys", "depth_fluid", "depth_boundary", "fill_image", "shade"]
    times = {s: [] for s in steps + ["frame"]}
    for it in range(args.warmup + args.samples):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(steps) + 1)]
        ev[0].record()
        kf = torch.full((1, H, W), -1, dtype=torch.int64, device=dev)
        kb = torch.full((1, H, W), -1, dtype=torch.int64, device=dev)
        ev[1].record()
        ops.splat_depth(fluid, r, cam, W, H, out=kf)
        ev[2].record()
        ops.splat_depth(bnd, r, cam, W, H, farthest=True, out=kb)
        ev[3].record()
        img = torch.ones((1, H, W, 3), dtype=torch.float32, device=dev)
        ev[4].record()
        ops.splat_shade([ops.SplatLayer(kf, fluid, r, 0xff0071c5), ops.SplatLayer(kb, bnd, r, 0xff9e9e9e, True)], cam, W, H, out=img)
        ev[5].record()
        torch.cuda.synchronize()
        if it >= args.warmup:
            for j, s in enumerate(steps):
                times[s].append(ev[j].elapsed_time(ev[j + 1]))
            times["frame"].append(ev[0].elapsed_time(ev[5]))
    q = ops.rgba8(img)
    fluid_px = int(((q[0, ..., 2].int() - q[0, ..., 0].int()) > 40).sum().item())
    covered = int((kf[0] != -1).sum().item()), int((kb[0] != -1).sum().item())

    edges = [0, 1, 5, 17, 65, 257, 1025, 16385, 1 << 62]
    names = ["off_image", "1-4", "5-16", "17-64", "65-256", "257-1024", "1025-16384", ">16384"]
    hist = {}
    for label, pts in (("fluid", sc["pos"]), ("boundary", sc["box"])):
        area, R, centres = footprints(cam, pts, r, W, H)
        counts = np.histogram(area, bins=edges)[0]
        hist[label] = dict(zip(names, (int(c) for c in counts)), radius_px_median=round(float(np.median(R)), 3),
                           radius_px_max=round(float(R.max()), 3), box_pixels_total=int(area.sum()),
                           wave_path_spheres=int((area > 256).sum()))
        if label == "fluid":
            xy_f, r_px = centres, float(np.median(R))
        else:
            xy_b = centres

    # the yardstick: the 2-D disc rasterizer on the projected centres (no depth test, two calls with a host read each)
    xf, xb = (torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev) for a in (xy_f, xy_b))
    disc = []
    for it in range(args.warmup + args.samples):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        img2 = torch.ones((1, H, W, 3), dtype=torch.float32, device=dev)
        ops.raster_discs(xf, r_px, 0xff0071c5, W, H, out=img2)
        ops.raster_discs(xb, r_px, 0xff9e9e9e, W, H, out=img2)
        e1.record()
        torch.cuda.synchronize()
        if it >= args.warmup:
            disc.append(e0.elapsed_time(e1))

    print(json.dumps(dict(scene=f"box_scene({args.side})", fluid=int(fluid.shape[0]), boundary=int(bnd.shape[0]), width=W, height=H,
                          radius=r, samples=args.samples, ms={s: _stats(times[s]) for s in times},
                          launches_per_frame=dict(kernels=3, fills=3), pixels_with_fluid_key=covered[0],
                          pixels_with_boundary_key=covered[1], pixels_showing_fluid=fluid_px, footprints=hist,
                          raster_discs_yardstick_ms=_stats(disc), raster_discs_radius_px=round(r_px, 3))), flush=True)


if __name__ == "__main__":
    main()
