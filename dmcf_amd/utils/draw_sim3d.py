"""Renders a 3-D simulation result file: what ``draw_sim2d`` does for 2-D results, with every particle drawn as a shaded,
depth-tested sphere on the GPU (``ops.splat_depth`` / ``ops.splat_shade``, dmcf_amd/csrc/splat.hip).  The reference has no 3-D
renderer; the file handling, the frame selection, the labels and the layout of the output are ``draw_sim2d``'s.

    python -m dmcf_amd.utils.draw_sim3d <result.hdf5 | .npz> <out.png> [--out_pattern 'dir/{pointset}_{frame:04d}.png']
        [--height 360 | --width W] [--aspect 1.7778] [--pr 0.005] [--br R] [--pointsets gt,GT pred,Ours] [--font_size 36]
        [--num_frames 5 | --frames i j ...] [--pc 0xff0071c5] [--bc 0xff9e9e9e] [--eye x y z] [--target x y z] [--up 0 1 0]
        [--fov 35 | --ortho H] [--bnd far|near|none] [--ambient 0.3]

The group ``SymNet`` (or the file's only group); ``bnd`` [M, 3] is the boundary, the point sets are sequences [T, N, 3].  Radii
are in simulation units.  Without ``--eye`` / ``--target`` the camera looks at the centre of the boundary's bounding box (of the
first drawn frame's fluid when ``bnd`` is empty) from ``target + 1.6 diagonal normalize(0.8, 0.5, 1.0)``; ``--up`` defaults to
+y (gravity is -y in the shipped 3-D configs).

``--bnd far`` (the default) keeps, per pixel, the FARTHEST boundary sphere: result files hold boundary positions without
normals, and a domain box is closed, so this shows the far walls and the floor as seen from inside, with the fluid (nearest
sphere per pixel) depth-tested in front of them -- a camera outside a closed box sees the fluid inside it.  ``--bnd near`` keeps
the nearest boundary sphere (open scenes: a terrain seen from above); ``--bnd none`` draws the fluid alone.

Per point set: one depth call for the chosen frames of the fluid, one for the boundary (the same points into every frame), one
shade call.  A 2-D file (a last dimension of 2, or all z equal) is a ``ValueError``: ``draw_sim2d`` draws those.
"""
import argparse
import sys
from collections import OrderedDict
from pathlib import Path

import numpy as np

from .draw_sim2d import _read_group, draw_labels, select_frames

DEFAULT_HEIGHT = 360
DEFAULT_DIRECTION = (0.8, 0.5, 1.0)  # eye - target of the default camera, before normalisation
DEFAULT_DISTANCE = 1.6               # ... in units of the bounding box's diagonal


def frame_size(height=None, width=None, aspect=16.0 / 9.0):
    """(width, height) of a frame: both as given; one of them from the other by ``aspect`` = width / height, rounded to whole
    pixels; neither: a height of 360."""
    if height is None and width is None:
        height = DEFAULT_HEIGHT
    if not aspect > 0.0:
        raise ValueError(f"--aspect must be positive, got {aspect}")
    if width is None:
        width = int(np.round(height * aspect))
    elif height is None:
        height = int(np.round(width / aspect))
    if width <= 0 or height <= 0:
        raise ValueError(f"the frame size must be positive, got {width} x {height}")
    return int(width), int(height)


def default_pose(bnd, fluid):
    """(eye, target) of the default camera, float64: the target is the centre of the bounding box of ``bnd`` [M, 3] (of
    ``fluid`` [N, 3] when ``bnd`` is empty), the eye ``DEFAULT_DISTANCE`` diagonals away along ``DEFAULT_DIRECTION``."""
    pts = np.asarray(bnd if len(bnd) else fluid, dtype=np.float64).reshape(-1, 3)
    pts = pts[np.isfinite(pts).all(axis=1)]
    if not len(pts):
        raise ValueError("no finite point to aim the default camera at (pass --eye and --target)")
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    target = 0.5 * (lo + hi)
    diagonal = float(np.linalg.norm(hi - lo))
    if not diagonal > 0.0:
        diagonal = 1.0
    d = np.asarray(DEFAULT_DIRECTION, dtype=np.float64)
    return target + DEFAULT_DISTANCE * diagonal * d / np.linalg.norm(d), target


def _device(device):
    import torch
    if device is None:
        if not torch.cuda.is_available():
            raise RuntimeError("draw_sim3d renders on the GPU (ops.splat_depth / ops.splat_shade): no GPU is visible")
        device = "cuda"
    return torch.device(device)


def draw_frames(bnd, particles, camera, width, height, particle_color, boundary_color, particle_radius, boundary_radius,
                bnd_mode="far", ambient=0.3, device=None):
    """F frames in three calls: the depth pass of ``particles`` [F, N, 3], the depth pass of ``bnd`` [M, 3] (the same boundary
    into every frame; skipped for ``bnd_mode`` 'none'), one shade pass with the fluid as layer 0.  Returns uint8 RGBA
    [F, height, width, 4]."""
    import torch

    from .. import ops
    if bnd_mode not in ("far", "near", "none"):
        raise ValueError(f"bnd_mode must be 'far', 'near' or 'none', got {bnd_mode!r}")
    dev = _device(device)
    p = torch.as_tensor(np.ascontiguousarray(particles, dtype=np.float32)).to(dev)
    if p.dim() != 3 or p.shape[-1] != 3:
        raise ValueError(f"particles must have shape [F, N, 3], got {tuple(p.shape)}")
    layers = [ops.SplatLayer(ops.splat_depth(p, float(particle_radius), camera, width, height), p, float(particle_radius),
                             int(particle_color), False)]
    if bnd_mode != "none":
        b = torch.as_tensor(np.ascontiguousarray(np.reshape(bnd, (-1, 3)), dtype=np.float32)).to(dev)
        far = bnd_mode == "far"
        keys = torch.full((p.shape[0], int(height), int(width)), -1, dtype=torch.int64, device=dev)
        ops.splat_depth(b, float(boundary_radius), camera, width, height, farthest=far, out=keys)
        layers.append(ops.SplatLayer(keys, b, float(boundary_radius), int(boundary_color), far))
    img = ops.splat_shade(layers, camera, width, height, ambient=float(ambient))
    return ops.rgba8(img).cpu().numpy()


def _parser():
    ap = argparse.ArgumentParser(description="Draw frames of a 3-D result file (HDF5 or .npz) into one PNG: a row per point set.",
                                 formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    ap.add_argument("path", type=str, help="result file written by run_test / run_sample")
    ap.add_argument("output", type=str, help="PNG to write")
    ap.add_argument("--out_pattern", type=str,
                    help="also write every drawn frame on its own, to this str.format pattern with the fields {pointset} and {frame}")
    ap.add_argument("--height", type=int, help=f"frame height in pixels ({DEFAULT_HEIGHT} when neither --height nor --width is given)")
    ap.add_argument("--width", type=int, help="frame width in pixels")
    ap.add_argument("--aspect", type=float, default=16.0 / 9.0, help="width / height, used when only one of --height / --width is given")
    ap.add_argument("--pr", dest="particle_radius", type=float, default=0.005, help="fluid sphere radius, simulation units")
    ap.add_argument("--br", dest="boundary_radius", type=float, help="boundary sphere radius, simulation units (default: --pr)")
    ap.add_argument("--pointsets", type=str, nargs="+", default=["gt,GT", "pred,Ours"], help="one 'dataset,label' entry per row")
    ap.add_argument("--font_size", type=float, default=36.0, help="label text size")
    ap.add_argument("--num_frames", type=int, default=5, help="how many evenly spread frames to draw")
    ap.add_argument("--frames", type=int, nargs="+", help="explicit frame indices (replaces --num_frames)")
    ap.add_argument("--pc", type=str, default="0xff0071c5", help="fluid colour, hexadecimal 0xAARRGGBB")
    ap.add_argument("--bc", type=str, default="0xff9e9e9e", help="boundary colour, hexadecimal 0xAARRGGBB")
    ap.add_argument("--eye", type=float, nargs=3, metavar=("X", "Y", "Z"), help="camera position (default: from the bounding box)")
    ap.add_argument("--target", type=float, nargs=3, metavar=("X", "Y", "Z"), help="point the camera looks at (default: the box centre)")
    ap.add_argument("--up", type=float, nargs=3, metavar=("X", "Y", "Z"), default=[0.0, 1.0, 0.0], help="world direction that is up in the image")
    ap.add_argument("--fov", type=float, default=35.0, help="vertical field of view of the perspective camera, degrees")
    ap.add_argument("--ortho", type=float, metavar="H", help="orthographic camera showing H simulation units from top to bottom")
    ap.add_argument("--bnd", type=str, choices=["far", "near", "none"], default="far",
                    help="boundary layer: its farthest sphere per pixel (closed boxes), its nearest, or no boundary")
    ap.add_argument("--ambient", type=float, default=0.3, help="ambient share of the headlight shading, in [0, 1]")
    return ap


def _require_3d(path, data, names):
    for name in names:
        arr = data[name]
        if arr.shape[-1] == 2:
            raise ValueError(f"{path}: {name!r} holds 2-D points (shape {arr.shape}): draw_sim2d draws 2-D result files")
        if arr.shape[-1] != 3:
            raise ValueError(f"{path}: {name!r} must hold points [..., 3], got shape {arr.shape}")
    z = np.concatenate([np.asarray(data[name][..., 2]).reshape(-1) for name in names])
    z = z[np.isfinite(z)]
    if z.size and (z == z[0]).all():
        raise ValueError(f"{path}: every z is {z[0]}: a 2-D scene, which draw_sim2d draws")


def main(argv=None):
    from PIL import Image

    from .. import ops
    ap = _parser()
    argv = sys.argv[1:] if argv is None else list(argv)
    if not argv:
        ap.print_help(sys.stderr)
        return 1
    opt = ap.parse_args(argv)
    fluid_argb, boundary_argb = int(opt.pc, base=16), int(opt.bc, base=16)

    data = _read_group(opt.path)
    rows_spec = [(entry.split(",")[0], entry.split(",")[-1]) for entry in opt.pointsets]
    names = [n for n, _ in rows_spec] + ["bnd"]
    for name in names:
        if name not in data:
            raise ValueError(f"{opt.path}: no point set {name!r} (the group holds {', '.join(data)})")
    _require_3d(opt.path, data, names)

    width, height = frame_size(opt.height, opt.width, opt.aspect)
    fluid_r = opt.particle_radius
    boundary_r = fluid_r if opt.boundary_radius is None else opt.boundary_radius
    seq_len = OrderedDict((k, arr.shape[0]) for k, arr in data.items() if arr.ndim == 3)
    frames = select_frames(seq_len, opt.num_frames, opt.frames)
    for name, _ in rows_spec:
        seq = data[name]
        if seq.ndim != 3:
            raise ValueError(f"point set {name!r} is not a sequence [T, N, d] (shape {seq.shape})")
        bad = [f for f in frames if not -seq.shape[0] <= f < seq.shape[0]]
        if bad:
            raise ValueError(f"frame {bad[0]} is outside the point set {name!r} of {seq.shape[0]} frames")

    boundary = np.reshape(data["bnd"], (-1, 3))
    eye, target = default_pose(boundary, data[rows_spec[0][0]][frames[0]])
    eye = eye if opt.eye is None else np.asarray(opt.eye, dtype=np.float64)
    target = target if opt.target is None else np.asarray(opt.target, dtype=np.float64)
    camera = ops.look_at(eye, target, opt.up, width, height, fov_deg=opt.fov, ortho_height=opt.ortho)
    print(f"draw_sim3d: {opt.path} -> {opt.output}: {width} x {height} px per frame, frames {[int(f) for f in frames]} "
          f"(sequence lengths {dict(seq_len)}), eye {np.round(eye, 4).tolist()}, target {np.round(target, 4).tolist()}")

    labels = draw_labels([label for _, label in rows_spec], height, opt.font_size)
    rows = []
    for (name, _), label in zip(rows_spec, labels):
        tiles = draw_frames(boundary, data[name][np.asarray(frames)], camera, width, height, fluid_argb, boundary_argb, fluid_r,
                            boundary_r, bnd_mode=opt.bnd, ambient=opt.ambient)
        if opt.out_pattern:
            for f, tile in zip(frames, tiles):
                out = Path(opt.out_pattern.format(pointset=name, frame=f))
                out.parent.mkdir(parents=True, exist_ok=True)
                Image.fromarray(tile, "RGBA").save(str(out))
        rows.append(np.concatenate([label, *tiles], axis=1))
    Image.fromarray(np.concatenate(rows, axis=0), "RGBA").save(opt.output)
    return 0


if __name__ == "__main__":
    sys.exit(main())
