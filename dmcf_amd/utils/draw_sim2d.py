"""Renders a 2-D simulation result file: the reference's ``utils/draw_sim2d.py``, restated from its behaviour, with the discs
drawn on the GPU (``ops.raster_discs``, dmcf_amd/csrc/raster.hip) instead of one skia ``canvas.drawCircle`` per particle.

    python -m dmcf_amd.utils.draw_sim2d <result.hdf5 | .npz> <out.png> [--out_pattern 'dir/{pointset}_{frame:04d}.png']
        [--height 360 | --width W] [--pr 0.005] [--br R] [--margin 0.1] [--pointsets gt,GT pred,Ours] [--font_size 36]
        [--num_frames 5 | --frames i j ...] [--pc 0xff0071c5]

Same flags, defaults and arithmetic as the reference (``:85-229``): the group ``SymNet`` (or the file's only group); x and y
with y mirrored; the canvas from the bounding box of ``bnd`` ([-0.5, 0.5]^2 when it is empty) grown by the margin, scaled to
``--height`` (or ``--width``) with the other side ``int(np.round(...))``; radii in simulation units scaled alike; frames from
``np.array_split(range(T), num_frames)`` over the shortest sequence, or ``--frames``.  Output (``:233-257``): one row per point
set -- its label, then its frames -- rows stacked; ``--out_pattern`` files per (point set, frame).  Fluid particles are drawn
first, the boundary (colour 0xff000000) on top, as the reference's two loops do (``:29-43``).

Deliberate differences from skia, whose output therefore is not reproduced pixel for pixel (skia is not a dependency here, so
that equality is neither checked nor claimed):

  - anti-aliasing follows the pixel model of include/dmcf_hip.h (coverage ``clamp(r + 0.5 - d, 0, 1) * min(1, 2r)``);
  - compositing is done in float over the whole group and rounded to 8 bits once at the end;
  - the labels' glyphs come from Pillow's default font (FreeType), not skia's;
  - images are RGBA; skia's ``Surface.toarray()`` returns its N32 colour type, which is BGRA on little-endian machines.

Where the reference would crash, a ``ValueError`` says why: ``num_frames`` larger than the shortest sequence, a point set the
file does not hold, a frame outside a sequence, a file with a single sequence (``min(*lengths)`` of one length).
"""
import argparse
import sys
from collections import OrderedDict
from pathlib import Path

import numpy as np

BOUNDARY_COLOR = 0xff000000


def _device(device):
    import torch
    if device is None:
        if not torch.cuda.is_available():
            raise RuntimeError("draw_sim2d renders on the GPU (ops.raster_discs): no GPU is visible")
        device = "cuda"
    return torch.device(device)


def draw_frames(bnd, particles, width, height, particle_color, boundary_color, particle_radius, boundary_radius, device=None):
    """F frames in two raster calls: ``particles`` [F, N, 2] (pixel coordinates), then ``bnd`` [M, 2], the same boundary in
    every frame (binned once), on top.  Returns uint8 RGBA [F, height, width, 4]."""
    import torch

    from .. import ops
    dev = _device(device)
    p = torch.as_tensor(np.ascontiguousarray(particles, dtype=np.float32)).to(dev)
    if p.dim() != 3 or p.shape[-1] != 2:
        raise ValueError(f"particles must have shape [F, N, 2], got {tuple(p.shape)}")
    b = torch.as_tensor(np.ascontiguousarray(np.reshape(bnd, (-1, 2)), dtype=np.float32)).to(dev)
    img = torch.ones((p.shape[0], int(height), int(width), 3), dtype=torch.float32, device=dev)
    ops.raster_discs(p, float(particle_radius), int(particle_color), width, height, out=img)
    ops.raster_discs(b, float(boundary_radius), int(boundary_color), width, height, out=img)
    return ops.rgba8(img).cpu().numpy()


def draw_frame(bnd, particles, width, height, particle_color, boundary_color, particle_radius, boundary_radius, **kwargs):
    """The reference's ``draw_frame`` (``:11-45``): white background, the fluid particles ``particles`` [N, 2], then the
    boundary particles ``bnd`` [M, 2] on top, both in pixel coordinates, colours ARGB (e.g. 0xffff0000), radii in pixels.
    Returns the frame as uint8 RGBA [height, width, 4] (skia's ``toarray()`` is N32: BGRA on little-endian).  ``device`` may be
    given among ``kwargs``; the other keywords are ignored, as in the reference, which is called with all of its arguments."""
    return draw_frames(bnd, np.asarray(particles)[None], width, height, particle_color, boundary_color, particle_radius,
                       boundary_radius, device=kwargs.get("device"))[0]


def draw_labels(labels, height, font_size=36, rot90=True):
    """The reference's ``draw_labels`` (``:48-82``): one uint8 RGBA image per label, black anti-aliased text centred on white;
    ``rot90``: [height, w, 4] with the text reading bottom to top, w the tallest label's height (``ceil``); otherwise
    [height, w, 4] with w the widest label's width.  Glyphs from Pillow's default font at ``font_size``."""
    from PIL import Image, ImageDraw, ImageFont
    font = ImageFont.load_default(size=font_size)
    boxes = [font.getbbox(label) for label in labels]
    extent = [(int(np.ceil(b[3] - b[1])) if rot90 else int(np.ceil(b[2] - b[0]))) for b in boxes]
    width = max(max(extent), 1)
    result = []
    for label, (l, t, r, b) in zip(labels, boxes):
        text = Image.new("L", (max(int(np.ceil(r - l)), 1), max(int(np.ceil(b - t)), 1)), 255)
        ImageDraw.Draw(text).text((-l, -t), label, font=font, fill=0)
        if rot90:
            text = text.rotate(90, expand=True)  # counter-clockwise: reads bottom to top
        canvas = Image.new("L", (width, int(height)), 255)
        canvas.paste(text, ((width - text.width) // 2, (int(height) - text.height) // 2))
        grey = np.asarray(canvas, dtype=np.uint8)
        result.append(np.concatenate([np.repeat(grey[..., None], 3, axis=-1), np.full_like(grey[..., None], 255)], axis=-1))
    return result


def canvas_layout(bnd, margin, height=360, width=None):
    """(width, height, scale, shift) of the canvas for the boundary points ``bnd`` [M, 2] (x, mirrored y), as ``:185-204``
    computes them: a pixel position is ``scale * (p + shift)``.  The box of ``bnd`` ([-0.5, 0.5]^2 without points) grows by
    ``margin`` of its size on every side; its lower corner goes to the origin; the given side fixes the scale and the other
    side is rounded to whole pixels."""
    if len(bnd):
        lo, hi = bnd.min(axis=0), bnd.max(axis=0)
    else:
        lo, hi = np.full(2, -0.5), np.full(2, 0.5)
    extent = (1 + 2 * margin) * (hi - lo)
    corner = 0.5 * (lo + hi) - 0.5 * extent
    if width is None:
        scale = height / extent[1]
        width = int(np.round(extent[0] * scale))
    else:
        scale = width / extent[0]
        height = int(np.round(extent[1] * scale))
    return width, height, scale, -corner


def select_frames(lengths, num_frames=5, frames=None):
    """``:217-231``: ``frames`` when given, else the first frame of each of ``np.array_split(range(min(lengths)),
    num_frames)``.  ``lengths``: {array name: sequence length} of the file's particle sequences."""
    if frames is not None:
        return list(frames)
    if len(lengths) < 2:
        raise ValueError(f"the file holds {len(lengths)} particle sequence(s) ({', '.join(lengths) or 'none'}): the reference takes "
                         "min(*lengths) over at least two (pass --frames to choose frames explicitly)")
    shortest = min(lengths.values())
    if num_frames > shortest:
        raise ValueError(f"--num_frames {num_frames} is larger than the shortest sequence ({shortest} frames)")
    return [x[0] for x in np.array_split(np.arange(shortest), num_frames)]


def _parser():
    # flag names, destinations, types and defaults are the reference's (:85-149); the help texts are this project's
    ap = argparse.ArgumentParser(description="Draw frames of a 2-D result file (HDF5 or .npz) into one PNG: a row per point set.",
                                 formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    ap.add_argument("path", type=str, help="result file written by run_test / run_sample")
    ap.add_argument("output", type=str, help="PNG to write")
    ap.add_argument("--out_pattern", type=str,
                    help="also write every drawn frame on its own, to this str.format pattern with the fields {pointset} and {frame}")
    ap.add_argument("--height", type=int, default=360, help="frame height in pixels")
    ap.add_argument("--width", type=int, help="frame width in pixels; when given, the height follows from it instead")
    ap.add_argument("--pr", dest="particle_radius", type=float, default=0.005, help="fluid disc radius, simulation units")
    ap.add_argument("--br", dest="boundary_radius", type=float, help="boundary disc radius, simulation units (default: --pr)")
    ap.add_argument("--margin", type=float, default=0.1, help="border around the boundary's box, as a fraction of its size")
    ap.add_argument("--pointsets", type=str, nargs="+", default=["gt,GT", "pred,Ours"],
                    help="one 'dataset,label' entry per row")
    ap.add_argument("--font_size", type=float, default=36.0, help="label text size")
    ap.add_argument("--num_frames", type=int, default=5, help="how many evenly spread frames to draw")
    ap.add_argument("--frames", type=int, nargs="+", help="explicit frame indices (replaces --num_frames)")
    ap.add_argument("--pc", type=str, default="0xff0071c5", help="fluid colour, hexadecimal 0xAARRGGBB")
    return ap


def _read_group(path):
    """The arrays of the result file's group ``SymNet``; a file with a single group may name it otherwise (``:170-174``)."""
    from .hdf5_reader import read_results
    groups = read_results(path)
    name = "SymNet" if ("SymNet" in groups or len(groups) != 1) else next(iter(groups))
    if name not in groups:
        raise ValueError(f"{path}: no group 'SymNet' and {len(groups)} groups ({', '.join(groups)})")
    return {k: arr for k, (arr, _) in groups[name].items()}


def _plane(v):
    """x and y of points [..., d] with y negated (image rows grow downwards)."""
    return v[..., :2] * np.array([1, -1], dtype=v.dtype)


def main(argv=None):
    from PIL import Image
    ap = _parser()
    argv = sys.argv[1:] if argv is None else list(argv)
    if not argv:
        ap.print_help(sys.stderr)
        return 1
    opt = ap.parse_args(argv)
    fluid_argb = int(opt.pc, base=16)

    data = _read_group(opt.path)
    rows_spec = [(entry.split(",")[0], entry.split(",")[-1]) for entry in opt.pointsets]
    for name in [n for n, _ in rows_spec] + ["bnd"]:
        if name not in data:
            raise ValueError(f"{opt.path}: no point set {name!r} (the group holds {', '.join(data)})")

    boundary = _plane(data["bnd"])
    width, height, scale, shift = canvas_layout(boundary, opt.margin, opt.height, opt.width)
    fluid_r = opt.particle_radius * scale  # radii in pixels (:211-215)
    boundary_r = fluid_r if opt.boundary_radius is None else opt.boundary_radius * scale
    seq_len = OrderedDict((k, arr.shape[0]) for k, arr in data.items() if arr.ndim == 3)
    frames = select_frames(seq_len, opt.num_frames, opt.frames)
    print(f"draw_sim2d: {opt.path} -> {opt.output}: {width} x {height} px per frame, frames {[int(f) for f in frames]} "
          f"(sequence lengths {dict(seq_len)})")

    boundary_px = scale * (boundary + shift)
    labels = draw_labels([label for _, label in rows_spec], height, opt.font_size)
    rows = []
    for (name, _), label in zip(rows_spec, labels):
        seq = data[name]
        if seq.ndim != 3:
            raise ValueError(f"point set {name!r} is not a sequence [T, N, d] (shape {seq.shape})")
        bad = [f for f in frames if not -seq.shape[0] <= f < seq.shape[0]]
        if bad:
            raise ValueError(f"frame {bad[0]} is outside the point set {name!r} of {seq.shape[0]} frames")
        tiles = draw_frames(boundary_px, scale * (_plane(seq[np.asarray(frames)]) + shift), width, height, fluid_argb,
                            BOUNDARY_COLOR, fluid_r, boundary_r)
        if opt.out_pattern:
            for f, tile in zip(frames, tiles):
                target = Path(opt.out_pattern.format(pointset=name, frame=f))
                target.parent.mkdir(parents=True, exist_ok=True)
                Image.fromarray(tile, "RGBA").save(str(target))
        rows.append(np.concatenate([label, *tiles], axis=1))
    Image.fromarray(np.concatenate(rows, axis=0), "RGBA").save(opt.output)
    return 0


if __name__ == "__main__":
    sys.exit(main())
