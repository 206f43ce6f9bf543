"""A numpy restatement of the sphere splat's pixel model (include/dmcf_hip.h, "Depth-tested sphere splat"): every operation is
one float32 operation in the header's order (numpy rounds each float32 product, sum, quotient and square root to nearest and
fuses nothing), so the key map, the depth and -- up to the last place of the compositing -- the image of the HIP kernels are
reproduced.  Brute force: every sphere against every pixel of the image.

A camera is any object with the attributes of ``ops.Camera``: view (12 values, row-major 3 x 4), focal, cx, cy, near,
orthographic.
"""
import collections

import numpy as np

F32 = np.float32
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)

Cam = collections.namedtuple("Cam", ["view", "focal", "cx", "cy", "near", "orthographic"])
Layer = collections.namedtuple("Layer", ["keys", "xyz", "radius", "color_argb", "farthest"])


def project(cam, xyz, radius, min_px):
    """Per sphere of ``xyz`` [n, 3]: dict of float32 arrays sx, sy, R, R2, zc, m and the bool array live (false: skipped)."""
    p = np.asarray(xyz, dtype=F32).reshape(-1, 3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    v = np.asarray(cam.view, dtype=F32)
    with np.errstate(all="ignore"):
        row = lambda i: ((v[4 * i] * x + v[4 * i + 1] * y) + v[4 * i + 2] * z) + v[4 * i + 3]  # noqa: E731
        xc, yc, zc = row(0), row(1), row(2)
        focal = F32(cam.focal)
        m = np.full_like(zc, focal) if cam.orthographic else focal / zc
        sx = F32(cam.cx) + m * xc
        sy = F32(cam.cy) + m * yc
        R = np.maximum(m * F32(radius), F32(min_px))
        R2 = R * R
        live = np.isfinite(p).all(axis=1) & (zc > F32(cam.near))
    return dict(sx=sx, sy=sy, R=R, R2=R2, zc=zc, m=m, live=live)


def _pixel_terms(s, i, width, height):
    """d2 [H, W] of sphere i (float32, the header's order)."""
    dx = (np.arange(width, dtype=F32) + F32(0.5)) - s["sx"][i]
    dy = (np.arange(height, dtype=F32) + F32(0.5)) - s["sy"][i]
    return (dx * dx)[None, :] + (dy * dy)[:, None]


def depth_keys(cam, xyz, radius, width, height, frames=None, farthest=False, min_px=0.75, keys=None):
    """The key map uint64 [F, H, W] after splatting ``xyz`` ([F, n, 3], or [n, 3]: the same points into all ``frames``) into
    ``keys`` (all empty when None)."""
    xyz = np.asarray(xyz, dtype=F32)
    if xyz.ndim == 2:
        frames = 1 if frames is None and keys is None else (frames if keys is None else keys.shape[0])
        xyz = np.broadcast_to(xyz, (frames,) + xyz.shape)
    F = xyz.shape[0]
    keys = np.full((F, height, width), EMPTY, dtype=np.uint64) if keys is None else keys.copy()
    if not (np.isfinite(radius) and radius > 0):
        return keys
    near = F32(cam.near)
    for f in range(F):
        s = project(cam, xyz[f], radius, min_px)
        for i in np.flatnonzero(s["live"]):
            with np.errstate(all="ignore"):
                d2 = _pixel_terms(s, i, width, height)
                cover = d2 < s["R2"][i]
                z = s["zc"][i] - np.sqrt(s["R2"][i] - d2) / s["m"][i]
                ok = cover & np.isfinite(z) & (z > near)
            bits = z.astype(F32).view(np.uint32)
            hi = (~bits if farthest else bits).astype(np.uint64)
            key = (hi << np.uint64(32)) | np.uint64(i)
            keys[f] = np.where(ok, np.minimum(keys[f], key), keys[f])
    return keys


def decode(keys, farthest):
    """(depth float32 with +inf where empty, index int64 with -1 where empty) of a key map."""
    keys = np.asarray(keys).view(np.uint64)
    hi = (keys >> np.uint64(32)).astype(np.uint32)
    z = (~hi if farthest else hi).view(F32).copy()
    idx = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    empty = keys == EMPTY
    z[empty] = np.inf
    idx[empty] = -1
    return z, idx


def shade(cam, layers, width, height, image, ambient=0.3, min_px=0.75):
    """(image float32 [F, H, W, 3], depth float32 [F, H, W]) after the shade pass over ``layers`` (``Layer`` tuples, keys as
    uint64 or int64 bits) composited onto a copy of ``image``."""
    image = np.array(image, dtype=F32)
    F = image.shape[0]
    best = np.full((F, height, width), np.inf, dtype=F32)
    which = np.full((F, height, width), -1, dtype=np.int64)
    index = np.full((F, height, width), -1, dtype=np.int64)
    for j, layer in enumerate(layers):
        z, idx = decode(layer.keys, layer.farthest)
        take = z < best  # strict: ties stay with the lower layer
        best[take], which[take], index[take] = z[take], j, idx[take]
    amb = F32(ambient)
    px = np.arange(width, dtype=F32) + F32(0.5)
    py = np.arange(height, dtype=F32) + F32(0.5)
    for j, layer in enumerate(layers):
        xyz = np.asarray(layer.xyz, dtype=F32)
        argb = int(layer.color_argb)
        a = F32((argb >> 24) & 255) / F32(255)
        col = [F32((argb >> sh) & 255) / F32(255) for sh in (16, 8, 0)]
        for f in range(F):
            s = project(cam, xyz[f] if xyz.ndim == 3 else xyz, layer.radius, min_px)
            rows, cols = np.nonzero(which[f] == j)
            if not len(rows):
                continue
            i = index[f, rows, cols]
            dx, dy = px[cols] - s["sx"][i], py[rows] - s["sy"][i]
            d2 = dx * dx + dy * dy
            nz = np.sqrt(np.maximum(s["R2"][i] - d2, F32(0))) / s["R"][i]
            sh = amb + (F32(1) - amb) * nz
            for ch in range(3):
                C = image[f, rows, cols, ch]
                image[f, rows, cols, ch] = C * (F32(1) - a) + (col[ch] * sh) * a
    return image, best


def rgba8(image):
    q = np.clip(np.round(np.asarray(image, dtype=F32) * F32(255)), 0, 255).astype(np.uint8)
    return np.concatenate([q, np.full_like(q[..., :1], 255)], axis=-1)


def look_at(eye, target, up, width, height, fov_deg=35.0, ortho_height=None, near=1e-3):
    """The camera of ``ops.look_at`` in float64, unrounded: (view [3, 4], focal, cx, cy, near)."""
    eye, target, up = (np.asarray(v, dtype=np.float64) for v in (eye, target, up))
    f = (target - eye) / np.linalg.norm(target - eye)
    r = np.cross(f, up)
    r = r / np.linalg.norm(r)
    d = np.cross(f, r)
    rows = np.stack([r, d, f])
    view = np.concatenate([rows, -(rows @ eye)[:, None]], axis=1)
    focal = 0.5 * height / np.tan(np.deg2rad(fov_deg) / 2) if ortho_height is None else height / ortho_height
    return view, focal, 0.5 * width, 0.5 * height, near
