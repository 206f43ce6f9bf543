"""Float64 restatement of the renderer for the tests: the pixel model of include/dmcf_hip.h (dmcf_raster_discs) and the
layout arithmetic of the reference's utils/draw_sim2d.py:185-214, written independently of dmcf_amd."""
import numpy as np


def coverage(xy, radius, x0, x1, y0, y1):
    """cov [n, y1 - y0, x1 - x0] of the discs ``xy`` [n, 2] over the pixels [x0, x1) x [y0, y1) (float64):
    clamp(r + 0.5 - |p - centre|, 0, 1) * min(1, 2 r); 0 for discs whose centre is not finite or r <= 0."""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    r = float(radius)
    px = np.arange(x0, x1, dtype=np.float64) + 0.5
    py = np.arange(y0, y1, dtype=np.float64) + 0.5
    if not (np.isfinite(r) and r > 0) or len(xy) == 0:
        return np.zeros((len(xy), len(py), len(px)))
    ok = np.isfinite(xy).all(axis=1)
    c = np.where(ok[:, None], xy, 0.0)
    d = np.sqrt((px[None, None, :] - c[:, 0, None, None]) ** 2 + (py[None, :, None] - c[:, 1, None, None]) ** 2)
    cov = np.clip(r + 0.5 - d, 0.0, 1.0) * min(1.0, 2.0 * r)
    cov[~ok] = 0.0
    return cov


def transmittance(xy, radius, alpha, x0, x1, y0, y1, chunk=2048):
    """(T, k) over the pixels [x0, x1) x [y0, y1): T = prod (1 - a cov), a = alpha / 255, and k the number of discs with
    cov > 0.  Only discs that can reach the region are evaluated."""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    a = alpha / 255.0
    reach = float(radius) + 1.0
    with np.errstate(invalid="ignore"):
        near = ((xy[:, 0] > x0 - reach) & (xy[:, 0] < x1 + reach) & (xy[:, 1] > y0 - reach) & (xy[:, 1] < y1 + reach))
    sel = xy[near]
    T = np.ones((y1 - y0, x1 - x0))
    k = np.zeros((y1 - y0, x1 - x0), dtype=np.int64)
    for s in range(0, len(sel), chunk):
        cov = coverage(sel[s:s + chunk], radius, x0, x1, y0, y1)
        T *= np.prod(1.0 - a * cov, axis=0)
        k += (cov > 0).sum(axis=0)
    return T, k


def argb(color):
    return (color >> 24) / 255.0, np.array([(color >> 16) & 255, (color >> 8) & 255, color & 255], dtype=np.float64) / 255.0


def composite(image, T, color):
    """C T + colour (1 - T) over float64 RGB [..., 3]."""
    _, col = argb(color)
    return image * T[..., None] + col * (1.0 - T[..., None])


def raster(xy, radius, color, width, height, image=None):
    """Whole-image restatement: ``xy`` [F, n, 2] or [n, 2] (the same points in every frame) -> (image [F, H, W, 3], T [F, H, W],
    k [F, H, W]) composited over ``image`` (white when None)."""
    xy = np.asarray(xy, dtype=np.float64)
    frames = xy.shape[0] if xy.ndim == 3 else (1 if image is None else image.shape[0])
    img = np.ones((frames, height, width, 3)) if image is None else np.asarray(image, dtype=np.float64).copy()
    Ts, ks = [], []
    for f in range(frames):
        T, k = transmittance(xy[f] if xy.ndim == 3 else xy, radius, color >> 24, 0, width, 0, height)
        img[f] = composite(img[f], T, color)
        Ts.append(T)
        ks.append(k)
    return img, np.stack(Ts), np.stack(ks)


def rgba8(image):
    """round(255 C) half to even, alpha 255 (float64)."""
    q = np.clip(np.round(np.asarray(image, dtype=np.float64) * 255.0), 0, 255).astype(np.uint8)
    return np.concatenate([q, np.full(q.shape[:-1] + (1,), 255, np.uint8)], axis=-1)


def layout(bnd, margin, height=360, width=None, particle_radius=0.005, boundary_radius=None):
    """utils/draw_sim2d.py:185-215 as written there: (width, height, scale, shift, particle radius, boundary radius) in pixels
    for the boundary points ``bnd`` [M, 2] (x and mirrored y)."""
    if len(bnd) > 0:
        lo, hi = bnd.min(axis=0), bnd.max(axis=0)
    else:
        lo, hi = np.full(2, -0.5), np.full(2, 0.5)
    size = (1 + 2 * margin) * (hi - lo)
    center = 0.5 * (lo + hi)
    shift = -(center - 0.5 * size)
    if width is not None:
        scale = width / size[0]
        height = int(np.round(size[1] * scale))
    else:
        scale = height / size[1]
        width = int(np.round(size[0] * scale))
    pr = particle_radius * scale
    br = pr if boundary_radius is None else boundary_radius * scale
    return width, height, scale, shift, pr, br
