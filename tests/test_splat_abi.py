"""CPU checks of the 3-D renderer (ABI 2.27: dmcf_splat_depth / dmcf_splat_shade, ops.look_at, dmcf_amd/utils/draw_sim3d.py): the
symbols and the camera struct against the header, every host-side refusal on fake addresses (no device is touched), look_at
against a float64 computation, the command line's defaults and default camera, the refusal of 2-D files, and the sanity of the
restatement tests/splat_ref.py itself.  The kernels run in tests/test_gpu_splat.py."""
import ctypes
import os
import re

import numpy as np
import pytest

import splat_ref as S
from dmcf_amd.datasets import write_results
from dmcf_amd.utils import draw_sim3d as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


@pytest.fixture(scope="module")
def hip_lib():
    from dmcf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def _header():
    return open(os.path.join(ROOT, "include", "dmcf_hip.h")).read()


def test_symbols_declared_listed_and_exported(hip_lib):
    from dmcf_amd import _lib
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in ("dmcf_splat_depth", "dmcf_splat_shade"):
        assert re.search(r"\b" + name + r"\s*\(", code), name
        assert name in _lib.SYMBOLS and hasattr(hip_lib, name)
    assert name in _header()[:_header().index("#ifndef DMCF_HIP_H_")]  # the table at the top of the header
    assert hip_lib.dmcf_version() >= 22700
    assert re.search(r"#define DMCF_SPLAT_FARTHEST 1\b", code) and _lib.SPLAT_FARTHEST == 1
    assert re.search(r"#define DMCF_SPLAT_MAX_LAYERS 4\b", code) and _lib.SPLAT_MAX_LAYERS == 4


def test_struct_mirrors_match_the_header():
    from dmcf_amd import _lib
    text = _header()
    for cname, mirror in (("dmcf_camera", _lib.Camera), ("dmcf_splat_layer", _lib.SplatLayer)):
        body = text[text.index("typedef struct %s {" % cname):text.index("} %s;" % cname)]
        size = int(re.search(r"sizeof\(%s\) = (\d+)" % cname, body).group(1))
        assert ctypes.sizeof(mirror) == size, cname
        fields = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        decls = re.findall(r"^\s*(?:const\s+)?\w+\s*\*?\s+([a-z_]+(?:\s*,\s*[a-z_]+)*)(?:\[\d+\])?;", fields, flags=re.M)
        names = [n for decl in decls for n in decl.replace(" ", "").split(",")]
        assert names == [f[0] for f in mirror._fields_], cname
    assert int(re.search(r"struct dmcf_camera, sizeof = (\d+)", text).group(1)) == ctypes.sizeof(_lib.Camera) == 80
    assert _lib.Camera.focal.offset == 48 and _lib.Camera.orthographic.offset == 64
    assert _lib.SplatLayer.radius.offset == 32 and ctypes.sizeof(_lib.SplatLayer) == 48


def _camera(**kw):
    from dmcf_amd import _lib
    c = _lib.Camera()
    c.view = (ctypes.c_float * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
    c.focal, c.cx, c.cy, c.near = 100.0, 32.0, 24.0, 1e-3
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_depth_host_validation(hip_lib):
    L = hip_lib
    buf = ctypes.create_string_buffer(64)
    a8 = ctypes.addressof(buf) + (-ctypes.addressof(buf) % 8)  # a fake aligned address: never dereferenced by a refusal
    cam = ctypes.byref(_camera())

    def depth(xyz=a8, n=100, F=3, stride=100, radius=0.1, min_px=0.75, camera=cam, W=64, H=48, flags=0, keys=a8):
        return L.dmcf_splat_depth(xyz, n, F, stride, radius, min_px, camera, W, H, flags, keys, None)

    assert depth(keys=None) == EINVAL
    assert depth(xyz=None) == EINVAL
    assert depth(camera=None) == EINVAL
    assert depth(n=-1) == EINVAL and depth(F=-3) == EINVAL and depth(stride=-1) == EINVAL
    assert depth(n=1 << 31, stride=1 << 31) == EINVAL  # the index is the key's low word
    assert depth(stride=50) == EINVAL  # overlapping frames: 0 < stride < n
    assert depth(F=65536) == EINVAL
    assert depth(W=0) == EINVAL and depth(H=-48) == EINVAL
    assert depth(W=32769) == EINVAL and depth(H=32769) == EINVAL
    assert depth(flags=2) == EINVAL
    assert depth(keys=a8 + 4) == EINVAL and depth(xyz=a8 + 2) == EINVAL  # misaligned
    assert depth(min_px=-1.0) == EINVAL and depth(min_px=float("nan")) == EINVAL
    assert depth(camera=ctypes.byref(_camera(focal=0.0))) == EINVAL
    assert depth(camera=ctypes.byref(_camera(near=-1.0))) == EINVAL
    assert depth(camera=ctypes.byref(_camera(cx=float("inf")))) == EINVAL
    bad = _camera()
    bad.view[7] = float("nan")
    assert depth(camera=ctypes.byref(bad)) == EINVAL
    # valid calls that splat nothing return before any device work
    assert depth(radius=0.0) == 0 and depth(radius=float("nan")) == 0 and depth(radius=float("inf")) == 0
    assert depth(n=0, stride=0) == 0 and depth(F=0) == 0
    assert depth(W=32768, H=32768, radius=-1.0) == 0  # the limit itself is legal


def test_shade_host_validation(hip_lib):
    from dmcf_amd import _lib
    L = hip_lib
    buf = ctypes.create_string_buffer(64)
    a8 = ctypes.addressof(buf) + (-ctypes.addressof(buf) % 8)
    cam = ctypes.byref(_camera())

    def layers(count, **kw):
        recs = (_lib.SplatLayer * max(count, 1))()
        for r in recs:
            r.keys, r.xyz, r.n_points, r.frame_stride, r.radius, r.color_argb = a8, a8, 100, 100, 0.1, 0xff0071c5
            for k, v in kw.items():
                setattr(r, k, v)
        return recs

    def shade(recs, count, camera=cam, min_px=0.75, ambient=0.3, W=64, H=48, F=3, image=a8, depth=None):
        return L.dmcf_splat_shade(recs, count, camera, min_px, ambient, W, H, F, image, depth, None)

    assert shade(layers(5), 5) == EINVAL  # more than 4 layers
    assert shade(layers(1), -1) == EINVAL
    assert shade(None, 2) == EINVAL
    assert shade(layers(2), 2, image=None) == EINVAL
    assert shade(layers(2), 2, camera=None) == EINVAL
    assert shade(layers(2), 2, W=32769) == EINVAL and shade(layers(2), 2, H=0) == EINVAL
    assert shade(layers(2), 2, F=-1) == EINVAL and shade(layers(2), 2, F=65536) == EINVAL
    assert shade(layers(2), 2, ambient=1.5) == EINVAL and shade(layers(2), 2, ambient=float("nan")) == EINVAL
    assert shade(layers(2), 2, min_px=-0.5) == EINVAL
    assert shade(layers(2, keys=None), 2) == EINVAL
    assert shade(layers(2, xyz=None), 2) == EINVAL
    assert shade(layers(2, keys=a8 + 4), 2) == EINVAL
    assert shade(layers(2, frame_stride=50), 2) == EINVAL  # overlapping frames
    assert shade(layers(2, n_points=-1), 2) == EINVAL
    assert shade(layers(2, flags=4), 2) == EINVAL
    assert shade(layers(2), 2, image=a8 + 2) == EINVAL
    # nothing to shade: no device work
    assert shade(layers(2), 2, F=0) == 0
    assert shade(layers(0), 0) == 0
    assert shade(layers(3, radius=0.0), 3) == 0


def test_ops_validation_runs_before_any_pointer_reaches_the_library(hip_lib):
    import torch

    from dmcf_amd import _lib, ops
    cam = ops.look_at((0, 0, -3), (0, 0, 0), (0, 1, 0), 16, 12)
    with pytest.raises(_lib.DmcfError):
        ops.splat_depth(torch.zeros(5, 3), 0.1, cam, 16, 12)  # a CPU tensor: no fallback
    with pytest.raises(ValueError):
        ops.splat_depth(torch.zeros(5, 2), 0.1, cam, 16, 12)
    with pytest.raises(TypeError):
        ops.splat_depth(np.zeros((5, 3), np.float32), 0.1, cam, 16, 12)
    with pytest.raises(TypeError):
        ops.splat_depth(torch.zeros(5, 3), 0.1, (1, 2, 3), 16, 12)
    with pytest.raises(ValueError):
        ops.splat_depth(torch.zeros(5, 3), 0.1, cam, 40000, 12)
    with pytest.raises(ValueError):
        ops.splat_depth(torch.zeros(5, 3), 0.1, cam, 16, 12, min_px=float("nan"))
    layer = ops.SplatLayer(torch.zeros(1, 12, 16, dtype=torch.int64), torch.zeros(5, 3), 0.1, 0xff0071c5)
    assert layer.farthest is False
    with pytest.raises(ValueError, match="at most 4 layers"):
        ops.splat_shade([layer] * 5, cam, 16, 12)
    with pytest.raises(_lib.DmcfError):
        ops.splat_shade([layer], cam, 16, 12)
    with pytest.raises(ValueError):
        ops.splat_shade([layer], cam, 16, 12, ambient=2.0)
    with pytest.raises(TypeError):
        ops.splat_shade([("keys", "xyz")], cam, 16, 12)


@pytest.mark.parametrize("ortho", [None, 2.5])
def test_look_at_equals_a_float64_computation(ortho):
    from dmcf_amd import ops
    rng = np.random.default_rng(11)
    for _ in range(20):
        eye, target, up = rng.normal(size=3) * 3, rng.normal(size=3), rng.normal(size=3)
        W, H = int(rng.integers(8, 2000)), int(rng.integers(8, 1200))
        fov = float(rng.uniform(10, 120))
        cam = ops.look_at(eye, target, up, W, H, fov_deg=fov, ortho_height=ortho, near=0.01)
        view, focal, cx, cy, near = S.look_at(eye, target, up, W, H, fov, ortho, 0.01)
        assert np.array_equal(np.float32(cam.view), view.astype(np.float32).reshape(-1))  # float64, rounded once
        assert cam.focal == float(np.float32(focal)) and (cam.cx, cam.cy) == (W / 2, H / 2)
        assert cam.near == float(np.float32(near)) and cam.orthographic == (ortho is not None)
        v = np.float64(cam.view).reshape(3, 4)
        R = v[:, :3]
        assert np.allclose(R @ R.T, np.eye(3), atol=1e-6) and np.linalg.det(R) > 0.999  # a rotation: right-handed
        # a point on the view axis projects to the principal point, at its distance from the eye
        for t in (0.5, 1.0, 7.0):
            p = eye + t * (target - eye)
            c = v @ np.append(p, 1.0)
            d = t * np.linalg.norm(target - eye)
            assert abs(c[0]) < 1e-5 * (1 + d) and abs(c[1]) < 1e-5 * (1 + d) and abs(c[2] - d) < 1e-5 * (1 + d)
            m = cam.focal if cam.orthographic else cam.focal / c[2]
            assert abs(cam.cx + m * c[0] - W / 2) < 1e-2 and abs(cam.cy + m * c[1] - H / 2) < 1e-2
        # up points up in the image: a step along up lowers the row (y is down)
        c0, c1 = v @ np.append(target, 1.0), v @ np.append(target + 0.1 * up, 1.0)
        assert c1[1] < c0[1]
    # focal: 0.5 H / tan(fov / 2), or H / ortho_height
    cam = ops.look_at((0, 0, -3), (0, 0, 0), (0, 1, 0), 640, 480, fov_deg=90.0, ortho_height=ortho)
    assert cam.focal == (240.0 if ortho is None else float(np.float32(480 / 2.5)))
    assert cam.view == (-1.0, 0.0, 0.0, 0.0, 0.0, -1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 3.0) or \
        np.allclose(cam.view, (-1, 0, 0, 0, 0, -1, 0, 0, 0, 0, 1, 3))


def test_look_at_refuses_degenerate_input():
    from dmcf_amd import ops
    with pytest.raises(ValueError, match="coincide"):
        ops.look_at((1, 2, 3), (1, 2, 3), (0, 1, 0), 64, 48)
    with pytest.raises(ValueError, match="parallel"):
        ops.look_at((0, 0, 0), (0, 5, 0), (0, 1, 0), 64, 48)
    with pytest.raises(ValueError, match="parallel"):
        ops.look_at((0, 0, 0), (0, 0, 1), (0, 0, 0), 64, 48)
    with pytest.raises(ValueError, match="finite"):
        ops.look_at((0, 0, float("nan")), (0, 0, 1), (0, 1, 0), 64, 48)
    with pytest.raises(ValueError):
        ops.look_at((0, 0, 0), (0, 0, 1), (0, 1, 0), 0, 48)
    with pytest.raises(ValueError):
        ops.look_at((0, 0, 0), (0, 0, 1), (0, 1, 0), 64, 48, fov_deg=180.0)
    with pytest.raises(ValueError):
        ops.look_at((0, 0, 0), (0, 0, 1), (0, 1, 0), 64, 48, ortho_height=0.0)
    with pytest.raises(ValueError):
        ops.look_at((0, 0, 0), (0, 0, 1), (0, 1, 0), 64, 48, near=-1.0)
    with pytest.raises(ValueError):
        ops.look_at((0, 0), (0, 0, 1), (0, 1, 0), 64, 48)


def test_cli_defaults():
    from dmcf_amd.utils import draw_sim2d as D2
    args = vars(D._parser().parse_args(["in.hdf5", "out.png"]))
    assert args.pop("path") == "in.hdf5" and args.pop("output") == "out.png"
    assert args == dict(out_pattern=None, height=None, width=None, aspect=16.0 / 9.0, particle_radius=0.005, boundary_radius=None,
                        pointsets=["gt,GT", "pred,Ours"], font_size=36.0, num_frames=5, frames=None, pc="0xff0071c5",
                        bc="0xff9e9e9e", eye=None, target=None, up=[0.0, 1.0, 0.0], fov=35.0, ortho=None, bnd="far", ambient=0.3)
    # the shared flags keep draw_sim2d's defaults (its fixed --height default is the size used when none is given)
    shared = vars(D2._parser().parse_args(["in.hdf5", "out.png"]))
    for k in ("out_pattern", "width", "particle_radius", "boundary_radius", "pointsets", "font_size", "num_frames", "frames", "pc"):
        assert args[k] == shared[k], k
    assert D.frame_size() == (640, shared["height"]) and D.DEFAULT_HEIGHT == shared["height"]
    assert D.frame_size(height=1080) == (1920, 1080) and D.frame_size(width=1920) == (1920, 1080)
    assert D.frame_size(height=100, width=30) == (30, 100) and D.frame_size(height=90, aspect=1.0) == (90, 90)
    assert D.select_frames is D2.select_frames and D.draw_labels is D2.draw_labels and D._read_group is D2._read_group
    got = D._parser().parse_args(["a", "b", "--eye", "1", "2", "3", "--bnd", "near", "--ortho", "2", "--bc", "0x80ffffff"])
    assert got.eye == [1.0, 2.0, 3.0] and got.bnd == "near" and got.ortho == 2.0 and int(got.bc, 16) == 0x80ffffff
    with pytest.raises(SystemExit):
        D._parser().parse_args(["a", "b", "--bnd", "front"])


def test_default_camera_arithmetic():
    rng = np.random.default_rng(12)
    bnd = rng.uniform((-1, 0, 2), (3, 2.5, 4), size=(60, 3)).astype(np.float32)
    bnd[0], bnd[1] = (-1, 0, 2), (3, 2.5, 4)
    fluid = rng.uniform(-9, 9, size=(30, 3)).astype(np.float32)
    eye, target = D.default_pose(bnd, fluid)
    assert np.allclose(target, (1.0, 1.25, 3.0))
    diag = np.sqrt(4.0 ** 2 + 2.5 ** 2 + 2.0 ** 2)
    assert np.allclose(eye, target + 1.6 * diag * np.array([0.8, 0.5, 1.0]) / np.sqrt(0.64 + 0.25 + 1.0))
    # no boundary: the fluid's box
    eye2, target2 = D.default_pose(np.zeros((0, 3), np.float32), fluid)
    lo, hi = fluid.astype(np.float64).min(0), fluid.astype(np.float64).max(0)
    assert np.allclose(target2, 0.5 * (lo + hi))
    assert np.isclose(np.linalg.norm(eye2 - target2), 1.6 * np.linalg.norm(hi - lo))
    with pytest.raises(ValueError):
        D.default_pose(np.zeros((0, 3)), np.full((4, 3), np.nan))


def _results(rng, T=4, n=20, m=12, d=3, flat=False):
    pred = rng.uniform(-1, 1, size=(T, n, d)).astype(np.float32)
    gt = rng.uniform(-1, 1, size=(T, n, d)).astype(np.float32)
    bnd = rng.uniform(-2, 2, size=(m, d)).astype(np.float32)
    if flat:
        pred[..., 2], gt[..., 2], bnd[..., 2] = 0.25, 0.25, 0.25
    return [(pred, {"name": "pred", "type": "PARTICLE"}), (gt, {"name": "gt", "type": "PARTICLE"}),
            (bnd, {"name": "bnd", "type": "PARTICLE"})]


def test_a_2d_file_is_refused_with_a_pointer_to_draw_sim2d(tmp_path):
    rng = np.random.default_rng(13)
    out = str(tmp_path / "o.png")
    two = str(tmp_path / "two.hdf5")
    write_results(two, "SymNet", _results(rng, d=2))
    with pytest.raises(ValueError, match="draw_sim2d"):
        D.main([two, out, "--num_frames", "2"])
    flat = str(tmp_path / "flat.hdf5")
    write_results(flat, "SymNet", _results(rng, flat=True))
    with pytest.raises(ValueError, match="draw_sim2d"):
        D.main([flat, out, "--num_frames", "2"])
    ok = str(tmp_path / "ok.hdf5")
    write_results(ok, "SymNet", _results(rng))
    with pytest.raises(ValueError, match="no point set 'ours'"):
        D.main([ok, out, "--num_frames", "2", "--pointsets", "ours,Ours"])
    with pytest.raises(ValueError, match="outside"):
        D.main([ok, out, "--frames", "0", "4"])
    assert not os.path.exists(out) and D.main([]) == 1


# ----------------------------------------------------------------------------------------------------------------------
# the restatement's own sanity


def test_restatement_one_centred_sphere_is_mirror_symmetric():
    W, H = 21, 15
    # orthographic and perspective: the sphere's centre on the view axis, the principal point on the centre pixel's centre
    for ortho in (False, True):
        cam = S.Cam((1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0), 40.0, 10.5, 7.5, 1e-3, ortho)
        for farthest in (False, True):
            keys = S.depth_keys(cam, np.float32([[0, 0, 4.0]]), 0.5 if not ortho else 0.12, W, H, farthest=farthest)[0]
            assert np.array_equal(keys, keys[:, ::-1]) and np.array_equal(keys, keys[::-1, :])
            z, idx = S.decode(keys, farthest)
            covered = idx == 0
            assert covered[7, 10] and not covered[0, 0] and 1 < covered.sum() < W * H
            assert z[7, 10] == z[covered].min() and np.isinf(z[~covered]).all()  # the centre pixel is the nearest sample
            R = np.float32(40.0 / 4.0 * 0.5) if not ortho else np.float32(40.0 * 0.12)
            m = np.float32(10.0) if not ortho else np.float32(40.0)
            assert z[7, 10] == np.float32(4.0) - R / m  # d2 = 0 there: z = zc - R / m, nz = 1
            img, depth = S.shade(cam, [S.Layer(keys[None], np.float32([[0, 0, 4.0]]), 0.5 if not ortho else 0.12, 0xffff8000, farthest)],
                                 W, H, np.ones((1, H, W, 3), np.float32), ambient=0.3)
            assert np.array_equal(depth[0], z)
            assert np.allclose(img[0, 7, 10], (1.0, 128 / 255, 0.0), atol=1e-7)  # nz = 1: shade = 1, the colour itself
            assert np.array_equal(img[0][~covered], np.ones((int((~covered).sum()), 3), np.float32))
            assert np.array_equal(img[0], img[0][:, ::-1]) and np.array_equal(img[0], img[0][::-1])
            assert (img[0][covered] <= img[0, 7, 10] + 1e-7).all() and img[0][covered][:, 0].min() >= 0.3 - 1e-6


def test_restatement_depth_order_ties_and_min_px():
    cam = S.Cam((1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0), 20.0, 8.0, 8.0, 1e-3, False)
    pts = np.float32([[0.05, 0.0, 5.0], [0.05, 0.0, 3.0], [0.05, 0.0, 3.0], [30.0, 20.0, 200.0]])
    near = S.decode(S.depth_keys(cam, pts, 0.4, 16, 16)[0], False)
    far = S.decode(S.depth_keys(cam, pts, 0.4, 16, 16, farthest=True)[0], True)
    assert near[1][8, 8] == 1 and far[1][8, 8] == 0  # nearest: index 1 (the tie with 2 goes to the lower index); farthest: 0
    assert not (near[1] == 2).any() and not (far[1] == 2).any()
    # the far sphere is 0.04 px wide: min_px keeps it on one pixel at least
    assert (S.decode(S.depth_keys(cam, pts[3:], 0.4, 16, 16)[0], False)[1] == 0).sum() >= 1
    assert (S.decode(S.depth_keys(cam, pts[3:], 0.4, 16, 16, min_px=0.0)[0], False)[1] == 0).sum() == 0
    # splatting in two steps into one buffer equals one step (indices are per call, so compare the depths)
    both = S.depth_keys(cam, pts[:2], 0.4, 16, 16)
    step = S.depth_keys(cam, pts[1:2], 0.4, 16, 16, keys=S.depth_keys(cam, pts[:1], 0.4, 16, 16))
    assert np.array_equal(S.decode(both, False)[0], S.decode(step, False)[0])
    # behind the camera, not finite, radius 0: nothing
    empty = np.full((1, 16, 16), S.EMPTY)
    assert np.array_equal(S.depth_keys(cam, np.float32([[0, 0, -2.0], [np.nan, 0, 3], [0, np.inf, 3]]), 0.4, 16, 16), empty)
    assert np.array_equal(S.depth_keys(cam, pts, 0.0, 16, 16), empty)
