"""CPU checks of the renderer (dmcf_amd/utils/draw_sim2d.py, the reference's utils/draw_sim2d.py): the result-file reader, the
layout and frame arithmetic against the restatement tests/render_ref.py, the CLI's defaults and error cases, the labels, and
the host-side validation of the raster entry points (ABI 2.12).  The discs themselves are drawn on the GPU:
tests/test_gpu_render.py."""
import ctypes
import os
import struct

import numpy as np
import pytest
from PIL import Image, ImageFont

import render_ref as R
from dmcf_amd.datasets import write_results, write_results_npz
from dmcf_amd.utils import draw_sim2d as D
from dmcf_amd.utils.hdf5_reader import read_hdf5, read_results
from dmcf_amd.utils.hdf5_writer import write_hdf5

REFERENCE_DEFAULTS = dict(out_pattern=None, height=360, width=None, particle_radius=0.005, boundary_radius=None, margin=0.1,
                          pointsets=["gt,GT", "pred,Ours"], font_size=36.0, num_frames=5, frames=None, pc="0xff0071c5")


def _results(rng, T=7, n=50, m=20, empty_bnd=False):
    pred = rng.uniform(-1, 1, size=(T, n, 3)).astype(np.float32)
    gt = rng.uniform(-1, 1, size=(T + 2, n, 3)).astype(np.float32)
    bnd = np.zeros((0, 3), np.float32) if empty_bnd else rng.uniform(-2, 2, size=(m, 3)).astype(np.float32)
    return [(pred, {"name": "pred", "type": "PARTICLE"}), (gt, {"name": "gt", "type": "PARTICLE"}),
            (bnd, {"name": "bnd", "type": "PARTICLE"})]


# ----------------------------------------------------------------------------------------------------------------------
# reader


@pytest.mark.parametrize("empty_bnd", [False, True])
def test_reader_round_trips_write_results_and_the_npz_stand_in(tmp_path, empty_bnd):
    data = _results(np.random.default_rng(1), empty_bnd=empty_bnd)
    h5, npz = str(tmp_path / "r.hdf5"), str(tmp_path / "r.npz")
    write_results(h5, "SymNet", data)
    write_results_npz(npz, "SymNet", data)
    for path in (h5, npz):
        got = read_results(path)
        assert list(got) == ["SymNet"] and sorted(got["SymNet"]) == ["bnd", "gt", "pred"]
        for arr, props in data:
            a, attrs = got["SymNet"][props["name"]]
            assert a.dtype == arr.dtype and a.shape == arr.shape and np.array_equal(a, arr)
            assert attrs["type"] == "PARTICLE"
            assert np.array_equal(attrs["dim"], arr.shape) and attrs["dim"].dtype == np.int64


def test_reader_round_trips_other_dtypes_and_attributes(tmp_path):
    rng = np.random.default_rng(2)
    arrays = {"f64": rng.normal(size=(3, 4)), "i8": np.arange(-5, 5, dtype=np.int8), "u16": np.arange(9, dtype=np.uint16),
              "i32": rng.integers(-9, 9, size=(2, 2, 2)).astype(np.int32), "u64": np.arange(4, dtype=np.uint64),
              "empty": np.zeros((0,), np.float64), "i64": np.arange(6, dtype=np.int64).reshape(2, 3)}
    attrs = {"type": "DENSITY", "dim": np.asarray([1, 2, 3], np.int64), "w": np.float64(0.25), "v": np.arange(3, dtype=np.float32)}
    path = str(tmp_path / "t.h5")
    write_hdf5(path, "grp", [(k, v, attrs) for k, v in arrays.items()])
    got = read_hdf5(path)
    assert list(got) == ["grp"]
    for k, v in arrays.items():
        a, at = got["grp"][k]
        assert a.dtype == np.asarray(v).dtype and a.shape == np.shape(v) and np.array_equal(a, v), k
        assert at["type"] == "DENSITY" and np.array_equal(at["dim"], [1, 2, 3]) and at["w"] == 0.25
        assert at["v"].dtype == np.float32 and np.array_equal(at["v"], [0, 1, 2])


def _patched(tmp_path, data, find, replace, name):
    i = data.find(find)
    assert i >= 0, "pattern not in the file"
    bad = data[:i] + replace + data[i + len(replace):]
    path = str(tmp_path / name)
    with open(path, "wb") as f:
        f.write(bad)
    return path


def test_reader_refuses_unsupported_structures(tmp_path):
    arr = np.arange(12, dtype=np.float32).reshape(3, 4)
    path = str(tmp_path / "ok.h5")
    write_hdf5(path, "g", [("x", arr, {})])
    data = open(path, "rb").read()
    layout = struct.pack("<HHBBBB", 8, 24, 0, 0, 0, 0) + bytes([3, 1])
    f32 = bytes([0x11, 0x20, 31, 0]) + struct.pack("<I", 4)
    cases = {
        "superblock version": (data[:8], data[:8] + b"\x02", "superblock version 2"),
        "chunked": (layout, layout[:-1] + b"\x02", "chunked"),
        "vlen": (f32, bytes([0x19]) + f32[1:], "variable-length"),
        "big-endian": (f32, bytes([0x11, 0x21]) + f32[2:], "big-endian"),
        "filter": (layout, struct.pack("<H", 0x000B) + layout[2:], "filter pipeline"),
        "shared": (layout, layout[:4] + b"\x02" + layout[5:], "shared message"),
        "layout v2": (layout, layout[:-2] + b"\x02\x01", "layout message version 2"),
        "normalisation": (f32, bytes([0x11, 0x00]) + f32[2:], "normalisation 0"),
        "sign bit": (f32, bytes([0x11, 0x20, 30]) + f32[3:], "sign bit at 30"),
    }
    for name, (find, repl, msg) in cases.items():
        bad = _patched(tmp_path, data, find, repl, name + ".h5")
        with pytest.raises(ValueError, match=msg):
            read_hdf5(bad)
    # string attributes: space padding and an unknown character set are refused, not misread
    spath = str(tmp_path / "s.h5")
    write_hdf5(spath, "g", [("x", arr, {"type": "DENSITY"})])
    sdata = open(spath, "rb").read()
    s8 = bytes([0x13, 0x00, 0, 0]) + struct.pack("<I", 8)
    assert read_hdf5(spath)["g"]["x"][1]["type"] == "DENSITY"
    for name, repl, msg in (("space", bytes([0x13, 0x02]) + s8[2:], "padding type 2"),
                            ("charset", bytes([0x13, 0x20]) + s8[2:], "character set 2")):
        with pytest.raises(ValueError, match=msg):
            read_hdf5(_patched(tmp_path, sdata, s8, repl, name + ".h5"))
    trunc = str(tmp_path / "trunc.h5")
    open(trunc, "wb").write(data[:len(data) // 2])
    with pytest.raises(ValueError):
        read_hdf5(trunc)
    noth5 = str(tmp_path / "not.h5")
    open(noth5, "wb").write(b"\0" * 200)
    with pytest.raises(ValueError, match="not an HDF5 file"):
        read_hdf5(noth5)


# ----------------------------------------------------------------------------------------------------------------------
# layout, frames, CLI (main with the GPU drawing replaced by a recorder)


@pytest.mark.parametrize("box", [((-1.0, -0.5), (2.0, 1.5)), ((0.0, 0.0), (50.0, 50.0)), ((-3.0, -1.0), (-2.0, 4.0)), None])
@pytest.mark.parametrize("margin", [0.0, 0.1, 0.37])
@pytest.mark.parametrize("size", [dict(height=360), dict(height=1081), dict(width=640), dict(width=333)])
def test_canvas_layout_equals_the_restatement(box, margin, size):
    rng = np.random.default_rng(3)
    if box is None:
        bnd = np.zeros((0, 2), np.float32)
    else:
        bnd = rng.uniform(box[0], box[1], size=(40, 2)).astype(np.float32)
        bnd[0], bnd[1] = box[0], box[1]
    w, h, scale, shift = D.canvas_layout(bnd, margin, size.get("height", 360), size.get("width"))
    rw, rh, rscale, rshift, _, _ = R.layout(bnd, margin, size.get("height", 360), size.get("width"))
    assert (w, h) == (rw, rh) and scale == rscale and np.array_equal(shift, rshift)
    assert (size.get("height", h), size.get("width", w)) == (h, w)


def test_frame_selection():
    for T in (1, 5, 7, 50, 101):
        for k in (1, 2, 5, T):
            if k > T:
                continue
            ref = [x[0] for x in np.array_split(np.arange(T), k)]
            assert D.select_frames({"gt": T, "pred": T + 3}, k) == ref
    assert D.select_frames({"gt": 10, "pred": 12}, 3, frames=[9, 0, 4]) == [9, 0, 4]
    with pytest.raises(ValueError, match="larger than the shortest"):
        D.select_frames({"gt": 4, "pred": 9}, 5)
    with pytest.raises(ValueError, match="min"):
        D.select_frames({"pred": 9}, 5)


def test_cli_defaults_equal_the_reference():
    args = vars(D._parser().parse_args(["in.hdf5", "out.png"]))
    assert args.pop("path") == "in.hdf5" and args.pop("output") == "out.png"
    assert args == REFERENCE_DEFAULTS
    assert D.BOUNDARY_COLOR == 0xff000000


class _Recorder:
    def __init__(self):
        self.calls = []

    def __call__(self, bnd, particles, width, height, particle_color, boundary_color, particle_radius, boundary_radius, device=None):
        self.calls.append(dict(bnd=np.array(bnd), particles=np.array(particles), width=width, height=height, pc=particle_color,
                               bc=boundary_color, pr=particle_radius, br=boundary_radius))
        out = np.zeros((len(particles), height, width, 4), np.uint8)
        out[..., 0] = len(self.calls)  # row marker
        out[..., 1] = np.arange(len(particles))[:, None, None]  # frame marker
        out[..., 3] = 255
        return out


@pytest.mark.parametrize("size", [["--height", "200"], ["--width", "150"]])
def test_main_layout_positions_radii_and_output(tmp_path, monkeypatch, size):
    rng = np.random.default_rng(4)
    data = _results(rng, T=9, n=30, m=25)
    path = str(tmp_path / "res.hdf5")
    write_results(path, "SymNet", data)
    rec = _Recorder()
    monkeypatch.setattr(D, "draw_frames", rec)
    out = str(tmp_path / "all.png")
    pattern = str(tmp_path / "frames" / "{pointset}_{frame:04d}.png")
    assert D.main([path, out, "--pr", "0.02", "--br", "0.05", "--margin", "0.2", "--num_frames", "4", "--pc", "0xff112233",
                   "--out_pattern", pattern] + size) == 0
    pred, gt, bnd = (d[0] for d in data)
    mirror = lambda v: v[..., [0, 1]] * np.float32([1, -1])  # noqa: E731
    height, width = (int(size[1]), None) if size[0] == "--height" else (360, int(size[1]))
    W, H, scale, shift, pr, br = R.layout(mirror(bnd), 0.2, height, width, 0.02, 0.05)
    frames = [x[0] for x in np.array_split(np.arange(9), 4)]
    assert [c["width"] for c in rec.calls] == [W, W] and [c["height"] for c in rec.calls] == [H, H]
    for c, seq in zip(rec.calls, (gt, pred)):
        assert c["pc"] == 0xff112233 and c["bc"] == 0xff000000
        assert np.isclose(c["pr"], pr, rtol=1e-6) and np.isclose(c["br"], br, rtol=1e-6)
        np.testing.assert_allclose(c["bnd"], scale * (mirror(bnd) + shift), rtol=1e-6, atol=1e-4)
        np.testing.assert_allclose(c["particles"], scale * (mirror(seq[frames]) + shift), rtol=1e-6, atol=1e-4)
    im = np.asarray(Image.open(out))
    labels = D.draw_labels(["GT", "Ours"], H, 36.0)
    lw = labels[0].shape[1]
    assert im.shape == (2 * H, lw + 4 * W, 4)
    assert np.array_equal(im[:H, :lw], labels[0]) and np.array_equal(im[H:, :lw], labels[1])
    for row, ps in enumerate(("gt", "pred")):
        for j, f in enumerate(frames):
            tile = im[row * H:(row + 1) * H, lw + j * W:lw + (j + 1) * W]
            assert (tile[..., 0] == row + 1).all() and (tile[..., 1] == j).all()
            assert np.array_equal(np.asarray(Image.open(pattern.format(pointset=ps, frame=f))), tile)


def test_main_error_cases(tmp_path, monkeypatch):
    monkeypatch.setattr(D, "draw_frames", _Recorder())
    rng = np.random.default_rng(5)
    path = str(tmp_path / "res.hdf5")
    write_results(path, "SymNet", _results(rng, T=3))
    out = str(tmp_path / "o.png")
    with pytest.raises(ValueError, match="larger than the shortest"):
        D.main([path, out])  # 5 frames of 3
    with pytest.raises(ValueError, match="no point set 'ours'"):
        D.main([path, out, "--num_frames", "2", "--pointsets", "gt,GT", "ours,Ours"])
    with pytest.raises(ValueError, match="outside"):
        D.main([path, out, "--frames", "0", "3"])
    single = str(tmp_path / "single.hdf5")
    write_results(single, "Other", _results(rng, T=3)[:1] + _results(rng)[2:])
    with pytest.raises(ValueError, match="min"):
        D.main([single, out, "--num_frames", "2", "--pointsets", "pred,Ours"])
    assert D.main([single, out, "--frames", "1", "--pointsets", "pred,Ours"]) == 0  # the only group, --frames given
    assert D.main([]) == 1


def test_labels():
    for height in (37, 360):
        imgs = D.draw_labels(["GT", "Ours", "a much longer label"], height, 36)
        font = ImageFont.load_default(size=36)
        w = max(int(np.ceil(b[3] - b[1])) for b in map(font.getbbox, ["GT", "Ours", "a much longer label"]))
        assert all(im.shape == (height, w, 4) and im.dtype == np.uint8 for im in imgs)
        assert all((im[..., 3] == 255).all() and (im[..., 0] == im[..., 1]).all() for im in imgs)
        assert all(im[..., 0].min() < 64 and im[..., 0].max() == 255 for im in imgs)  # black text on white
        again = D.draw_labels(["GT", "Ours", "a much longer label"], height, 36)
        assert all(np.array_equal(a, b) for a, b in zip(imgs, again))
    # bottom to top: the horizontal rendering of "Ours" is the label rotated back, up to where it was placed
    im = D.draw_labels(["Ours"], 300, 36)[0][..., 0]
    ink = np.argwhere(im < 128)
    assert np.ptp(ink[:, 0]) > np.ptp(ink[:, 1])  # taller than wide
    wide = D.draw_labels(["Ours"], 300, 36, rot90=False)[0][..., 0]
    assert wide.shape[1] == int(np.ceil(font.getbbox("Ours")[2] - font.getbbox("Ours")[0]))


# ----------------------------------------------------------------------------------------------------------------------
# ABI (no device touched)


@pytest.fixture(scope="module")
def hip_lib():
    from dmcf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_raster_abi_host_validation(hip_lib):
    L = hip_lib
    assert L.dmcf_version() >= 21200
    ws = ctypes.create_string_buffer(1 << 16)
    wsb = L.dmcf_raster_workspace_bytes(100, 3, 100, 64, 48)
    assert 0 < wsb <= len(ws)
    assert L.dmcf_raster_workspace_bytes(-1, 3, 100, 64, 48) == 0
    assert L.dmcf_raster_workspace_bytes(100, 3, 50, 64, 48) == 0  # overlapping frames
    assert L.dmcf_raster_workspace_bytes(100, 1, 0, 0, 48) == 0
    total = ctypes.c_int64()
    xy = ctypes.create_string_buffer(16)
    x8 = ctypes.addressof(xy) + (-ctypes.addressof(xy) % 8)
    count = lambda *a: L.dmcf_raster_count(*a)  # noqa: E731
    assert count(None, 100, 3, 100, 1.0, 64, 48, ws, wsb, ctypes.byref(total), None) == -1  # no points
    assert count(x8, -1, 3, 100, 1.0, 64, 48, ws, wsb, ctypes.byref(total), None) == -1
    assert count(x8, 100, -3, 100, 1.0, 64, 48, ws, wsb, ctypes.byref(total), None) == -1
    assert count(x8, 100, 3, -1, 1.0, 64, 48, ws, wsb, ctypes.byref(total), None) == -1
    assert count(x8, 100, 3, 100, 1.0, -64, 48, ws, wsb, ctypes.byref(total), None) == -1
    assert count(x8, 100, 3, 100, 1.0, 64, 48, None, wsb, ctypes.byref(total), None) == -1
    assert count(x8, 100, 3, 100, 1.0, 64, 48, ws, wsb, None, None) == -1
    assert count(x8 + 4, 100, 3, 100, 1.0, 64, 48, ws, wsb, ctypes.byref(total), None) == -1  # misaligned float2
    assert count(x8, 100, 3, 100, 1.0, 64, 48, ws, wsb - 1, ctypes.byref(total), None) == -2
    img, bins = ctypes.create_string_buffer(64), ctypes.create_string_buffer(64)
    disc = lambda *a: L.dmcf_raster_discs(*a)  # noqa: E731
    assert disc(x8, 100, 3, 100, 1.0, 0xff000000, 64, 48, None, ws, wsb, bins, 4, None) == -1  # no image
    assert disc(None, 100, 3, 100, 1.0, 0xff000000, 64, 48, img, ws, wsb, bins, 4, None) == -1
    assert disc(x8, 100, 3, 100, 1.0, 0xff000000, 64, 48, img, ws, wsb, None, 4, None) == -1  # no bins
    assert disc(x8, 100, 3, 100, 1.0, 0xff000000, 64, 48, img, ws, wsb, bins, -4, None) == -1
    assert disc(x8, -100, 3, 100, 1.0, 0xff000000, 64, 48, img, ws, wsb, bins, 4, None) == -1
    assert disc(x8, 100, 3, 100, 1.0, 0xff000000, 64, 0, img, ws, wsb, bins, 4, None) == -1
    assert disc(x8, 100, 3, 100, 1.0, 0xff000000, 64, 48, img, None, wsb, bins, 4, None) == -1
    # valid calls that draw nothing return before any device work
    assert disc(x8, 100, 3, 100, 0.0, 0xff000000, 64, 48, img, ws, wsb, bins, 4, None) == 0  # r = 0
    assert disc(x8, 100, 3, 100, float("nan"), 0xff000000, 64, 48, img, ws, wsb, bins, 4, None) == 0
    assert disc(x8, 100, 3, 100, 1.0, 0x00ffffff, 64, 48, img, ws, wsb, bins, 4, None) == 0  # alpha 0


def test_raster_op_refuses_cpu_tensors(hip_lib):
    import torch

    from dmcf_amd import _lib, ops
    with pytest.raises(_lib.DmcfError):
        ops.raster_discs(torch.zeros(3, 2), 1.0, 0xff000000, 8, 8)
    with pytest.raises(ValueError):
        ops.raster_discs(torch.zeros(3, 3), 1.0, 0xff000000, 8, 8)
    q = ops.rgba8(torch.tensor([[0.0, 0.5, 0.25], [0.75, 1.0, 1.2]]))
    assert q.tolist() == [[0, 128, 64, 255], [191, 255, 255, 255]]  # round(255 C), clamped, alpha 255
