"""The disc rasterizer on the GPU (dmcf_amd/csrc/raster.hip, ops.raster_discs) against the float64 restatement
tests/render_ref.py: transmittance, 8-bit output, edge cases, batching, the shared-boundary stride 0 and bitwise
repeatability; then the renderer (dmcf_amd/utils/draw_sim2d.py) end to end on a run_test result file, and one 1M-disc frame."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import render_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
BLUE = 0xff0071c5  # the reference's particle colour: red channel 0, so out[..., 0] is T over a white image
HALF = 0x800071c5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but torch.cuda.is_available() is False")
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def _draw(xy, radius, color, W, H, dev, out=None):
    from dmcf_amd import ops
    o = None if out is None else _t(out, dev)
    return ops.raster_discs(_t(xy, dev), radius, color, W, H, out=o).cpu().numpy()


def _check(got, xy, radius, color, W, H, base=None):
    """T within 1e-5 where <= 64 discs cover a pixel; 8-bit output within one level everywhere, equal away from rounding
    boundaries."""
    from dmcf_amd import ops
    xy32 = np.asarray(xy, dtype=np.float32).astype(np.float64)  # (the op sees float32 centres)
    ref, T, k = R.raster(xy32, radius, color, W, H, image=base)
    assert got.shape == ref.shape
    if base is None and (color >> 16) & 255 == 0:
        m = k <= 64
        err = np.abs(got[..., 0].astype(np.float64) - T)[m]
        assert err.size == 0 or err.max() <= 1e-5, err.max()
    else:
        assert np.abs(got - ref).max() <= 2e-5
    q = ops.rgba8(torch.from_numpy(got)).numpy().astype(np.int64)
    qr = R.rgba8(ref).astype(np.int64)
    assert np.abs(q - qr).max() <= 1
    v = ref * 255.0
    away = np.abs(v - np.floor(v) - 0.5) > 1e-4
    assert np.array_equal(q[..., :3][away], qr[..., :3][away])


@pytest.mark.parametrize("W,H,F,radius,color", [(100, 70, 3, 0.3, BLUE), (100, 70, 2, 1.7, HALF), (64, 64, 1, 4.5, BLUE),
                                                (37, 21, 2, 2.2, HALF), (256, 48, 1, 0.75, 0xc0ff8000)])
def test_raster_matches_restatement(dev, W, H, F, radius, color):
    rng = np.random.default_rng(W * 1000 + H)
    n = 600
    xy = rng.uniform([-6, -6], [W + 6, H + 6], size=(F, n // 2, 2))
    clump = rng.normal([W / 2, H / 2], 1.5, size=(F, n // 2, 2))  # a dense spot: pixels under more than 64 discs
    xy = np.concatenate([xy, clump], axis=1)
    _check(_draw(xy, radius, color, W, H, dev), xy, radius, color, W, H)


def test_composites_over_an_existing_image(dev):
    rng = np.random.default_rng(7)
    W, H = 50, 40
    base = rng.uniform(0, 1, size=(2, H, W, 3))
    xy = rng.uniform(-3, 53, size=(2, 200, 2))
    _check(_draw(xy, 1.3, HALF, W, H, dev, out=base), xy, 1.3, HALF, W, H, base=base)


def test_edge_cases(dev):
    rng = np.random.default_rng(8)
    W, H = 37, 21
    base = np.ones((1, H, W, 3), np.float32)
    # N = 0: the image comes back unchanged
    assert np.array_equal(_draw(np.zeros((1, 0, 2)), 2.0, BLUE, W, H, dev, out=base), base)
    # off the canvas, partly off it, at negative coordinates
    xy = np.float32([[[-50, -50], [-1.2, 5], [5, -0.8], [W + 0.7, 10], [10, H + 1.1], [1e30, 3], [-1e30, -1e30], [W * 3, H * 3]]])
    _check(_draw(xy, 1.5, BLUE, W, H, dev), xy, 1.5, BLUE, W, H)
    # NaN and infinite centres contribute nothing: the same bits as without them
    good = rng.uniform(0, 30, size=(1, 50, 2))
    bad = np.concatenate([good, np.float32([[[np.nan, 3], [4, np.nan], [np.inf, 2], [np.nan, np.nan]]])], axis=1)
    assert np.array_equal(_draw(bad, 2.0, HALF, W, H, dev), _draw(good, 2.0, HALF, W, H, dev))
    # r = 0 draws nothing; r below half a pixel; r larger than the image
    assert np.array_equal(_draw(good, 0.0, BLUE, W, H, dev, out=base), base)
    for r in (0.1, 0.45, 80.0):
        _check(_draw(good[:, :5], r, BLUE, W, H, dev), good[:, :5], r, BLUE, W, H)
    # a 1 x 1 image
    one = np.float32([[[0.5, 0.5], [0.9, 0.2], [3, 3]]])
    _check(_draw(one, 0.6, HALF, 1, 1, dev), one, 0.6, HALF, 1, 1)
    # 10^5 coincident discs in one tile
    many = np.broadcast_to(np.float32([20.3, 9.6]), (1, 100000, 2))
    # (identical discs add identical float32 rounding errors of the coverage: T within 1e-4 here)
    got = _draw(many, 1.2, 0x080071c5, W, H, dev)
    T1, _ = R.transmittance(many[0, :1], 1.2, 8, 0, W, 0, H)
    T = T1 ** 100000
    assert np.abs(got[0, ..., 0] - T).max() <= 1e-4
    assert np.abs(got[0, ..., 0] * 255 - T * 255).max() <= 1.0


def test_batching_stride_zero_and_repeatability(dev):
    from dmcf_amd import ops
    rng = np.random.default_rng(9)
    W, H, F = 83, 61, 4
    xy = rng.uniform(-2, 85, size=(F, 3000, 2))
    batch = _draw(xy, 1.1, HALF, W, H, dev)
    singles = np.concatenate([_draw(xy[f:f + 1], 1.1, HALF, W, H, dev) for f in range(F)])
    assert np.array_equal(batch, singles)
    assert np.array_equal(batch, _draw(xy, 1.1, HALF, W, H, dev))
    # stride 0 ([N, 2] into F frames) == the points replicated into every frame
    base = rng.uniform(0, 1, size=(F, H, W, 3)).astype(np.float32)
    shared = ops.raster_discs(_t(xy[0], dev), 0.9, 0xff000000, W, H, out=_t(base, dev)).cpu().numpy()
    rep = _draw(np.broadcast_to(xy[0], xy.shape), 0.9, 0xff000000, W, H, dev, out=base)
    assert np.array_equal(shared, rep)


def test_draw_frame_is_the_restatement(dev):
    from dmcf_amd.utils import draw_sim2d as D
    rng = np.random.default_rng(10)
    W, H = 120, 90
    p, b = rng.uniform(0, 120, size=(400, 2)), rng.uniform(0, 120, size=(100, 2))
    im = D.draw_frame(b, p, W, H, 0xff0071c5, 0xff000000, 1.4, 2.1)
    ref, _, _ = R.raster(p, 1.4, 0xff0071c5, W, H)
    ref, _, _ = R.raster(b, 2.1, 0xff000000, W, H, image=ref)
    assert im.shape == (H, W, 4) and im.dtype == np.uint8 and (im[..., 3] == 255).all()
    assert np.abs(im.astype(int) - R.rgba8(ref[0]).astype(int)).max() <= 1


def test_end_to_end_run_test_then_render(dev, tmp_path):
    """run_test on the canyon frames (as tests/test_gpu_model.py runs it) writes an HDF5 file; main renders it."""
    import yaml
    from PIL import Image

    from dmcf_amd import run_pipeline
    from dmcf_amd.utils import draw_sim2d as D
    from dmcf_amd.utils import tf_checkpoint as tc
    from dmcf_amd.utils.hdf5_reader import read_results
    from tools import configs
    w = dict(np.load(os.path.join(GOLDEN, "liquid3d_weights.npz")))
    cfg = dict(dataset=dict(name="CConvData3D"),
               model=dict(configs.LIQUID3D, ckpt_path=None),
               pipeline=dict(name="Simulator", version="v0", main_log_dir=str(tmp_path / "logs"), output_dir=str(tmp_path / "out"),
                             data_generator=dict(scale=[1.0, 1.0, 1.0], train=dict(stride=1), valid=dict(stride=1),
                                                 test=dict(stride=1, time_start=0, time_end=50))))
    yml = tmp_path / "liquid3d.yml"
    yml.write_text(yaml.safe_dump(cfg))
    args, extra = run_pipeline.parse_args(["-c", str(yml), "--split", "test", "--dataset_path", GOLDEN])
    pipe = run_pipeline.build(args, extra)
    tc.load_into_model(pipe.model, w, device=dev)
    path = pipe.run_test(epoch=1)[0]
    data = {k: v[0] for k, v in read_results(path)["SymNet"].items()}
    T = data["pred"].shape[0]
    out, pattern = str(tmp_path / "r.png"), str(tmp_path / "tiles" / "{pointset}_{frame:04d}.png")
    assert D.main([path, out, "--num_frames", str(T), "--out_pattern", pattern, "--pr", "0.03"]) == 0
    im = np.asarray(Image.open(out))
    mirror = lambda v: v[..., [0, 1]] * np.float32([1, -1])  # noqa: E731
    W, H, scale, shift, pr, br = R.layout(mirror(data["bnd"]), 0.1, 360, None, 0.03)
    lw = D.draw_labels(["GT", "Ours"], H, 36.0)[0].shape[1]
    assert im.shape == (2 * H, lw + T * W, 4)
    bnd_px = scale * (mirror(data["bnd"]) + shift)
    for row, ps in enumerate(("gt", "pred")):
        for f in range(T):
            tile = im[row * H:(row + 1) * H, lw + f * W:lw + (f + 1) * W]
            ref = D.draw_frame(bnd_px, scale * (mirror(data[ps][f]) + shift), W, H, 0xff0071c5, 0xff000000, pr, br)
            assert np.array_equal(tile, ref)
            assert np.array_equal(np.asarray(Image.open(pattern.format(pointset=ps, frame=f))), tile)
            assert (tile[..., :3] < 255).any()  # something was drawn
    # the --width path
    out2 = str(tmp_path / "w.png")
    assert D.main([path, out2, "--frames", "0", "2", "--width", "200"]) == 0
    W2, H2, _, _, _, _ = R.layout(mirror(data["bnd"]), 0.1, 360, 200)
    lw2 = D.draw_labels(["GT", "Ours"], H2, 36.0)[0].shape[1]
    assert np.asarray(Image.open(out2)).shape == (2 * H2, lw2 + 2 * 200, 4) and W2 == 200


def test_one_million_discs(dev):
    """The bench scene (tools/scenes.box_scene(1000, dim=2) with its shell, ~1M points) at 1080 pixels: sampled tiles against
    the restatement."""
    from dmcf_amd import ops
    from dmcf_amd.utils import draw_sim2d as D
    from tools.scenes import box_scene
    sc = box_scene(1000, dim=2)
    bnd = sc["box"][:, :2] * np.float32([1, -1])
    pos = sc["pos"][:, :2] * np.float32([1, -1])
    W, H, scale, shift = D.canvas_layout(bnd, 0.1, 1080)
    r = 0.025 * scale
    px = (scale * (np.concatenate([pos, bnd]) + shift)).astype(np.float32)
    assert px.shape[0] > 1_000_000
    got = ops.raster_discs(_t(px, dev), r, BLUE, W, H).cpu().numpy()[0]
    rng = np.random.default_rng(11)
    for _ in range(12):
        x0, y0 = int(rng.integers(0, W - 16)), int(rng.integers(0, H - 16))
        T, k = R.transmittance(px, r, 255, x0, x0 + 16, y0, y0 + 16)
        m = k <= 64
        assert m.any(), f"tile at ({x0}, {y0}): every pixel is under more than 64 discs, nothing to compare"
        assert np.abs(got[y0:y0 + 16, x0:x0 + 16, 0] - T)[m].max() <= 1e-5
