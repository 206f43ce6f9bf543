"""Shared by the column-generator tests: the cases of tests/golden/column_gen.npz (written by
tests/golden/make_column_gen_fixture.py from the reference's generator) and the error bar they are held to.

The bar, per scene and for positions and velocities separately, over all frames:

    |ours - reference| <= 4 * sens + 4 * ulp32(largest |value| of the reference's array)

``sens`` is the reference's OWN sensitivity: the largest change of that array when every fluid particle's initial position is
moved by one float32 ulp.  A solver that sums over j in another order than numpy differs from the reference only where a
float64 sum crosses a float32 rounding boundary or the ``err < eps`` threshold -- the way such a nudge does; 4 is the margin
over one nudge, and the ulp term covers the scenes where the nudge happens to change nothing."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DATASET = dict(res=100, gravity=-10.0, dt=0.0025)  # the dataset keys of configs/column/hrnet.yml
CASES = {  # name -> (seed, generator section); the same table as in make_column_gen_fixture.py
    "a": (44, dict(offset=10.0, pts_cnt=[1, 5], data_cnt=2, timesteps=100)),
    "b": (44, dict(pts_cnt=[20], data_cnt=1, timesteps=12)),
    "c": (7, dict(rnd=0.05, min_pts=3, max_pts=8, data_cnt=2, timesteps=20)),
    "d": (44, dict(pts_cnt=[40], data_cnt=1, timesteps=4)),
}
_fixture = None


def fixture():
    global _fixture
    if _fixture is None:
        with np.load(os.path.join(GOLDEN, "column_gen.npz")) as z:
            _fixture = {k: z[k] for k in z.files}
    return _fixture


def bound(ref, sens):
    return 4.0 * float(sens) + 4.0 * float(np.spacing(np.float32(np.abs(ref).max())))


def check_scene(name, s, pos, vel, frames=None, report=print):
    """Hold one generated scene's frame arrays ``pos`` / ``vel`` [T, n, 3] to the bar of scene ``s`` of case ``name`` (the first
    ``frames`` frames of it); prints every figure before it asserts."""
    fx, k = fixture(), f"{name}_s{s}_"
    for key, got in (("pos", pos), ("vel", vel)):
        ref = fx[k + key][:frames]
        got = np.asarray(got)
        assert got.shape == ref.shape and got.dtype == np.float32, (key, got.shape, got.dtype, ref.shape)
        dev = float(np.abs(got.astype(np.float64) - ref.astype(np.float64)).max())
        bar = bound(ref, fx[k + "sens_" + key])
        report(f"case {name} scene {s} {key}: deviation {dev:.4g}  bar {bar:.4g}  (sens {float(fx[k + 'sens_' + key]):.4g})")
        assert dev <= bar, f"case {name} scene {s} {key}: deviation {dev:.4g} exceeds the bar {bar:.4g}"
