"""CPU checks of the validation metrics (ABI 2.9, dmcf_amd/csrc/metrics.hip): symbols, ctypes mirror, host-side validation and
workspace queries of dmcf_nn_distance / dmcf_approx_match / dmcf_match_cost / dmcf_emd (no device is touched); the float64
restatement tests/metrics_ref.py against the algorithm's invariants; compare_dist against a per-point loop; get_rollout's
random_start; run_pipeline's --split valid."""
import ctypes
import os
import re

import numpy as np
import pytest

import metrics_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["dmcf_nn_distance_workspace_bytes", "dmcf_nn_distance", "dmcf_approx_match_workspace_bytes", "dmcf_approx_match",
       "dmcf_match_cost_workspace_bytes", "dmcf_match_cost", "dmcf_emd_workspace_bytes", "dmcf_emd"]
EINVAL, EWORKSPACE = -1, -2
FAKE = 1 << 20  # a non-NULL device address: validation returns before anything could dereference it


@pytest.fixture(scope="module")
def hip_lib():
    from dmcf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_version(hip_lib):
    assert hip_lib.dmcf_version() >= 20900


def test_symbols_declared_mirrored_exported(hip_lib):
    from dmcf_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dmcf_hip.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", text), f"{name} not declared in dmcf_hip.h"
        assert name in _lib.SYMBOLS
        fn = getattr(hip_lib, name)
        assert fn.argtypes is not None and fn.restype is not None, f"{name} has no ctypes prototype"


def _counts(vals):
    return (ctypes.c_int32 * len(vals))(*vals)


def test_nn_distance_host_validation(hip_lib):
    L = hip_lib
    ws = L.dmcf_nn_distance_workspace_bytes(2, 100, 50)
    assert ws > 0
    f = lambda *a: L.dmcf_nn_distance(*a)  # noqa: E731
    ok = (FAKE, FAKE, 2, 100, 50, FAKE, FAKE, FAKE, FAKE, FAKE, ws, None)
    bad = [
        (None, FAKE) + ok[2:],                                   # null xyz1
        (FAKE, None) + ok[2:],                                   # null xyz2
        ok[:9] + (None,) + ok[10:],                              # null workspace
        ok[:2] + (-1,) + ok[3:],                                 # negative b
        ok[:3] + (-5,) + ok[4:],                                 # negative n
        ok[:4] + (-5,) + ok[5:],                                 # negative m
        ok[:5] + (None, None, None, None) + ok[9:],              # no direction requested
        ok[:5] + (FAKE, None) + ok[7:],                          # dist1 without idx1
        ok[:3] + (0,) + ok[4:],                                  # empty xyz1 with b > 0
    ]
    for args in bad:
        assert f(*args) == EINVAL, args
    assert f(*(ok[:10] + (ws - 1,) + ok[11:])) == EWORKSPACE
    assert f(*(ok[:2] + (0,) + ok[3:])) == 0  # b == 0: nothing to do
    # workspace grows with the sizes
    assert L.dmcf_nn_distance_workspace_bytes(1, 10 ** 5, 10 ** 5) > L.dmcf_nn_distance_workspace_bytes(1, 10 ** 4, 10 ** 4) > \
        L.dmcf_nn_distance_workspace_bytes(1, 1000, 1000) > 0
    assert L.dmcf_nn_distance_workspace_bytes(-1, 10, 10) == 0


@pytest.mark.parametrize("entry", ["dmcf_approx_match", "dmcf_emd"])
def test_approx_match_host_validation(hip_lib, entry):
    L = hip_lib
    f = getattr(L, entry)
    q = getattr(L, entry + "_workspace_bytes")
    b, n, m = 2, 100, 50
    ws = q(b, n, m)
    assert ws >= 4 * (3 * n + 2 * m)
    ok = (FAKE, FAKE, b, n, m, None, None, FAKE, FAKE, ws, None)
    assert f(*(None,) + ok[1:]) == EINVAL
    assert f(*ok[:1] + (None,) + ok[2:]) == EINVAL
    assert f(*ok[:7] + (None,) + ok[8:]) == EINVAL       # no output
    assert f(*ok[:8] + (None,) + ok[9:]) == EINVAL       # no workspace
    assert f(*ok[:2] + (-1,) + ok[3:]) == EINVAL
    assert f(*ok[:3] + (-1,) + ok[4:]) == EINVAL
    assert f(*ok[:4] + (-1,) + ok[5:]) == EINVAL
    assert f(*ok[:5] + (_counts([100, 101]), None) + ok[7:]) == EINVAL   # count above n
    assert f(*ok[:5] + (None, _counts([50, 51])) + ok[7:]) == EINVAL     # count above m
    assert f(*ok[:5] + (_counts([-1, 3]), None) + ok[7:]) == EINVAL      # negative count
    assert f(*ok[:9] + (ws - 1,) + ok[10:]) == EWORKSPACE
    assert f(*ok[:2] + (0,) + ok[3:]) == 0
    assert q(1, 10 ** 5, 10 ** 5) > q(1, 10 ** 4, 10 ** 4) > q(1, 1000, 1000) > 0
    # O(n + m): far below the 4 n m bytes of a dense match
    assert q(1, 10 ** 5, 10 ** 5) < 4 * 10 ** 10 / 100


def test_match_cost_host_validation(hip_lib):
    L = hip_lib
    ws = L.dmcf_match_cost_workspace_bytes(2, 100, 50)
    assert ws > 0
    ok = (FAKE, FAKE, 2, 100, 50, FAKE, FAKE, FAKE, ws, None)
    assert L.dmcf_match_cost(*(None,) + ok[1:]) == EINVAL
    assert L.dmcf_match_cost(*ok[:5] + (None,) + ok[6:]) == EINVAL   # no match
    assert L.dmcf_match_cost(*ok[:6] + (None,) + ok[7:]) == EINVAL   # no cost
    assert L.dmcf_match_cost(*ok[:7] + (None,) + ok[8:]) == EINVAL   # no workspace
    assert L.dmcf_match_cost(*ok[:3] + (-1,) + ok[4:]) == EINVAL
    assert L.dmcf_match_cost(*ok[:8] + (ws - 1,) + ok[9:]) == EWORKSPACE
    assert L.dmcf_match_cost_workspace_bytes(1, 10 ** 5, 10 ** 5) > L.dmcf_match_cost_workspace_bytes(1, 1000, 1000)


def test_ops_refuse_cpu_tensors():
    torch = pytest.importorskip("torch")
    from dmcf_amd import _lib, ops
    a = torch.zeros((1, 5, 3))
    for fn in (lambda: ops.nn_distance(a, a), lambda: ops.approx_match(a, a), lambda: ops.emd(a, a),
               lambda: ops.match_cost(a, a, torch.zeros((1, 5, 5)))):
        with pytest.raises(_lib.DmcfError):
            fn()


# ----------------------------------------------------------------------------------------------------------------------
# the float64 restatement
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", [(1999, 1000), (1000, 1999), (7, 3), (3, 7), (64, 64), (1, 5)])
def test_restatement_invariants(n, m):
    rng = np.random.default_rng(n * 7 + m)
    a = rng.uniform(0, 1, (1, n, 3))
    b = rng.uniform(0, 1, (1, m, 3))
    ml, mr = R.multipliers(n, m)
    assert (ml, mr) == ((1, n // m) if n >= m else (m // n, 1))
    match = R.approx_match(a, b)[0]  # [m, n]
    assert match.shape == (m, n)
    assert (match >= 0).all()
    assert (match.sum(0) <= ml + 1e-9).all()   # column k: what xyz1[k] gave away
    assert (match.sum(1) <= mr + 1e-9).all()   # row l: what xyz2[l] took
    # the smaller side is (nearly) used up: the assignment is a transport plan, not an arbitrary weighting
    total = match.sum()
    assert total <= min(n * ml, m * mr) + 1e-6 and total > 0.5 * min(n * ml, m * mr)
    cost = R.match_cost(a, b, match[None])[0]
    assert cost > 0


def test_restatement_integer_division_and_counts():
    rng = np.random.default_rng(3)
    a = rng.uniform(0, 1, (2, 9, 3))
    b = rng.uniform(0, 1, (2, 4, 3))
    # (7, 3): multiR = 7 // 3 = 2, not 7 / 3
    match = R.approx_match(a, b, n=[7, 9], m=[3, 4])
    assert (match[0, 3:] == 0).all() and (match[0, :, 7:] == 0).all()
    assert match[0].sum(1).max() > 1.5 and (match[0].sum(1) <= 2 + 1e-9).all()
    np.testing.assert_array_equal(match[0, :3, :7], R.approx_match_one(a[0, :7], b[0, :3]))
    # 2-D points are z = 0
    np.testing.assert_array_equal(R.approx_match(a[:, :, :2], b[:, :, :2]),
                                  R.approx_match(np.concatenate([a[:, :, :2], np.zeros((2, 9, 1))], -1),
                                                 np.concatenate([b[:, :, :2], np.zeros((2, 4, 1))], -1)))


def test_restatement_identical_sets():
    """Matching a set with itself: a diagonal plan and zero cost at the sharp levels."""
    rng = np.random.default_rng(5)
    a = rng.uniform(0, 1, (1, 50, 3))
    match = R.approx_match(a, a)[0]
    assert np.allclose(np.diag(match), 1.0, atol=1e-6)
    assert R.match_cost(a, a, match[None])[0] < 1e-6


# ----------------------------------------------------------------------------------------------------------------------
# host helpers of run_valid
# ----------------------------------------------------------------------------------------------------------------------
def _compare_dist_loop(x, y, bin_size=25):
    """Per-point histogram KL, one point at a time (the reference's formulation)."""
    from scipy.stats import entropy
    dim = x.shape[-1]
    per = int((x.shape[0] // bin_size) ** (1 / dim))
    lo = np.percentile(np.concatenate((x, y), axis=0), 5, axis=0)
    hi = np.percentile(np.concatenate((x, y), axis=0), 95, axis=0)
    w = (hi - lo + 1e-6) / per
    hx = np.zeros((per + 1,) * dim) + 1e-5
    hy = np.zeros((per + 1,) * dim) + 1e-5
    for pts, h in ((x, hx), (y, hy)):
        for p in pts:
            cell = tuple(np.clip(((np.array(p) - lo) / w).astype("int32"), 0, per))
            h[cell] += 1
    return entropy(hx.reshape(-1), hy.reshape(-1))


@pytest.mark.parametrize("shape,dtype", [((2000, 3), np.float32), ((1280, 3), np.float32), ((700, 2), np.float64), ((30, 3), np.float32)])
def test_compare_dist_matches_loop(shape, dtype):
    pytest.importorskip("scipy")
    from dmcf_amd.utils.evaluation_helper import compare_dist
    rng = np.random.default_rng(shape[0])
    x = rng.normal(size=shape).astype(dtype)
    y = (rng.normal(size=shape) * 1.3 + 0.2).astype(dtype)
    for a, b in ((x, y), (y, x), (x, x)):
        got, want = compare_dist(a, b), _compare_dist_loop(a, b)
        assert abs(got - want) <= 1e-12 * max(1.0, abs(want)), (got, want)


def test_distance_and_merge_dicts():
    from dmcf_amd.utils.evaluation_helper import distance, merge_dicts
    x = np.float32([[0, 0, 0], [1, 1, 1]])
    y = np.float32([[3, 4, 0], [1, 1, 1]])
    np.testing.assert_allclose(distance(x, y), [5.0, 0.0])
    d = merge_dicts([{"a": 1.0, "b": 2.0}, {"a": 3.0}], lambda s, v: s + v / 2)
    assert d == {"a": 2.0, "b": 1.0}


def _scenes(n_scenes=3, frames=40):
    out = []
    for s in range(n_scenes):
        fr = []
        for f in range(frames):
            fr.append(dict(pos=np.full((4, 3), 100 * s + f, np.float32), vel=np.zeros((4, 3), np.float32), frame_id=f,
                           scene_id="s%d" % s, box=np.zeros((2, 3), np.float32), box_normals=np.zeros((2, 3), np.float32)))
        out.append(fr)
    return out


def test_get_rollout_random_start():
    from dmcf_amd.datasets import get_rollout
    from dmcf_amd.datasets.dataset_reader_physics import Dataset
    ds = Dataset(data=_scenes())
    np.random.seed(7)
    base = get_rollout(ds, stride=2, time_start=1, time_end=6)
    state = np.random.get_state()[1].copy()
    # random_start = 1 draws nothing and keeps the plain window
    np.random.seed(7)
    again = get_rollout(ds, stride=2, time_start=1, time_end=6, random_start=1)
    assert np.array_equal(np.random.get_state()[1], state)
    for a, b in zip(base, again):
        assert a.keys() == b.keys()
        for k in a:
            np.testing.assert_array_equal(a[k], b[k])
    assert [list(r["frame_id"]) for r in base] == [[2, 4, 6, 8, 10]] * 3
    # random_start > 1: one draw per scene, randint(random_start * stride), shifting both ends of the window
    np.random.seed(42)
    got = get_rollout(ds, stride=2, time_start=1, time_end=6, random_start=5)
    np.random.seed(42)
    offs = [np.random.randint(5 * 2) for _ in range(3)]
    assert len(got) == 3
    for s, (r, off) in enumerate(zip(got, offs)):
        want = [f for f in range(40) if f >= 2 + off and f % 2 == 0 and f < 12 + off]
        assert list(r["frame_id"]) == want
        np.testing.assert_array_equal(r["pos"][:, 0, 0], [100 * s + f for f in want])
    assert len(set(offs)) > 1  # (the seed gives the scenes different windows)


def test_run_pipeline_accepts_valid_split():
    from dmcf_amd import run_pipeline
    args, extra = run_pipeline.parse_args(["-c", "x.yml", "--split", "valid", "--pipeline.version", "v1"])
    assert args.split == "valid" and extra == {"pipeline.version": "v1"}
    from dmcf_amd.datasets import DatasetGroup
    g = DatasetGroup(name="x", dataset_path=os.path.join(ROOT, "tests", "golden"), split="valid")
    assert len(g.valid) == 1 and g.test is None


def test_emd_loss_is_validation_only():
    from dmcf_amd.utils.tools import losses
    assert callable(losses.emd_loss)
    for typ in ("chamfer", "emd", "hist", "dense"):
        with pytest.raises(NotImplementedError):
            losses.get_loss(typ)(None, None)
