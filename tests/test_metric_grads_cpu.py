"""CPU checks of the point-cloud op gradients (ABI 2.13, dmcf_amd/csrc/metrics_bwd.hip): the float64 restatement
tests/metric_grads_ref.py against central finite differences and the gradients' identities; the C ABI's symbols, version,
workspace queries and host-side validation (no device is touched); the reference-path mirror modules."""
import ctypes
import os
import re

import numpy as np
import pytest

import metric_grads_ref as G
import metrics_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["dmcf_nn_distance_backward_workspace_bytes", "dmcf_nn_distance_backward", "dmcf_match_cost_backward_workspace_bytes",
       "dmcf_match_cost_backward", "dmcf_emd_with_levels", "dmcf_emd_backward_workspace_bytes", "dmcf_emd_backward",
       "dmcf_gather_point_backward_workspace_bytes", "dmcf_gather_point_backward"]
EINVAL, EWORKSPACE = -1, -2
FAKE = 1 << 20  # a non-NULL device address: validation returns before anything could dereference it


def _fd(f, x, h=1e-6):
    g = np.zeros_like(x)
    for i in np.ndindex(x.shape):
        xp, xm = x.copy(), x.copy()
        xp[i] += h
        xm[i] -= h
        g[i] = (f(xp) - f(xm)) / (2 * h)
    return g


def _separated(rng, shape, min_gap=0.05):
    """points with pairwise distances >= min_gap (nearest neighbours stay put under the finite-difference steps)."""
    while True:
        x = rng.uniform(0, 1, size=shape)
        ok = True
        for a in x:
            d = np.sqrt(R.sqdist(a, a)) + np.eye(len(a))
            ok &= d.min() >= min_gap
        if ok:
            return x


# ----------------------------------------------------------------------------------------------------------------------
# the restatement against finite differences
# ----------------------------------------------------------------------------------------------------------------------
def test_nn_distance_grad_finite_differences():
    rng = np.random.default_rng(1)
    x1, x2 = _separated(rng, (2, 9, 3)), _separated(rng, (2, 6, 3))
    x1[1, :, 2] = 0.0  # a 2-D item
    x2[1, :, 2] = 0.0
    g1, g2 = rng.normal(size=(2, 9)), rng.normal(size=(2, 6))
    _, i1, _, i2 = R.nn_distance(x1, x2)
    gr1, gr2, _, _ = G.nn_distance_grad(x1, x2, g1, g2)
    fd1 = _fd(lambda x: G.nn_distance_value(x, x2, g1, g2, i1, i2), x1)
    fd2 = _fd(lambda x: G.nn_distance_value(x1, x, g1, g2, i1, i2), x2)
    np.testing.assert_allclose(gr1, fd1, atol=1e-6)
    np.testing.assert_allclose(gr2, fd2, atol=1e-6)
    # the held indices are the true nearest ones after the step: the restatement is the gradient of dist itself
    _, j1, _, j2 = R.nn_distance(x1 + 1e-6, x2)
    assert np.array_equal(i1, j1) and np.array_equal(i2, j2)


def test_match_cost_grad_finite_differences():
    rng = np.random.default_rng(2)
    x1, x2 = rng.uniform(size=(2, 8, 3)), rng.uniform(size=(2, 5, 3))
    mt = R.approx_match(x1, x2)  # held fixed
    g = np.array([0.8, -1.7])
    gr1, gr2, _, _ = G.match_cost_grad(x1, x2, mt, g)
    np.testing.assert_allclose(gr1, _fd(lambda x: (g * R.match_cost(x, x2, mt)).sum(), x1), atol=1e-6)
    np.testing.assert_allclose(gr2, _fd(lambda x: (g * R.match_cost(x1, x, mt)).sum(), x2), atol=1e-6)


def test_gather_point_grad_finite_differences():
    rng = np.random.default_rng(3)
    inp, idx = rng.normal(size=(7, 3)), np.array([0, 3, 3, 6, 0, 3, 5])
    go = rng.normal(size=(len(idx), 3))
    gi, a = G.gather_point_grad(go, idx, 7)
    np.testing.assert_allclose(gi, _fd(lambda x: (go * x[idx]).sum(), inp), atol=1e-6)
    assert (gi[[1, 2, 4]] == 0).all() and (a >= np.abs(gi)).all()


def test_chamfer_grad_finite_differences():
    rng = np.random.default_rng(4)
    t, p = _separated(rng, (1, 7, 3)), _separated(rng, (1, 9, 3))
    gt, gp, _, _ = G.chamfer_grad(t, p)
    np.testing.assert_allclose(gt, _fd(lambda x: G.chamfer(x, p).sum(), t), atol=1e-6)
    np.testing.assert_allclose(gp, _fd(lambda x: G.chamfer(t, x).sum(), p), atol=1e-6)


# ----------------------------------------------------------------------------------------------------------------------
# identities
# ----------------------------------------------------------------------------------------------------------------------
def test_translation_invariance():
    rng = np.random.default_rng(5)
    x1, x2 = rng.uniform(size=(3, 11, 3)), rng.uniform(size=(3, 7, 3))
    g1, g2 = rng.normal(size=(3, 11)), rng.normal(size=(3, 7))
    gr1, gr2, a1, a2 = G.nn_distance_grad(x1, x2, g1, g2)
    assert np.abs(gr1.sum(1) + gr2.sum(1)).max() <= 1e-12 * (a1.sum() + a2.sum())
    gr1, gr2, a1, a2 = G.match_cost_grad(x1, x2, R.approx_match(x1, x2), rng.normal(size=3))
    assert np.abs(gr1.sum(1) + gr2.sum(1)).max() <= 1e-12 * (a1.sum() + a2.sum())


def test_euler_relation():
    """dist is homogeneous of degree 2 in (x1, x2), match_cost of degree 1: <x, grad> = 2 sum g d and g cost."""
    rng = np.random.default_rng(6)
    x1, x2 = rng.uniform(size=(2, 10, 3)), rng.uniform(size=(2, 6, 3))
    g1, g2 = rng.normal(size=(2, 10)), rng.normal(size=(2, 6))
    d1, _, d2, _ = R.nn_distance(x1, x2)
    gr1, gr2, _, _ = G.nn_distance_grad(x1, x2, g1, g2)
    lhs = (x1 * gr1).sum() + (x2 * gr2).sum()
    assert abs(lhs - 2 * ((g1 * d1).sum() + (g2 * d2).sum())) <= 1e-12 * (1 + abs(lhs))
    mt, g = R.approx_match(x1, x2), np.array([1.5, 0.25])
    gr1, gr2, _, _ = G.match_cost_grad(x1, x2, mt, g)
    lhs = (x1 * gr1).sum() + (x2 * gr2).sum()
    assert abs(lhs - (g * R.match_cost(x1, x2, mt)).sum()) <= 1e-12 * (1 + abs(lhs))


# ----------------------------------------------------------------------------------------------------------------------
# C ABI without a device
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hip_lib():
    from dmcf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_version(hip_lib):
    assert hip_lib.dmcf_version() >= 21300


def test_symbols_declared_mirrored_exported(hip_lib):
    from dmcf_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dmcf_hip.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", text), f"{name} not declared in dmcf_hip.h"
        assert name in _lib.SYMBOLS
        fn = getattr(hip_lib, name)
        assert fn.argtypes is not None and fn.restype is not None, f"{name} has no ctypes prototype"


@pytest.mark.parametrize("q", ["dmcf_nn_distance_backward_workspace_bytes", "dmcf_match_cost_backward_workspace_bytes",
                               "dmcf_emd_backward_workspace_bytes"])
def test_pair_workspace_queries(hip_lib, q):
    f = getattr(hip_lib, q)
    assert f(1, 10 ** 5, 10 ** 5) >= f(1, 10 ** 4, 10 ** 4) >= f(1, 1000, 1000) > 0
    assert f(2, 1000, 1000) >= f(1, 1000, 1000)
    assert f(1, 1000, 2000) >= f(1, 1000, 1000) and f(1, 2000, 1000) >= f(1, 1000, 1000)
    for bad in ((-1, 10, 10), (1, -1, 10), (1, 10, -1)):
        assert f(*bad) == 0


def test_gather_workspace_query(hip_lib):
    f = hip_lib.dmcf_gather_point_backward_workspace_bytes
    assert f(10 ** 5, 10 ** 5) >= f(10 ** 4, 10 ** 5) >= f(10 ** 4, 10 ** 4) > 0
    assert f(-1, 10) == 0 and f(10, -1) == 0


def _counts(vals):
    return (ctypes.c_int32 * len(vals))(*vals)


def _check(f, ok, bad, ws_index):
    for args in bad:
        assert f(*args) == EINVAL, args
    short = list(ok)
    short[ws_index] -= 1
    assert f(*short) == EWORKSPACE


def test_nn_distance_backward_validation(hip_lib):
    L = hip_lib
    b, n, m = 2, 100, 50
    ws = L.dmcf_nn_distance_backward_workspace_bytes(b, n, m)
    ok = (FAKE, FAKE, b, n, m, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, ws, None)
    bad = [
        (None,) + ok[1:],                          # null xyz1
        ok[:1] + (None,) + ok[2:],                 # null xyz2
        ok[:2] + (-1,) + ok[3:],                   # negative b
        ok[:3] + (-5,) + ok[4:],                   # negative n
        ok[:4] + (-5,) + ok[5:],                   # negative m
        ok[:3] + (0,) + ok[4:],                    # empty xyz1 with b > 0
        ok[:5] + (None,) + ok[6:],                 # grad_dist1 without idx1
        ok[:6] + (None,) + ok[7:],                 # grad_dist2 without idx2
        ok[:9] + (None, None) + ok[11:],           # no output wanted
        ok[:11] + (None,) + ok[12:],               # null workspace
    ]
    _check(L.dmcf_nn_distance_backward, ok, bad, 12)
    assert L.dmcf_nn_distance_backward(*(ok[:2] + (0,) + ok[3:])) == 0  # b == 0: nothing to do


def test_match_cost_backward_validation(hip_lib):
    L = hip_lib
    b, n, m = 2, 100, 50
    ws = L.dmcf_match_cost_backward_workspace_bytes(b, n, m)
    ok = (FAKE, FAKE, b, n, m, FAKE, FAKE, FAKE, FAKE, FAKE, ws, None)
    bad = [
        (None,) + ok[1:], ok[:1] + (None,) + ok[2:],
        ok[:2] + (-1,) + ok[3:], ok[:3] + (-1,) + ok[4:], ok[:4] + (-1,) + ok[5:],
        ok[:5] + (None,) + ok[6:],                 # null match
        ok[:6] + (None,) + ok[7:],                 # null grad_cost
        ok[:7] + (None, None) + ok[9:],            # no output wanted
        ok[:9] + (None,) + ok[10:],                # null workspace
    ]
    _check(L.dmcf_match_cost_backward, ok, bad, 10)


def test_emd_backward_validation(hip_lib):
    L = hip_lib
    b, n, m = 2, 100, 50
    ws = L.dmcf_emd_backward_workspace_bytes(b, n, m)
    c1, c2 = _counts([100, 60]), _counts([50, 50])
    ok = (FAKE, FAKE, b, n, m, c1, c2, FAKE, FAKE, FAKE, FAKE, FAKE, ws, None)
    bad = [
        (None,) + ok[1:], ok[:1] + (None,) + ok[2:],
        ok[:2] + (-1,) + ok[3:], ok[:3] + (-1,) + ok[4:], ok[:4] + (-1,) + ok[5:],
        ok[:5] + (_counts([101, 3]),) + ok[6:],   # count beyond n
        ok[:6] + (_counts([5, -1]),) + ok[7:],    # negative count
        ok[:7] + (None,) + ok[8:],                 # null levels
        ok[:8] + (None,) + ok[9:],                 # null grad_cost
        ok[:9] + (None, None) + ok[11:],           # no output wanted
        ok[:11] + (None,) + ok[12:],               # null workspace
    ]
    _check(L.dmcf_emd_backward, ok, bad, 12)


def test_emd_with_levels_validation(hip_lib):
    L = hip_lib
    b, n, m = 2, 100, 50
    ws = L.dmcf_emd_workspace_bytes(b, n, m)
    ok = (FAKE, FAKE, b, n, m, None, None, FAKE, FAKE, FAKE, ws, None)
    bad = [
        (None,) + ok[1:], ok[:2] + (-1,) + ok[3:],
        ok[:5] + (_counts([101, 3]),) + ok[6:],
        ok[:7] + (None,) + ok[8:],                 # null cost
        ok[:8] + (None,) + ok[9:],                 # null levels
        ok[:9] + (None,) + ok[10:],                # null workspace
    ]
    _check(L.dmcf_emd_with_levels, ok, bad, 10)


def test_gather_point_backward_validation(hip_lib):
    L = hip_lib
    ws = L.dmcf_gather_point_backward_workspace_bytes(64, 100)
    ok = (FAKE, FAKE, 64, 3, 100, FAKE, FAKE, ws, None)
    bad = [
        (None,) + ok[1:], ok[:1] + (None,) + ok[2:],
        ok[:2] + (-1,) + ok[3:], ok[:3] + (0,) + ok[4:], ok[:4] + (-1,) + ok[5:],
        ok[:5] + (None,) + ok[6:],                 # null grad_inp
        ok[:6] + (None,) + ok[7:],                 # null workspace
    ]
    _check(L.dmcf_gather_point_backward, ok, bad, 7)


def test_reference_module_mirrors():
    from dmcf_amd import ops
    from dmcf_amd.utils.tools import nn_distance, sampling, tf_approxmatch
    assert nn_distance.nn_distance is ops.nn_distance and callable(nn_distance.chamfer_loss)
    assert tf_approxmatch.approx_match is ops.approx_match and tf_approxmatch.match_cost is ops.match_cost
    assert sampling.farthest_point_sample is ops.farthest_point_sample and sampling.gather_point is ops.gather_point
    assert issubclass(ops.EmdFunction, __import__("torch").autograd.Function)


def test_backward_helpers_refuse_cpu_tensors(hip_lib):
    """The public backward helpers check their operands before any pointer reaches the library: CPU tensors raise."""
    torch = pytest.importorskip("torch")
    from dmcf_amd import _lib, ops
    x1, x2 = torch.zeros(2, 5, 3), torch.zeros(2, 4, 3)
    calls = [
        lambda: ops.emd_with_levels(x1, x2),
        lambda: ops.emd_backward(x1, x2, torch.zeros(2, 10, 9), torch.ones(2)),
        lambda: ops.match_cost_backward(x1, x2, torch.zeros(2, 4, 5), torch.ones(2)),
        lambda: ops.nn_distance_backward(x1, x2, torch.zeros(2, 5, dtype=torch.int32), torch.zeros(2, 4, dtype=torch.int32),
                                         torch.ones(2, 5), torch.ones(2, 4)),
        lambda: ops.gather_point_backward(torch.ones(4, 3), torch.zeros(4, dtype=torch.int32), 10),
    ]
    for f in calls:
        with pytest.raises(_lib.DmcfError, match="no CPU fallback"):
            f()
