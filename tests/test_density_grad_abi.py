"""CPU checks of dmcf_frs_window_sum_backward (ABI 2.14, dmcf_amd/csrc/frs.hip): version, symbol, ctypes mirror and the
argument errors, which are returned before anything is enqueued (no device is touched)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "dmcf_frs_window_sum_backward"
EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -4
FAKE = 1 << 20  # a non-NULL device address: validation returns before anything could dereference it
WINDOW_NONE, WINDOW_EXPLICIT, WINDOW_POLY6, WINDOW_CUBIC_GRAD = 0, 1, 2, 6
IGNORE_QUERY_POINT, OPEN3D_CORNER_VOXELS, OPEN3D_VOXEL_WALK = 1, 2, 4


@pytest.fixture(scope="module")
def hip_lib():
    from dmcf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_version(hip_lib):
    assert hip_lib.dmcf_version() >= 21400


def test_symbol_declared_mirrored_exported(hip_lib):
    from dmcf_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dmcf_hip.h")).read(), flags=re.S)
    assert re.search(r"\b" + NAME + r"\s*\(", text), f"{NAME} not declared in dmcf_hip.h"
    assert NAME in _lib.SYMBOLS
    fn = getattr(hip_lib, NAME)
    assert fn.argtypes is not None and len(fn.argtypes) == 12 and fn.restype is not None


def test_host_validation(hip_lib):
    L = hip_lib
    m, n = 100, 50
    ws = L.dmcf_frs_workspace_bytes(n, m)
    assert ws > 0
    f = getattr(L, NAME)
    #     queries m  n  radius flags window        cq    cp    workspace bytes grad stream
    ok = (FAKE, m, n, 0.1, 0, WINDOW_POLY6, FAKE, FAKE, FAKE, ws, FAKE, None)
    bad = [
        (None,) + ok[1:],                            # null queries
        ok[:10] + (None,) + ok[11:],                 # null output
        ok[:8] + (None,) + ok[9:],                   # null workspace
        ok[:6] + (None, None) + ok[8:],              # both coefficients NULL
        ok[:1] + (-1,) + ok[2:],                     # negative query count
        ok[:2] + (-1,) + ok[3:],                     # negative point count
        ok[:3] + (0.0,) + ok[4:],                    # radius
        ok[:3] + (float("nan"),) + ok[4:],
        ok[:4] + (8,) + ok[5:],                      # unknown flag
        ok[:4] + (OPEN3D_CORNER_VOXELS | OPEN3D_VOXEL_WALK,) + ok[5:],
        ok[:5] + (-1,) + ok[6:],                     # window ids
        ok[:5] + (WINDOW_CUBIC_GRAD + 1,) + ok[6:],
    ]
    for args in bad:
        assert f(*args) == EINVAL, args
    # the count has no gradient; the open3d readings are differentiated on the pair list
    assert f(*(ok[:5] + (WINDOW_NONE,) + ok[6:])) == EUNSUPPORTED
    for flag in (OPEN3D_CORNER_VOXELS, OPEN3D_VOXEL_WALK, OPEN3D_VOXEL_WALK | IGNORE_QUERY_POINT):
        assert f(*(ok[:4] + (flag,) + ok[5:])) == EUNSUPPORTED
    assert f(*(ok[:9] + (ws - 1,) + ok[10:])) == EWORKSPACE
    # nothing to do: no query (either coefficient alone is enough, every differentiable window is accepted)
    for window in range(WINDOW_EXPLICIT, WINDOW_CUBIC_GRAD + 1):
        assert f(*(ok[:1] + (0,) + ok[2:5] + (window, None, FAKE) + ok[8:])) == 0
        assert f(*(ok[:1] + (0,) + ok[2:4] + (IGNORE_QUERY_POINT, window, FAKE, None) + ok[8:])) == 0
    assert f(*((None, 0) + ok[2:10] + (None, None))) == 0


def test_ops_refuse_cpu_tensors():
    torch = pytest.importorskip("torch")
    from dmcf_amd import _lib, ops
    a = torch.zeros((5, 3), requires_grad=True)
    with pytest.raises(_lib.DmcfError):
        ops.window_sum(a, a, 0.1, "poly6")
