"""CPU checks of the per-point extent entry points (dmcf_radius_search_*, dmcf_cconv_forward_extents) and of their Python
surface: symbols, host-side validation and the errors raised before any launch.  No device is touched."""
import ctypes
import os
import re

import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["dmcf_radius_search_count", "dmcf_radius_search_write", "dmcf_cconv_forward_extents", "dmcf_cconv_extents_kernel_name"]
EINVAL, EUNSUPPORTED = -1, -4
FAKE = 1 << 20  # a non-NULL device address: validation returns before anything could dereference it


@pytest.fixture(scope="module")
def hip_lib():
    from dmcf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_symbols_exported_declared_and_listed(hip_lib):
    from dmcf_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dmcf_hip.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", text), f"{name} not declared in dmcf_hip.h"
        assert name in _lib.SYMBOLS
        assert hasattr(hip_lib, name)


def test_version(hip_lib):
    assert hip_lib.dmcf_version() >= 20700


def test_radius_search_host_validation(hip_lib):
    from dmcf_amd import ops
    L = hip_lib
    nb = L.dmcf_frs_workspace_bytes(100, 100)
    rs = ctypes.c_void_p(FAKE)
    q, r, ws = ctypes.c_void_p(FAKE), ctypes.c_void_p(FAKE), ctypes.c_void_p(FAKE)
    # null workspace, null radii, max_radius <= 0
    assert L.dmcf_radius_search_count(q, 100, 100, r, 0.5, 0, None, nb, rs, None) == EINVAL
    assert L.dmcf_radius_search_count(q, 100, 100, None, 0.5, 0, ws, nb, rs, None) == EINVAL
    assert L.dmcf_radius_search_count(q, 100, 100, r, 0.0, 0, ws, nb, rs, None) == EINVAL
    assert L.dmcf_radius_search_count(q, 100, 100, r, -1.0, 0, ws, nb, rs, None) == EINVAL
    assert L.dmcf_radius_search_count(q, 100, 100, r, float("nan"), 0, ws, nb, rs, None) == EINVAL
    idx = ctypes.c_void_p(FAKE)
    assert L.dmcf_radius_search_write(q, 100, 100, r, 0.5, 0, None, nb, rs, idx, None, 10, None) == EINVAL
    assert L.dmcf_radius_search_write(q, 100, 100, None, 0.5, 0, ws, nb, rs, idx, None, 10, None) == EINVAL
    assert L.dmcf_radius_search_write(q, 100, 100, r, 0.0, 0, ws, nb, rs, idx, None, 10, None) == EINVAL
    # the hash-walk emulations of FixedRadiusSearch have no meaning for RadiusSearch
    for flag in (ops.FRS_OPEN3D_VOXEL_WALK, ops.FRS_OPEN3D_CORNER_VOXELS, 8):
        assert L.dmcf_radius_search_count(q, 100, 100, r, 0.5, flag, ws, nb, rs, None) == EINVAL
        assert L.dmcf_radius_search_write(q, 100, 100, r, 0.5, flag, ws, nb, rs, idx, None, 10, None) == EINVAL


def _args(n_out=16, flags=0):
    from dmcf_amd._lib import CconvArgs
    a = CconvArgs()
    a.filters = FAKE
    for d, v in enumerate((4, 4, 4, 8, 16)):
        a.filter_dims[d] = v
    a.out_positions, a.inp_positions, a.inp_features = FAKE, FAKE, FAKE
    a.n_out, a.n_inp = n_out, 32
    a.neighbors_index, a.neighbors_row_splits = FAKE, FAKE
    a.extent = 0.0  # ignored by the extents entry points
    a.window_fac = 1.0
    a.coordinate_mapping, a.interpolation = 1, 0
    a.flags = flags
    a.out = FAKE
    return a


def test_cconv_extents_host_validation(hip_lib):
    from dmcf_amd import ops
    L = hip_lib
    ext = ctypes.c_void_p(FAKE)
    a = _args()
    assert L.dmcf_cconv_forward_extents(ctypes.byref(a), None, None, 0, None) == EINVAL  # out_extents NULL, n_out > 0
    a = _args(flags=ops.FLAG_SKIP_SELF)
    assert L.dmcf_cconv_forward_extents(ctypes.byref(a), ext, None, 0, None) == EUNSUPPORTED
    name = ctypes.create_string_buffer(96)
    assert L.dmcf_cconv_extents_kernel_name(ctypes.byref(a), name, 96) == EUNSUPPORTED
    # args->extent is ignored: a zero extent names the kernel, and an empty output set is a no-op without extents
    a = _args()
    assert L.dmcf_cconv_extents_kernel_name(ctypes.byref(a), name, 96) == 0
    assert name.value.decode() == "cconv_ext_kernel<8>"
    a = _args(n_out=0)
    assert L.dmcf_cconv_forward_extents(ctypes.byref(a), None, None, 0, None) == 0
    # the scalar entry point still rejects the zero extent
    assert L.dmcf_cconv_forward(ctypes.byref(_args()), None, 0, None) == EINVAL


def test_radius_search_refuses_cpu_and_other_metrics():
    from dmcf_amd import ops, _lib
    rs = ops.RadiusSearch(return_distances=True, normalize_distances=True)
    with pytest.raises(_lib.DmcfError):
        rs(torch.zeros(4, 3), torch.zeros(4, 3), torch.full((4,), 0.5))
    with pytest.raises(NotImplementedError):
        ops.RadiusSearch(metric="L1")
    with pytest.raises(NotImplementedError):
        rs(torch.zeros(4, 3), torch.zeros(4, 3), torch.full((4,), 0.5), points_row_splits=torch.tensor([0, 4]))


def _conv_operands(n_out=5):
    filt = torch.zeros(4, 4, 4, 8, 16)
    out_pos, inp_pos, feat = torch.zeros(n_out, 3), torch.zeros(7, 3), torch.zeros(7, 8)
    idx = torch.zeros(0, dtype=torch.int32)
    rs = torch.zeros(n_out + 1, dtype=torch.int64)
    return filt, out_pos, inp_pos, feat, idx, rs


def test_continuous_conv_extents_errors():
    from dmcf_amd import ops, _lib
    filt, out_pos, inp_pos, feat, idx, rs = _conv_operands(5)
    empty = torch.zeros(0)

    def call(ext):
        return ops.continuous_conv(filt, out_pos, ext, torch.zeros(3), inp_pos, feat, empty, idx, rs, empty)

    with pytest.raises(_lib.DmcfError):  # CPU tensors, extents of a valid shape
        call(torch.full((5,), 0.2))
    with pytest.raises(_lib.DmcfError):
        call(torch.full((5, 1), 0.2))
    with pytest.raises(NotImplementedError):  # anisotropic
        call(torch.full((5, 3), 0.2))
    with pytest.raises(NotImplementedError):
        call(torch.full((1, 3), 0.2))
    with pytest.raises(ValueError):  # wrong length
        call(torch.full((4,), 0.2))
    with pytest.raises(ValueError):
        call(torch.full((6, 1), 0.2))
    with pytest.raises(ValueError):
        ops.cconv_forward(filt, out_pos, torch.full((4,), 0.2), inp_pos, feat, idx, rs)


def test_layers_reject_wrong_length_extents():
    from dmcf_amd.utils.convolutions import ContinuousConv, PointSampling
    conv = ContinuousConv(filters=4, kernel_size=[4, 4, 4], device="cpu")
    with pytest.raises(ValueError):
        conv(torch.zeros(7, 2), torch.zeros(7, 3), torch.zeros(5, 3), torch.full((4,), 0.2))
    with pytest.raises(NotImplementedError):
        conv(torch.zeros(7, 2), torch.zeros(7, 3), torch.zeros(5, 3), torch.full((5, 3), 0.2))
    with pytest.raises(ValueError):
        PointSampling()(torch.zeros(7, 2), torch.zeros(7, 3), torch.zeros(5, 3), torch.full((6,), 0.2))
