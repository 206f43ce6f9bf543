"""CPU checks of dmcf_lattice_conv_backward (ABI 2.16, dmcf_amd/csrc/cconv_lat_bwd.inc): version, symbols, the ctypes
declarations and the host-side validation -- every argument error comes back before anything is enqueued.  No device is touched."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["dmcf_lattice_conv_backward_workspace_bytes", "dmcf_lattice_conv_backward"]
OK, EINVAL, EWORKSPACE, EUNSUPPORTED = 0, -1, -2, -4
FAKE = 1 << 20  # a non-NULL, 256-byte aligned device address: validation returns before anything could dereference it
FLAG_NORMALIZE, FLAG_SYMMETRIC = 2, 4


@pytest.fixture(scope="module")
def hip_lib():
    from dmcf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def _part(n_out=100, dims=(4, 4, 4, 8, 16), base=(20, 6, 5), reach=2, step=1, stride=1, flags=0, filters=FAKE):
    """One launch over a base box at the origin whose volume is padded as the forward asks."""
    from dmcf_amd._lib import LatticeConvArgs
    a = LatticeConvArgs()
    a.filters = filters
    for k in range(5):
        a.filter_dims[k] = dims[k]
    a.inp_volume = a.out_table = a.offsets = FAKE
    a.out = None  # (the backward ignores it)
    for k in range(3):
        ext = (base[k] + 15) // 16 * 16 if k == 0 else base[k]
        a.inp_min[k] = -reach
        a.inp_dims[k] = (ext - 1) * step + 2 * reach + 1
        a.out_min[k], a.out_dims[k] = 0, base[k] * stride
        a.base_min[k], a.base_dims[k] = 0, base[k]
        a.reach[k] = reach
        a.voxel[k] = 0.125
    a.n_out, a.n_offsets = n_out, 57
    a.inp_step, a.out_stride = step, stride
    a.extent, a.window_fac, a.window = 0.6, 1.0, 2
    a.coordinate_mapping, a.interpolation = 1, 0
    a.flags = flags
    return a


def _arr(*parts):
    from dmcf_amd._lib import LatticeConvArgs
    arr = (LatticeConvArgs * max(len(parts), 1))()
    for i, p in enumerate(parts):
        arr[i] = p
    return arr


def _call(hip_lib, arr, n, grad_out=FAKE, gv=FAKE, gw=FAKE, ws=FAKE, nbytes=None):
    if nbytes is None:
        nbytes = hip_lib.dmcf_lattice_conv_backward_workspace_bytes(arr, n)
    return hip_lib.dmcf_lattice_conv_backward(arr, n, grad_out, gv, gw, ws, nbytes, None)


def test_version(hip_lib):
    assert hip_lib.dmcf_version() >= 21600


def test_symbols_exported_declared_and_listed(hip_lib):
    from dmcf_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dmcf_hip.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", text), f"{name} not declared in dmcf_hip.h"
        assert name in _lib.SYMBOLS
        assert hasattr(hip_lib, name)
    c = ctypes
    fn = hip_lib.dmcf_lattice_conv_backward
    assert fn.restype is c.c_int
    assert fn.argtypes == [c.POINTER(_lib.LatticeConvArgs), c.c_int32, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_size_t,
                           c.c_void_p]
    ws = hip_lib.dmcf_lattice_conv_backward_workspace_bytes
    assert ws.restype is c.c_size_t and ws.argtypes == [c.POINTER(_lib.LatticeConvArgs), c.c_int32]
    proto = re.search(r"int\s+dmcf_lattice_conv_backward\s*\(([^)]*)\)", text).group(1)
    assert [p.split()[-1].lstrip("*") for p in proto.split(",")] == ["parts", "n_parts", "grad_out", "grad_volume", "grad_filters",
                                                                     "workspace", "workspace_bytes", "stream"]


def test_number_of_parts(hip_lib):
    arr = _arr(*[_part() for _ in range(9)])
    for n in (0, 9, -1):
        assert _call(hip_lib, arr, n, nbytes=1 << 30) == EINVAL
        assert hip_lib.dmcf_lattice_conv_backward_workspace_bytes(arr, n) == 256
    assert hip_lib.dmcf_lattice_conv_backward(None, 1, FAKE, FAKE, FAKE, FAKE, 1 << 30, None) == EINVAL


def test_parts_must_belong_together(hip_lib):
    assert _call(hip_lib, _arr(_part(), _part(filters=FAKE + 4096)), 2, nbytes=1 << 30) == EINVAL
    assert _call(hip_lib, _arr(_part(), _part(n_out=99)), 2, nbytes=1 << 30) == EINVAL
    other_volume = _part()
    other_volume.inp_volume = FAKE + 4096
    assert _call(hip_lib, _arr(_part(), other_volume), 2, nbytes=1 << 30) == EINVAL


@pytest.mark.parametrize("flags", [FLAG_SYMMETRIC, FLAG_NORMALIZE])
def test_options_the_forward_refuses(hip_lib, flags):
    assert _call(hip_lib, _arr(_part(flags=flags)), 1, nbytes=1 << 30) == EUNSUPPORTED


def test_channels_and_steps(hip_lib):
    assert _call(hip_lib, _arr(_part(dims=(4, 4, 4, 5, 16))), 1, nbytes=1 << 30) == EUNSUPPORTED
    assert _call(hip_lib, _arr(_part(dims=(4, 4, 4, 8, 33))), 1, nbytes=1 << 30) == EUNSUPPORTED
    assert _call(hip_lib, _arr(_part(step=3)), 1, nbytes=1 << 30) == EUNSUPPORTED
    assert _call(hip_lib, _arr(_part(step=2, stride=2)), 1, nbytes=1 << 30) == EUNSUPPORTED


def test_outputs_and_operands(hip_lib):
    arr = _arr(_part())
    assert _call(hip_lib, arr, 1, gv=None, gw=None) == EINVAL  # nothing to compute
    assert _call(hip_lib, arr, 1, grad_out=None) == EINVAL


def test_workspace(hip_lib):
    arr = _arr(_part())
    need = hip_lib.dmcf_lattice_conv_backward_workspace_bytes(arr, 1)
    assert need > hip_lib.dmcf_lattice_conv_workspace_bytes(arr)  # the forward's workspace is a part of it
    assert _call(hip_lib, arr, 1, nbytes=need - 1) == EWORKSPACE  # the forward's error for a short workspace
    assert _call(hip_lib, arr, 1, ws=None) == EINVAL
    assert _call(hip_lib, arr, 1, ws=FAKE + 8) == EINVAL  # not 256-byte aligned
    sizes = [hip_lib.dmcf_lattice_conv_backward_workspace_bytes(_arr(_part(n_out=n)), 1) for n in (0, 1, 1000, 1024, 1025, 10 ** 5, 10 ** 6)]
    assert sizes == sorted(sizes) and sizes[-1] > sizes[0]


def test_volume_must_hold_every_reachable_cell(hip_lib):
    short = _part()
    short.inp_dims[0] -= 1
    assert _call(hip_lib, _arr(short), 1, nbytes=1 << 30) == EINVAL


def test_ops_refuses_unknown_keywords():
    """A misspelt option must not be dropped: the gradient would be that of another convolution (raised at call binding)."""
    torch = pytest.importorskip("torch")
    from dmcf_amd import ops
    W, vol, table = torch.zeros(4, 4, 4, 8, 16), torch.zeros(9, 9, 9, 8), torch.zeros(5, 5, 5, dtype=torch.int32)
    with pytest.raises(TypeError):
        ops.lattice_conv_backward(W, vol, (-2, -2, -2), table, (0, 0, 0), 10, (0.125,) * 3, 0.6, torch.zeros(10, 16), windw="poly6")
