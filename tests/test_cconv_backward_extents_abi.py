"""CPU checks of dmcf_cconv_backward_extents (ABI 2.15, dmcf_amd/csrc/cconv_bwd.hip): version, symbols, the ctypes mirror,
host-side validation -- every argument error comes back before anything is enqueued -- and the kernel-name diagnostic.  No
device is touched."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["dmcf_cconv_backward_extents", "dmcf_cconv_backward_extents_kernel_names"]
EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -4
FAKE = 1 << 20  # a non-NULL, 256-byte aligned device address: validation returns before anything could dereference it
FLAG_NORMALIZE, FLAG_SYMMETRIC, FLAG_SKIP_SELF = 2, 4, 16


@pytest.fixture(scope="module")
def hip_lib():
    from dmcf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def _fwd(n_out=16, n_inp=16, flags=0, dims=(4, 4, 4, 3, 5), extent=0.0):
    from dmcf_amd._lib import CconvArgs
    a = CconvArgs()
    a.filters = FAKE
    for d in range(5):
        a.filter_dims[d] = dims[d]
    a.sym_axis = 2
    a.out_positions = a.inp_positions = a.inp_features = FAKE
    a.n_out, a.n_inp = n_out, n_inp
    a.neighbors_index = a.neighbors_row_splits = FAKE
    a.extent = extent  # (ignored by the individual-extent call: 0 would be DMCF_EINVAL in dmcf_cconv_backward)
    a.window_fac = 1.0
    a.window = 2
    a.coordinate_mapping = 1
    a.flags = flags
    a.n_pairs = 100
    return a


def _bwd(n_inp=16, **kw):
    from dmcf_amd._lib import CconvBackwardArgs
    b = CconvBackwardArgs()
    b.struct_size = ctypes.sizeof(CconvBackwardArgs)
    b.grad_out = FAKE
    b.inv_index = b.inv_pair = b.inv_row_splits = FAKE
    b.inv_n_rows = n_inp
    b.inv_n_pairs = 100
    b.grad_filters = b.grad_inp_features = FAKE
    for k, v in kw.items():
        setattr(b, k, v)
    return b


def test_version(hip_lib):
    assert hip_lib.dmcf_version() >= 21500


def test_symbols_exported_declared_and_listed(hip_lib):
    from dmcf_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dmcf_hip.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", text), f"{name} not declared in dmcf_hip.h"
        assert name in _lib.SYMBOLS
        assert hasattr(hip_lib, name)
    c = ctypes
    fn = hip_lib.dmcf_cconv_backward_extents
    assert fn.restype is c.c_int
    assert fn.argtypes == [c.POINTER(_lib.CconvArgs), c.POINTER(_lib.CconvBackwardArgs), c.c_void_p, c.c_void_p, c.c_size_t,
                           c.c_void_p]
    # the header's prototype: (fwd, bwd, out_extents, workspace, workspace_bytes, stream)
    proto = re.search(r"int\s+dmcf_cconv_backward_extents\s*\(([^)]*)\)", text).group(1)
    assert [p.split()[-1].lstrip("*") for p in proto.split(",")] == ["fwd", "bwd", "out_extents", "workspace", "workspace_bytes",
                                                                     "stream"]


def test_host_validation(hip_lib):
    L = hip_lib
    ext = ctypes.c_void_p(FAKE)
    ws = ctypes.c_void_p(FAKE)
    a = _fwd()

    def call(b, args=a, extents=ext, workspace=ws, nbytes=1 << 40):
        return L.dmcf_cconv_backward_extents(ctypes.byref(args), ctypes.byref(b), extents, workspace, nbytes, None)

    assert call(_bwd(), extents=None) == EINVAL                                      # NULL out_extents with n_out > 0
    assert call(_bwd(), _fwd(flags=FLAG_SKIP_SELF)) == EUNSUPPORTED                  # as the forward
    assert call(_bwd(struct_size=ctypes.sizeof(_bwd()) - 8)) == EINVAL               # short struct
    assert call(_bwd(struct_size=0)) == EINVAL
    assert call(_bwd(grad_out=None)) == EINVAL
    assert call(_bwd(inv_n_rows=17)) == EINVAL                                       # list of another point set
    assert call(_bwd(flags=2)) == EINVAL                                             # unknown flag
    assert L.dmcf_cconv_backward_extents(None, ctypes.byref(_bwd()), ext, ws, 1 << 40, None) == EINVAL
    assert L.dmcf_cconv_backward_extents(ctypes.byref(a), None, ext, ws, 1 << 40, None) == EINVAL
    # the unchanged limits of dmcf_cconv_backward: K * Cin / K * Cout, ASCC on the sharded layout
    assert call(_bwd(), _fwd(dims=(8, 8, 8, 64, 64))) == EUNSUPPORTED
    assert call(_bwd(inv_n_rows=20), _fwd(n_out=16, n_inp=20, flags=FLAG_SYMMETRIC, dims=(4, 4, 2, 3, 5))) == EUNSUPPORTED
    # the workspace: sized by dmcf_cconv_backward_workspace_bytes, whatever the (positive) extent
    need = L.dmcf_cconv_backward_workspace_bytes(ctypes.byref(_fwd(extent=0.2)), ctypes.byref(_bwd()))
    assert need > 256
    assert need == L.dmcf_cconv_backward_workspace_bytes(ctypes.byref(_fwd(extent=7.0)), ctypes.byref(_bwd()))
    assert call(_bwd(), nbytes=need - 1) == EWORKSPACE                               # too small
    assert call(_bwd(), workspace=None, nbytes=0) == EINVAL                          # none at all
    assert call(_bwd(), workspace=ctypes.c_void_p(FAKE + 8)) == EINVAL               # not 256-byte aligned
    # args->extent is ignored: the valid calls above ran with extent = 0, which the scalar entry point refuses
    assert L.dmcf_cconv_backward(ctypes.byref(a), ctypes.byref(_bwd()), ws, 1 << 40, None) == EINVAL
    # nothing wanted: nothing to do, no workspace needed
    assert call(_bwd(grad_filters=None, grad_inp_features=None), workspace=None, nbytes=0) == 0


def test_kernel_names(hip_lib):
    L = hip_lib
    name = ctypes.create_string_buffer(256)
    assert L.dmcf_cconv_backward_extents_kernel_names(ctypes.byref(_fwd()), ctypes.byref(_bwd()), name, 256) == 0
    assert name.value.decode().split(";") == ["cconv_bwd_input_ext", "cconv_bwd_filter_splat_ext", "cconv_bwd_filter_gemm",
                                              "cconv_bwd_filter_reduce", "cconv_bwd_filter_store"]
    a = _fwd(flags=FLAG_SYMMETRIC | FLAG_NORMALIZE, dims=(4, 4, 2, 3, 5))
    assert L.dmcf_cconv_backward_extents_kernel_names(ctypes.byref(a), ctypes.byref(_bwd(grad_filters=None)), name, 256) == 0
    assert name.value.decode() == "cconv_bwd_norm_ext;cconv_bwd_expand;cconv_bwd_input_ext"
    assert L.dmcf_cconv_backward_extents_kernel_names(ctypes.byref(_fwd(flags=FLAG_SKIP_SELF)), ctypes.byref(_bwd()), name,
                                                      256) == EUNSUPPORTED
    assert L.dmcf_cconv_backward_extents_kernel_names(ctypes.byref(_fwd()), ctypes.byref(_bwd(grad_out=None)), name, 256) == EINVAL
    assert L.dmcf_cconv_backward_extents_kernel_names(ctypes.byref(_fwd()), ctypes.byref(_bwd()), name, 8) == EINVAL
    # the scalar call keeps its names
    assert L.dmcf_cconv_backward_kernel_names(ctypes.byref(_fwd(extent=0.2)), ctypes.byref(_bwd()), name, 256) == 0
    assert "_ext" not in name.value.decode()


def test_ops_surface_before_launch():
    torch = pytest.importorskip("torch")
    from dmcf_amd import ops
    W = torch.zeros(4, 4, 4, 3, 5, requires_grad=True)
    P = torch.zeros(10, 3)
    F = torch.zeros(10, 3)
    idx = torch.zeros(0, dtype=torch.int32)
    rs = torch.zeros(11, dtype=torch.int64)
    G = torch.zeros(10, 5)
    ext = torch.full((10,), 0.2)
    # recording with per-point extents is opt-in, and then still refuses out= / accumulate
    with pytest.raises(NotImplementedError):
        ops.cconv_forward(W, P, ext, P, F, idx, rs)
    with pytest.raises(ValueError):
        ops.cconv_forward(W, P, ext, P, F, idx, rs, out=torch.zeros(10, 5), record_per_point_extents=True)
    with pytest.raises(ValueError):
        ops.cconv_backward(W.detach(), P, torch.full((9,), 0.2), P, F, idx, rs, G)       # one extent per output row
    with pytest.raises(NotImplementedError):
        ops.cconv_backward(W.detach(), P, torch.full((10, 3), 0.2), P, F, idx, rs, G)    # anisotropic
    with pytest.raises(TypeError):
        ops.cconv_backward(W.detach(), P, 0.2, P, F, idx, rs, G, normalise=True)             # a misspelt option is not dropped
