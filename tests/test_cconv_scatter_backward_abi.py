"""CPU checks of dmcf_cconv_scatter_backward (ABI 2.19, dmcf_amd/csrc/cconv_sct_bwd.inc): version, symbols, the ctypes
declarations and the host-side validation -- every argument error comes back before anything is enqueued.  No device is touched."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["dmcf_cconv_scatter_backward_workspace_bytes", "dmcf_cconv_scatter_backward"]
OK, EINVAL, EWORKSPACE, EUNSUPPORTED = 0, -1, -2, -4
FAKE = 1 << 20  # a non-NULL, 256-byte aligned device address: validation returns before anything could dereference it
FLAG_ALIGN_CORNERS, FLAG_ACCUMULATE = 1, 8
WINDOW_NONE, WINDOW_POLY6, WINDOW_CUBIC = 0, 2, 3


@pytest.fixture(scope="module")
def hip_lib():
    from dmcf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def _fwd(dims=(4, 4, 4, 24, 4), n_out=1000, n_inp=5000, window=WINDOW_POLY6, flags=FLAG_ALIGN_CORNERS, extent=0.8, cap=10 ** 5, **ptr):
    """The forward's struct as the backward reads it: no plan, no out, no bias."""
    from dmcf_amd._lib import CconvScatterArgs
    a = CconvScatterArgs()
    for k in range(5):
        a.filter_dims[k] = dims[k]
    for name in ("filters", "out_positions", "inp_positions", "inp_features", "t_index", "t_row_begin"):
        setattr(a, name, ptr.get(name, FAKE))
    a.t_row_count = ptr.get("t_row_count", None)
    a.n_out, a.n_inp, a.t_capacity = n_out, n_inp, cap
    a.plan = a.out = a.bias = a.error_flag = None
    a.block_cells = a.reach = 0
    a.extent, a.window_fac, a.window, a.flags = extent, 1.0, window, flags
    return a


def _bwd(grad_out=FAKE, gw=FAKE, gf=FAKE, flags=0, size=None):
    from dmcf_amd._lib import CconvScatterBackwardArgs
    b = CconvScatterBackwardArgs()
    b.struct_size = ctypes.sizeof(CconvScatterBackwardArgs) if size is None else size
    b.flags = flags
    b.grad_out, b.grad_filters, b.grad_inp_features = grad_out, gw, gf
    return b


def _call(hip_lib, a, b, ws=FAKE, nbytes=None):
    if nbytes is None:
        nbytes = hip_lib.dmcf_cconv_scatter_backward_workspace_bytes(ctypes.byref(a), ctypes.byref(b))
    return hip_lib.dmcf_cconv_scatter_backward(ctypes.byref(a), ctypes.byref(b), ws, nbytes, None)


def test_version(hip_lib):
    assert hip_lib.dmcf_version() >= 21900


def test_flag_values_are_the_header_s():
    text = open(os.path.join(ROOT, "include", "dmcf_hip.h")).read()
    for name, value in (("DMCF_FLAG_ALIGN_CORNERS", FLAG_ALIGN_CORNERS), ("DMCF_FLAG_ACCUMULATE", FLAG_ACCUMULATE),
                        ("DMCF_WINDOW_NONE", WINDOW_NONE), ("DMCF_WINDOW_POLY6", WINDOW_POLY6), ("DMCF_WINDOW_CUBIC", WINDOW_CUBIC)):
        m = re.search(r"\b" + name + r"\s*=?\s*\(?\s*(0x[0-9a-fA-F]+|\d+(?:\s*<<\s*\d+)?)", text)
        assert m, name
        assert eval(m.group(1)) == value, name  # noqa: S307 (a literal of the header)


def test_symbols_exported_declared_and_listed(hip_lib):
    from dmcf_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dmcf_hip.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", text), f"{name} not declared in dmcf_hip.h"
        assert name in _lib.SYMBOLS
        assert hasattr(hip_lib, name)
    c = ctypes
    fn = hip_lib.dmcf_cconv_scatter_backward
    assert fn.restype is c.c_int
    assert fn.argtypes == [c.POINTER(_lib.CconvScatterArgs), c.POINTER(_lib.CconvScatterBackwardArgs), c.c_void_p, c.c_size_t, c.c_void_p]
    ws = hip_lib.dmcf_cconv_scatter_backward_workspace_bytes
    assert ws.restype is c.c_size_t
    assert ws.argtypes == [c.POINTER(_lib.CconvScatterArgs), c.POINTER(_lib.CconvScatterBackwardArgs)]
    proto = re.search(r"int\s+dmcf_cconv_scatter_backward\s*\(([^)]*)\)", text).group(1)
    assert [p.split()[-1].lstrip("*") for p in proto.split(",")] == ["fwd", "bwd", "workspace", "workspace_bytes", "stream"]
    proto = re.search(r"size_t\s+dmcf_cconv_scatter_backward_workspace_bytes\s*\(([^)]*)\)", text).group(1)
    assert [p.split()[-1].lstrip("*") for p in proto.split(",")] == ["fwd", "bwd"]


def test_struct_matches_the_header():
    from dmcf_amd import _lib
    text = open(os.path.join(ROOT, "include", "dmcf_hip.h")).read()
    body = re.search(r"typedef struct dmcf_cconv_scatter_backward_args \{(.*?)\} dmcf_cconv_scatter_backward_args;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [d.split()[-1].lstrip("*") for d in body.split(";") if d.strip()]
    assert names == [f[0] for f in _lib.CconvScatterBackwardArgs._fields_]
    assert ctypes.sizeof(_lib.CconvScatterBackwardArgs) == 32


def test_a_valid_call_passes_validation_up_to_the_workspace(hip_lib):
    """The baseline of every case below: these arguments are refused for the workspace alone."""
    a, b = _fwd(), _bwd()
    assert _call(hip_lib, a, b, nbytes=0) == EWORKSPACE
    for cout in (4, 8):
        assert _call(hip_lib, _fwd(dims=(4, 4, 4, 32, cout)), b, nbytes=0) == EWORKSPACE
    assert _call(hip_lib, _fwd(window=WINDOW_NONE), b, nbytes=0) == EWORKSPACE
    assert _call(hip_lib, _fwd(flags=FLAG_ALIGN_CORNERS | FLAG_ACCUMULATE), b, nbytes=0) == EWORKSPACE  # (ignored)
    assert _call(hip_lib, _fwd(t_row_count=FAKE), b, nbytes=0) == EWORKSPACE
    assert _call(hip_lib, a, _bwd(gw=None), nbytes=0) == EWORKSPACE
    assert _call(hip_lib, a, _bwd(gf=None), nbytes=0) == EWORKSPACE


@pytest.mark.parametrize("spec", [dict(dims=(3, 3, 3, 24, 4)), dict(dims=(4, 4, 4, 24, 5)), dict(dims=(4, 4, 4, 33, 4)),
                                  dict(dims=(4, 4, 4, 24, 16)), dict(window=WINDOW_CUBIC), dict(flags=0), dict(flags=FLAG_ALIGN_CORNERS | 2)],
                         ids=["3x3x3", "cout5", "cin33", "cout16", "cubic", "no-align-corners", "normalize"])
def test_what_the_forward_refuses(hip_lib, spec):
    assert _call(hip_lib, _fwd(**spec), _bwd(), nbytes=1 << 30) == EUNSUPPORTED


def test_struct_size_and_flags(hip_lib):
    from dmcf_amd._lib import CconvScatterBackwardArgs
    a = _fwd()
    assert _call(hip_lib, a, _bwd(size=ctypes.sizeof(CconvScatterBackwardArgs) - 1), nbytes=1 << 30) == EINVAL
    assert _call(hip_lib, a, _bwd(size=0), nbytes=1 << 30) == EINVAL
    assert _call(hip_lib, a, _bwd(flags=1), nbytes=1 << 30) == EINVAL


def test_outputs_and_operands(hip_lib):
    a = _fwd()
    assert _call(hip_lib, a, _bwd(gw=None, gf=None), nbytes=1 << 30) == EINVAL  # nothing to compute
    assert _call(hip_lib, a, _bwd(grad_out=None), nbytes=1 << 30) == EINVAL
    for off in (4, 8, 12):  # its rows are read 16 bytes at a time
        assert _call(hip_lib, a, _bwd(grad_out=FAKE + off), nbytes=1 << 30) == EINVAL
    assert _call(hip_lib, a, _bwd(grad_out=FAKE + 16), nbytes=0) == EWORKSPACE
    for name in ("filters", "out_positions", "inp_positions", "inp_features", "t_index", "t_row_begin"):
        assert _call(hip_lib, _fwd(**{name: None}), _bwd(), nbytes=1 << 30) == EINVAL, name
    assert hip_lib.dmcf_cconv_scatter_backward(None, ctypes.byref(_bwd()), FAKE, 1 << 30, None) == EINVAL
    assert hip_lib.dmcf_cconv_scatter_backward(ctypes.byref(a), None, FAKE, 1 << 30, None) == EINVAL
    for spec in (dict(n_out=0), dict(n_inp=0), dict(n_out=-1), dict(n_inp=-5), dict(extent=0.0), dict(extent=-0.8), dict(cap=-1)):
        assert _call(hip_lib, _fwd(**spec), _bwd(), nbytes=1 << 30) == EINVAL, spec


def test_workspace(hip_lib):
    a, b = _fwd(), _bwd()
    need = hip_lib.dmcf_cconv_scatter_backward_workspace_bytes(ctypes.byref(a), ctypes.byref(b))
    assert need > 0
    assert _call(hip_lib, a, b, nbytes=need - 1) == EWORKSPACE
    assert _call(hip_lib, a, b, ws=None) == EINVAL
    assert _call(hip_lib, a, b, ws=FAKE + 8) == EINVAL  # not 256-byte aligned
    # without the filter gradient there are no partial sums to keep
    assert hip_lib.dmcf_cconv_scatter_backward_workspace_bytes(ctypes.byref(a), ctypes.byref(_bwd(gw=None))) < need
    assert hip_lib.dmcf_cconv_scatter_backward_workspace_bytes(None, ctypes.byref(b)) == 0


def test_workspace_is_monotone_in_n_inp(hip_lib):
    b = _bwd()
    sizes = [hip_lib.dmcf_cconv_scatter_backward_workspace_bytes(ctypes.byref(_fwd(n_inp=n)), ctypes.byref(b))
             for n in (1, 15, 16, 17, 1000, 16384, 16385, 10 ** 5, 10 ** 6, 10 ** 7)]
    assert sizes == sorted(sizes) and sizes[-1] > sizes[0]
    # the number of partial sums is capped: the size does not grow with the scene beyond that
    assert sizes[-1] == sizes[-2] <= 1024 * 24 * 64 * 4 * 4 + 512


def test_ops_refuses_unknown_keywords():
    """A misspelt option must not be dropped: the gradient would be that of another convolution (raised at call binding)."""
    torch = pytest.importorskip("torch")
    from dmcf_amd import ops
    W, Q, P, F = torch.zeros(4, 4, 4, 3, 4), torch.zeros(5, 3), torch.zeros(7, 3), torch.zeros(7, 3)
    idx, rs = torch.zeros(9, dtype=torch.int32), torch.zeros(8, dtype=torch.int64)
    with pytest.raises(TypeError):
        ops.cconv_scatter_backward(W, Q, 0.8, P, F, idx, rs, None, torch.zeros(5, 4), windw="poly6")
