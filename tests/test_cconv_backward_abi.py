"""CPU checks of the backward entry points (dmcf_invert_neighbors_list, dmcf_cconv_backward): symbols, the ctypes mirror of
dmcf_cconv_backward_args, host-side validation and the kernel-name diagnostic.  No device is touched."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["dmcf_invert_neighbors_list_workspace_bytes", "dmcf_invert_neighbors_list", "dmcf_cconv_backward_workspace_bytes",
       "dmcf_cconv_backward", "dmcf_cconv_backward_kernel_names"]
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
    assert hip_lib.dmcf_version() >= 20800


def test_backward_struct_mirrors_header():
    from dmcf_amd._lib import CconvBackwardArgs
    text = open(os.path.join(ROOT, "include", "dmcf_hip.h")).read()
    body = text[text.index("typedef struct dmcf_cconv_backward_args {"):text.index("} dmcf_cconv_backward_args;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"^\s*(?:const\s+)?([a-z0-9_]+\*?)\s+(\*?)([a-z_]+);", body, flags=re.M)
    names = [f[2] for f in fields]
    assert names == [f[0] for f in CconvBackwardArgs._fields_]
    ctypes_of = {"uint32_t": ctypes.c_uint32, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64}
    for (typ, star, name), (cname, ctyp) in zip(fields, CconvBackwardArgs._fields_):
        if typ.endswith("*") or star:
            assert ctyp is ctypes.c_void_p, name
        else:
            assert ctyp is ctypes_of[typ], name
    assert CconvBackwardArgs.struct_size.offset == 0
    assert ctypes.sizeof(CconvBackwardArgs) == 72


def _fwd(n_out=16, n_inp=16, flags=0, dims=(4, 4, 4, 3, 5)):
    from dmcf_amd._lib import CconvArgs
    a = CconvArgs()
    a.filters = FAKE
    for d in range(5):
        a.filter_dims[d] = dims[d]
    a.sym_axis = 2
    a.out_positions = a.inp_positions = a.inp_features = FAKE
    a.n_out, a.n_inp = n_out, n_inp
    a.neighbors_index = a.neighbors_row_splits = FAKE
    a.extent = 0.2
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


def test_backward_host_validation(hip_lib):
    L = hip_lib
    ws = ctypes.c_void_p(FAKE)
    a = _fwd()

    def call(b, args=a):
        return L.dmcf_cconv_backward(ctypes.byref(args), ctypes.byref(b), None, 0, None)

    assert call(_bwd(grad_out=None)) == EINVAL                                       # NULL grad_out
    assert call(_bwd(struct_size=ctypes.sizeof(_bwd()) - 8)) == EINVAL               # short struct
    assert call(_bwd(struct_size=0)) == EINVAL
    assert call(_bwd(inv_n_rows=17)) == EINVAL                                       # list of another point set
    assert call(_bwd(inv_row_splits=None)) == EINVAL                                 # no inverted list
    assert call(_bwd(inv_n_pairs=-1)) == EINVAL
    assert call(_bwd(flags=2)) == EINVAL                                             # unknown flag
    assert L.dmcf_cconv_backward(None, ctypes.byref(_bwd()), ws, 1 << 20, None) == EINVAL
    assert L.dmcf_cconv_backward(ctypes.byref(a), None, ws, 1 << 20, None) == EINVAL
    bad = _fwd()
    bad.extent = 0.0
    assert call(_bwd(), bad) == EINVAL
    # the inverted list is needed only for the input-feature gradient
    b = _bwd(inv_row_splits=None, inv_index=None, inv_pair=None, grad_inp_features=None)
    assert L.dmcf_cconv_backward_workspace_bytes(ctypes.byref(a), ctypes.byref(b)) > 256
    assert call(b) == EINVAL  # (valid arguments, NULL workspace)
    # ASCC on the sharded layout (ghost inputs after the owned points)
    assert call(_bwd(inv_n_rows=20), _fwd(n_out=16, n_inp=20, flags=4, dims=(4, 4, 2, 3, 5))) == EUNSUPPORTED
    # a full kernel too large for one wave's LDS
    assert call(_bwd(), _fwd(dims=(8, 8, 8, 64, 64))) == EUNSUPPORTED


def test_invert_host_validation(hip_lib):
    L = hip_lib
    f = ctypes.c_void_p(FAKE)
    nb = L.dmcf_invert_neighbors_list_workspace_bytes(0)
    assert nb >= 256
    assert L.dmcf_invert_neighbors_list(-1, f, f, None, 4, 10, None, f, f, f, None, f, 1 << 30, None) == EINVAL
    assert L.dmcf_invert_neighbors_list(4, f, f, None, 4, 10, None, f, None, f, None, f, 1 << 30, None) == EINVAL  # no row splits
    assert L.dmcf_invert_neighbors_list(4, None, f, None, 4, 10, None, f, f, f, None, f, 1 << 30, None) == EINVAL  # no index
    assert L.dmcf_invert_neighbors_list(4, f, f, None, 4, 10, None, f, f, f, f, f, 1 << 30, None) == EINVAL  # attributes out, none in


def test_backward_kernel_names(hip_lib):
    L = hip_lib
    name = ctypes.create_string_buffer(256)
    assert L.dmcf_cconv_backward_kernel_names(ctypes.byref(_fwd()), ctypes.byref(_bwd()), name, 256) == 0
    assert name.value.decode().split(";") == ["cconv_bwd_input", "cconv_bwd_filter_splat", "cconv_bwd_filter_gemm",
                                              "cconv_bwd_filter_reduce", "cconv_bwd_filter_store"]
    a = _fwd(flags=4 | 2, dims=(4, 4, 2, 3, 5))
    assert L.dmcf_cconv_backward_kernel_names(ctypes.byref(a), ctypes.byref(_bwd(grad_filters=None)), name, 256) == 0
    assert name.value.decode() == "cconv_bwd_norm;cconv_bwd_expand;cconv_bwd_input"
    assert L.dmcf_cconv_backward_kernel_names(ctypes.byref(_fwd()), ctypes.byref(_bwd(grad_out=None)), name, 256) == EINVAL


def test_ops_surface_errors_before_launch():
    torch = pytest.importorskip("torch")
    from dmcf_amd import ops
    # the autograd path refuses what it cannot record, before any launch
    W = torch.zeros(4, 4, 4, 3, 5, requires_grad=True)
    P = torch.zeros(10, 3)
    F = torch.zeros(10, 3)
    idx = torch.zeros(0, dtype=torch.int32)
    rs = torch.zeros(11, dtype=torch.int64)
    with pytest.raises(ValueError):
        ops.cconv_forward(W, P, 0.2, P, F, idx, rs, out=torch.zeros(10, 5))
    with pytest.raises(NotImplementedError):
        ops.cconv_forward(W, P, torch.full((10,), 0.2), P, F, idx, rs)


PLAN_SHAPES = [
    # (n_out, full dims, Cin, Cout, symmetric)
    (600, (4, 4, 4), 5, 7, False),         # one chunk
    (38836, (6, 6, 6), 32, 16, True),      # exactly R = 2^28 / 6912 rows
    (38837, (6, 6, 6), 32, 16, True),      # R + 1: a second chunk of one row
    (45000, (6, 6, 6), 32, 16, True),      # the shipped ASCC layer, two chunks
    (40000, (4, 4, 4), 256, 4, False),     # three chunks of R = 16384
    (70000, (4, 4, 4), 3, 5, False),       # the slab cap: S = 256, 274 rows per slab
    (1, (1, 8, 1), 1, 1, False),
]


@pytest.mark.parametrize("n_out,dims,cin,cout,sym", PLAN_SHAPES)
def test_plan_geometry_matches_workspace(hip_lib, n_out, dims, cin, cout, sym):
    """cconv_backward_ref.bwd_plan / bwd_workspace_bytes (what the GPU tests rely on to know the path a case takes) against
    dmcf_cconv_backward_workspace_bytes, for each combination of the wanted gradients."""
    import cconv_backward_ref as ref
    K = dims[0] * dims[1] * dims[2]
    stored = list(dims)
    if sym:
        stored[2] //= 2
    pl = ref.bwd_plan(n_out, K, cin, cout)
    for want_f in (True, False):
        for want_w in (True, False):
            a = _fwd(n_out=n_out, n_inp=n_out, flags=4 if sym else 0, dims=(*stored, cin, cout))
            b = _bwd(n_inp=n_out, grad_filters=FAKE if want_w else None, grad_inp_features=FAKE if want_f else None)
            got = hip_lib.dmcf_cconv_backward_workspace_bytes(ctypes.byref(a), ctypes.byref(b))
            assert got == ref.bwd_workspace_bytes(n_out, K, cin, cout, sym, want_f, want_w), (want_f, want_w)
    R = ref.BWD_CHUNK_FLOATS // (K * cin)
    assert pl["R"] == min(n_out, R)
    if n_out == R:
        assert len(pl["chunks"]) == 1
    if n_out == R + 1:
        assert len(pl["chunks"]) == 2 and pl["chunks"][-1][1] == 1
    if n_out == 70000:
        assert pl["S"] == ref.BWD_MAX_SLABS and pl["rows_per_slab"] == 274 and len(pl["chunks"]) == 1


@pytest.mark.parametrize("dims,cin,cout,ok", [
    ((4, 4, 4), 256, 3, True), ((4, 4, 4), 3, 256, True), ((4, 4, 4), 257, 3, False), ((4, 4, 4), 3, 257, False),
    ((1, 8, 8), 256, 256, True), ((1, 8, 8), 257, 1, False), ((6, 6, 3), 75, 75, True), ((6, 6, 3), 76, 1, False),
])
def test_lds_limit(hip_lib, dims, cin, cout, ok):
    """K * Cin and K * Cout up to 16384 are accepted; one channel more returns DMCF_EUNSUPPORTED (ASCC: K of the full kernel)."""
    import cconv_backward_ref as ref
    sym = dims == (6, 6, 3)
    K = dims[0] * dims[1] * dims[2] * (2 if sym else 1)
    assert ref.bwd_supported(K, cin, cout) == ok
    a = _fwd(flags=4 if sym else 0, dims=(*dims, cin, cout))
    rc = hip_lib.dmcf_cconv_backward(ctypes.byref(a), ctypes.byref(_bwd()), None, 0, None)
    assert rc == (EINVAL if ok else EUNSUPPORTED)  # (valid arguments stop at the NULL workspace)
    assert (hip_lib.dmcf_cconv_backward_workspace_bytes(ctypes.byref(a), ctypes.byref(_bwd())) > 256) == ok
