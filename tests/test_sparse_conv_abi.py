"""CPU checks of the voxel-convolution ABI (include/dmcf_hip.h, ABI 2.18): symbols, struct layout, host-side validation -- every
refusal comes before anything is enqueued, so none of this needs a GPU."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = -1, -4
LINF, IGNORE, CORNERS, WALK = 8, 1, 2, 4


@pytest.fixture(scope="module")
def hip_lib():
    from dmcf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def _args(**kw):
    from dmcf_amd._lib import SparseConvArgs
    a = SparseConvArgs()
    a.struct_size = ctypes.sizeof(SparseConvArgs)
    for k in range(5):
        a.filter_dims[k] = (3, 3, 3, 8, 16)[k]
    a.extent = 1.0
    a.filters = 256  # (never dereferenced on the host)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_symbols_and_version(hip_lib):
    for name in ("dmcf_sparse_conv_forward", "dmcf_sparse_conv_backward", "dmcf_sparse_conv_backward_workspace_bytes",
                 "dmcf_sparse_conv_kernel_names"):
        assert hasattr(hip_lib, name), name
    assert hip_lib.dmcf_version() >= 21800


def test_struct_matches_header():
    from dmcf_amd._lib import SparseConvArgs
    text = open(os.path.join(ROOT, "include", "dmcf_hip.h")).read()
    body = text[text.index("typedef struct dmcf_sparse_conv_args {"):text.index("} dmcf_sparse_conv_args;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(?:const\s+)?(\w+)\s*(\*?)\s*([a-z_]+)(?:\[(\d)\])?;", body)
    assert [f[2] for f in fields] == [f[0] for f in SparseConvArgs._fields_]
    # the size the header's types give on this ABI (LP64, natural alignment)
    sizes = {"uint32_t": 4, "int32_t": 4, "int64_t": 8, "float": 4}
    off = 0
    for typ, ptr, _, n in fields:
        sz = 8 if ptr else sizes[typ]
        off = (off + sz - 1) // sz * sz + sz * (int(n) if n else 1)
    assert (off + 7) // 8 * 8 == ctypes.sizeof(SparseConvArgs) == 152
    assert "#define DMCF_FRS_METRIC_LINF 8" in text


def test_forward_refuses_bad_arguments(hip_lib):
    f = hip_lib.dmcf_sparse_conv_forward
    assert f(None, None) == EINVAL
    a = _args()
    a.struct_size -= 8
    assert f(ctypes.byref(a), None) == EINVAL  # short struct
    assert f(ctypes.byref(_args(flags=8)), None) == EINVAL  # unknown flag
    assert f(ctypes.byref(_args(extent=0.0)), None) == EINVAL
    assert f(ctypes.byref(_args(filters=None)), None) == EINVAL
    assert f(ctypes.byref(_args(n_rows=-1)), None) == EINVAL
    assert f(ctypes.byref(_args(n_rows=4)), None) == EINVAL  # rows without positions, splits, output
    assert f(ctypes.byref(_args(n_rows=4, row_positions=256, neighbors_row_splits=256, out=256, n_pairs=3)), None) == EINVAL  # pairs without a list
    a = _args()
    a.filter_dims[3] = 0
    assert f(ctypes.byref(a), None) == EINVAL
    assert f(ctypes.byref(_args()), None) == 0  # no rows: nothing to do


def test_backward_refuses_bad_arguments(hip_lib):
    b = hip_lib.dmcf_sparse_conv_backward
    assert b(None, None, None, None, 0, None, None, None, 0, None) == EINVAL
    a = _args()
    assert b(ctypes.byref(a), None, None, None, 0, None, None, None, 0, None) == EINVAL  # no gradient wanted
    a = _args(n_rows=4, row_positions=256, neighbors_row_splits=256)
    assert b(ctypes.byref(a), None, None, None, 0, 256, None, None, 0, None) == EINVAL  # rows without grad_out
    a = _args(n_rows=4, n_cols=4, row_positions=256, neighbors_row_splits=256)
    assert b(ctypes.byref(a), 256, None, None, 0, None, 256, None, 0, None) == EINVAL  # feature gradient without the inverted list
    # pairs need the column positions (the rows of the feature gradient's launch); without pairs that gradient is a memset
    a = _args(n_rows=4, n_cols=4, n_pairs=8, row_positions=256, col_features=256, neighbors_index=256, neighbors_row_splits=256)
    assert b(ctypes.byref(a), 256, 256, 256, 8, None, 256, None, 0, None) == EINVAL
    a = _args(n_rows=4, n_cols=4, n_pairs=8, row_positions=256, col_positions=256, col_features=256, neighbors_index=256,
              neighbors_row_splits=256)
    need = hip_lib.dmcf_sparse_conv_backward_workspace_bytes(ctypes.byref(a), 1)
    assert need >= 3 * 8 * 4 + 27 * 8 * 16 * 4
    assert hip_lib.dmcf_sparse_conv_backward_workspace_bytes(ctypes.byref(a), 0) == 0
    assert b(ctypes.byref(a), 256, None, None, 0, 256, None, None, 0, None) == -2  # DMCF_EWORKSPACE
    assert hip_lib.dmcf_sparse_conv_backward_workspace_bytes(None, 1) == 0
    name = ctypes.create_string_buffer(128)
    assert hip_lib.dmcf_sparse_conv_kernel_names(ctypes.byref(a), 0, name, 128) == 0 and name.value == b"sparse_conv_kernel"
    assert hip_lib.dmcf_sparse_conv_kernel_names(ctypes.byref(a), 3, name, 128) == 0 and name.value.count(b";") == 3
    assert hip_lib.dmcf_sparse_conv_kernel_names(ctypes.byref(a), 3, name, 8) == EINVAL
    assert hip_lib.dmcf_sparse_conv_kernel_names(ctypes.byref(a), 4, name, 128) == EINVAL


def test_linf_flag_combinations(hip_lib):
    """With DMCF_FRS_METRIC_LINF: a distance output, the padded search, the window sums and the OPEN3D_* flags are
    DMCF_EUNSUPPORTED -- decided on the host, before the (fake) pointers are touched."""
    L = hip_lib
    ws, n = 256, 10
    nbytes = L.dmcf_frs_workspace_bytes(n, n)
    assert L.dmcf_frs_count(256, n, n, 0.5, LINF | WALK, ws, nbytes, 256, None) == EUNSUPPORTED
    assert L.dmcf_frs_count(256, n, n, 0.5, LINF | CORNERS, ws, nbytes, 256, None) == EUNSUPPORTED
    assert L.dmcf_frs_write(256, n, n, 0.5, LINF | WALK, ws, nbytes, 256, 256, None, 100, None) == EUNSUPPORTED
    assert L.dmcf_frs_write(256, n, n, 0.5, LINF | IGNORE, ws, nbytes, 256, 256, 256, 100, None) == EUNSUPPORTED  # distances
    assert L.dmcf_frs_search_padded(256, n, n, 0.5, LINF, ws, nbytes, 8, 256, 256, 256, None, 256, None) == EUNSUPPORTED
    assert L.dmcf_frs_window_sum(256, n, n, 0.5, LINF, 1, ws, nbytes, 256, None) == EUNSUPPORTED
    # (the window sum's gradient never knew the flag: unknown flags are DMCF_EINVAL there, which tests/test_density_grad_abi.py holds)
    assert L.dmcf_frs_window_sum_backward(256, n, n, 0.5, LINF, 1, 256, None, ws, nbytes, 256, None) == EINVAL
    assert L.dmcf_frs_count(256, n, n, 0.5, 16, ws, nbytes, 256, None) == EINVAL  # still unknown
    assert L.dmcf_frs_count(None, n, n, 0.5, LINF, ws, nbytes, 256, None) == EINVAL  # null queries
    assert L.dmcf_frs_count(256, n, n, 0.5, LINF, ws, 16, 256, None) == -2  # short workspace


def test_metrics_of_the_search_layers():
    from dmcf_amd import ops
    with pytest.raises(NotImplementedError):
        ops.FixedRadiusSearch(metric="L1")
    with pytest.raises(NotImplementedError):
        ops.FixedRadiusSearch(metric="Linf", return_distances=True)
    with pytest.raises(NotImplementedError):
        ops.RadiusSearch(metric="Linf")
    s = ops.FixedRadiusSearch(metric="Linf")
    assert s.metric == "Linf" and not s.return_distances


def test_ops_refuse_cpu_tensors_and_offsets(hip_lib):
    import torch
    from dmcf_amd import ops, _lib
    W, P, F = torch.zeros(3, 3, 3, 2, 2), torch.zeros(4, 3), torch.zeros(4, 2)
    idx, rs = torch.zeros(4, dtype=torch.int32), torch.arange(5, dtype=torch.int64)
    with pytest.raises(_lib.DmcfError):
        ops.sparse_conv(W, P, 1.0, [0, 0, 0], P, F, idx, rs)
    with pytest.raises(_lib.DmcfError):
        ops.sparse_conv_transpose(W, P, 1.0, [0, 0, 0], P, F, idx, rs, idx, rs)
    with pytest.raises(_lib.DmcfError):
        ops.fixed_radius_search(P, P, 0.5, return_distances=False, metric="Linf")
    with pytest.raises(NotImplementedError):  # a non-zero offset stays out of ContinuousConv's operator
        ops.continuous_conv(W, P, 1.0, torch.full((3,), -0.5), P, F, None, idx, rs, None)


def test_layers_are_exported_and_check_voxel_size():
    import torch
    from dmcf_amd.utils import convolutions as cv
    assert {"SparseConv", "SparseConvTranspose"} <= set(cv.__all__)
    for cls in (cv.SparseConv, cv.SparseConvTranspose):
        layer = cls(filters=4, kernel_size=[4, 4, 4], device="cpu")
        assert layer.offset.tolist() == [-0.5, -0.5, -0.5] and cls(4, [3, 3, 3]).offset.tolist() == [0, 0, 0]
        layer.build(3, "cpu")
        assert tuple(layer.kernel.shape) == (4, 4, 4, 3, 4) and not layer.kernel.requires_grad and not layer.bias.requires_grad
        with pytest.raises(ValueError):
            layer(torch.zeros(2, 3), torch.zeros(2, 3), torch.zeros(2, 3), torch.ones(2))


def test_ops_validate_the_bias_before_any_launch(hip_lib, monkeypatch):
    """A CPU bias raises DmcfError, and a bias of the wrong length or rank raises ValueError, before the library is entered (its
    entry point is replaced by one that fails the test)."""
    import torch
    from dmcf_amd import ops, _lib
    with pytest.raises(_lib.DmcfError):
        ops._sparse_bias(torch.zeros(4), 4, torch.device("cuda:0"))
    # the shape checks, and the public calls, with the "is on the GPU" check of the operands taken out
    monkeypatch.setattr(ops, "_dev_f32", lambda t, name, cols=None: t)
    monkeypatch.setattr(hip_lib, "dmcf_sparse_conv_forward", lambda *a: pytest.fail("launched"), raising=False)
    dev = torch.device("cpu")
    for bad in (torch.zeros(3), torch.zeros(5), torch.zeros(1, 4), torch.zeros(())):
        with pytest.raises(ValueError):
            ops._sparse_bias(bad, 4, dev)
    assert ops._sparse_bias(None, 4, dev) is None and ops._sparse_bias(torch.zeros(4), 4, dev).shape == (4,)
    W, P, F = torch.zeros(3, 3, 3, 2, 4), torch.zeros(4, 3), torch.zeros(4, 2)
    idx, rs = torch.zeros(4, dtype=torch.int32), torch.arange(5, dtype=torch.int64)
    for fn, lists in ((ops.sparse_conv, (idx, rs)), (ops.sparse_conv_transpose, (idx, rs, idx, rs))):
        with pytest.raises(ValueError, match="bias"):
            fn(W, P, 1.0, [0, 0, 0], P, F, *lists, bias=torch.zeros(5))
        with pytest.raises(ValueError, match="bias"):  # the recording path
            fn(W.clone().requires_grad_(True), P, 1.0, [0, 0, 0], P, F, *lists, bias=torch.zeros(2, 4))
    with pytest.raises(ValueError, match="bias"):
        ops._sparse_args(W, P, P, F, idx, rs, 1.0, [0.0, 0.0, 0.0], 0, bias=torch.zeros(3))
    with pytest.raises(ValueError, match="bias"):  # with the channels transposed the output has Cin channels
        ops._sparse_args(W, P, P, torch.zeros(4, 4), idx, rs, 1.0, [0.0, 0.0, 0.0], ops.SPARSE_W_TRANSPOSED, bias=torch.zeros(4))
