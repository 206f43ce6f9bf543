"""ctypes binding of libdmcf_hip.so (the C ABI declared in include/dmcf_hip.h).

The product path has NO fallback: if the HIP library is missing or a call fails, this raises.
"""
import ctypes
import os
import subprocess

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "libdmcf_hip.so")
_lib = None


class DmcfError(RuntimeError):
    pass


class CconvArgs(ctypes.Structure):
    """struct dmcf_cconv_args (include/dmcf_hip.h)."""
    _fields_ = [
        ("filters", ctypes.c_void_p),
        ("filter_dims", ctypes.c_int32 * 5),
        ("sym_axis", ctypes.c_int32),
        ("out_positions", ctypes.c_void_p),
        ("n_out", ctypes.c_int64),
        ("inp_positions", ctypes.c_void_p),
        ("n_inp", ctypes.c_int64),
        ("inp_features", ctypes.c_void_p),
        ("inp_importance", ctypes.c_void_p),
        ("neighbors_index", ctypes.c_void_p),
        ("neighbors_row_splits", ctypes.c_void_p),
        ("neighbors_value", ctypes.c_void_p),
        ("extent", ctypes.c_float),
        ("window_fac", ctypes.c_float),
        ("window", ctypes.c_int32),
        ("coordinate_mapping", ctypes.c_int32),
        ("interpolation", ctypes.c_int32),
        ("flags", ctypes.c_int32),
        ("bias", ctypes.c_void_p),
        ("out", ctypes.c_void_p),
        ("n_pairs", ctypes.c_int64),
        ("neighbors_row_count", ctypes.c_void_p),
        ("filter_tile_mask", ctypes.c_uint32),
        ("row_length_hint", ctypes.c_int32),
    ]


class CconvBackwardArgs(ctypes.Structure):
    """struct dmcf_cconv_backward_args (include/dmcf_hip.h)."""
    _fields_ = [
        ("struct_size", ctypes.c_uint32),
        ("flags", ctypes.c_int32),
        ("grad_out", ctypes.c_void_p),
        ("inv_index", ctypes.c_void_p),
        ("inv_pair", ctypes.c_void_p),
        ("inv_row_splits", ctypes.c_void_p),
        ("inv_n_rows", ctypes.c_int64),
        ("inv_n_pairs", ctypes.c_int64),
        ("grad_filters", ctypes.c_void_p),
        ("grad_inp_features", ctypes.c_void_p),
    ]


class NeighborDenseArgs(ctypes.Structure):
    """struct dmcf_neighbor_dense_args (include/dmcf_hip.h)."""
    _fields_ = [
        ("struct_size", ctypes.c_uint32),
        ("flags", ctypes.c_int32),
        ("x", ctypes.c_void_p),
        ("n_in", ctypes.c_int64),
        ("cin", ctypes.c_int32),
        ("cout", ctypes.c_int32),
        ("kernel", ctypes.c_void_p),
        ("bias", ctypes.c_void_p),
        ("residual", ctypes.c_void_p),
        ("mask", ctypes.c_void_p),
        ("neighbors_index", ctypes.c_void_p),
        ("neighbors_row_splits", ctypes.c_void_p),
        ("neighbors_row_count", ctypes.c_void_p),
        ("n_out", ctypes.c_int64),
        ("n_pairs", ctypes.c_int64),
        ("host_row_splits", ctypes.c_void_p),
        ("out", ctypes.c_void_p),
        ("record_s", ctypes.c_void_p),
        ("record_count", ctypes.c_void_p),
    ]


class NeighborDenseBackwardArgs(ctypes.Structure):
    """struct dmcf_neighbor_dense_backward_args (include/dmcf_hip.h)."""
    _fields_ = [
        ("struct_size", ctypes.c_uint32),
        ("flags", ctypes.c_int32),
        ("x", ctypes.c_void_p),
        ("n_in", ctypes.c_int64),
        ("cin", ctypes.c_int32),
        ("cout", ctypes.c_int32),
        ("kernel", ctypes.c_void_p),
        ("grad_out", ctypes.c_void_p),
        ("n_out", ctypes.c_int64),
        ("s", ctypes.c_void_p),
        ("count", ctypes.c_void_p),
        ("inv_index", ctypes.c_void_p),
        ("inv_row_splits", ctypes.c_void_p),
        ("inv_n_pairs", ctypes.c_int64),
        ("grad_x", ctypes.c_void_p),
        ("grad_kernel", ctypes.c_void_p),
        ("grad_bias", ctypes.c_void_p),
    ]


class LatticeConvArgs(ctypes.Structure):
    """struct dmcf_lattice_conv_args (include/dmcf_hip.h)."""
    _fields_ = [
        ("filters", ctypes.c_void_p),
        ("filter_dims", ctypes.c_int32 * 5),
        ("inp_volume", ctypes.c_void_p),
        ("inp_min", ctypes.c_int32 * 3),
        ("inp_dims", ctypes.c_int32 * 3),
        ("out_table", ctypes.c_void_p),
        ("out_min", ctypes.c_int32 * 3),
        ("out_dims", ctypes.c_int32 * 3),
        ("n_out", ctypes.c_int64),
        ("inp_step", ctypes.c_int32),
        ("out_stride", ctypes.c_int32),
        ("out_phase", ctypes.c_int32 * 3),
        ("base_min", ctypes.c_int32 * 3),
        ("base_dims", ctypes.c_int32 * 3),
        ("rel_shift", ctypes.c_float * 3),
        ("voxel", ctypes.c_float * 3),
        ("offsets", ctypes.c_void_p),
        ("n_offsets", ctypes.c_int64),
        ("reach", ctypes.c_int32 * 3),
        ("extent", ctypes.c_float),
        ("window_fac", ctypes.c_float),
        ("window", ctypes.c_int32),
        ("coordinate_mapping", ctypes.c_int32),
        ("interpolation", ctypes.c_int32),
        ("flags", ctypes.c_int32),
        ("bias", ctypes.c_void_p),
        ("out", ctypes.c_void_p),
    ]


class CconvScatterArgs(ctypes.Structure):
    """struct dmcf_cconv_scatter_args (include/dmcf_hip.h)."""
    _fields_ = [
        ("filters", ctypes.c_void_p),
        ("filter_dims", ctypes.c_int32 * 5),
        ("out_positions", ctypes.c_void_p),
        ("n_out", ctypes.c_int64),
        ("inp_positions", ctypes.c_void_p),
        ("n_inp", ctypes.c_int64),
        ("inp_features", ctypes.c_void_p),
        ("t_index", ctypes.c_void_p),
        ("t_row_begin", ctypes.c_void_p),
        ("t_row_count", ctypes.c_void_p),
        ("t_capacity", ctypes.c_int64),
        ("plan", ctypes.c_void_p),
        ("block_cells", ctypes.c_int32),
        ("reach", ctypes.c_int32),
        ("extent", ctypes.c_float),
        ("window_fac", ctypes.c_float),
        ("window", ctypes.c_int32),
        ("flags", ctypes.c_int32),
        ("bias", ctypes.c_void_p),
        ("out", ctypes.c_void_p),
        ("error_flag", ctypes.c_void_p),
    ]


class CconvScatterBackwardArgs(ctypes.Structure):
    """struct dmcf_cconv_scatter_backward_args (include/dmcf_hip.h)."""
    _fields_ = [
        ("struct_size", ctypes.c_uint32),
        ("flags", ctypes.c_int32),
        ("grad_out", ctypes.c_void_p),
        ("grad_filters", ctypes.c_void_p),
        ("grad_inp_features", ctypes.c_void_p),
    ]


class SparseConvArgs(ctypes.Structure):
    """struct dmcf_sparse_conv_args (include/dmcf_hip.h)."""
    _fields_ = [
        ("struct_size", ctypes.c_uint32),
        ("flags", ctypes.c_int32),
        ("filters", ctypes.c_void_p),
        ("filter_dims", ctypes.c_int32 * 5),
        ("reserved", ctypes.c_int32),
        ("row_positions", ctypes.c_void_p),
        ("n_rows", ctypes.c_int64),
        ("col_positions", ctypes.c_void_p),
        ("n_cols", ctypes.c_int64),
        ("col_features", ctypes.c_void_p),
        ("row_scale", ctypes.c_void_p),
        ("col_scale", ctypes.c_void_p),
        ("neighbors_index", ctypes.c_void_p),
        ("neighbors_row_splits", ctypes.c_void_p),
        ("n_pairs", ctypes.c_int64),
        ("extent", ctypes.c_float),
        ("offset", ctypes.c_float * 3),
        ("bias", ctypes.c_void_p),
        ("out", ctypes.c_void_p),
    ]


class HistPlan(ctypes.Structure):
    """struct dmcf_hist_plan (include/dmcf_hip.h)."""
    _fields_ = [
        ("per", ctypes.c_int32),
        ("rank", ctypes.c_int32 * 4),
        ("gamma", ctypes.c_float * 2),
        ("reserved", ctypes.c_int32),
    ]


class AdamTensor(ctypes.Structure):
    """struct dmcf_adam_tensor (include/dmcf_hip.h)."""
    _fields_ = [
        ("param", ctypes.c_void_p),
        ("grad", ctypes.c_void_p),
        ("m", ctypes.c_void_p),
        ("v", ctypes.c_void_p),
        ("n", ctypes.c_int64),
    ]


class AdamArgs(ctypes.Structure):
    """struct dmcf_adam_args (include/dmcf_hip.h)."""
    _fields_ = [
        ("struct_size", ctypes.c_uint32),
        ("n_tensors", ctypes.c_int32),
        ("tensors", ctypes.c_void_p),
        ("device_tensors", ctypes.c_void_p),
        ("lr", ctypes.c_float),
        ("beta_1", ctypes.c_float),
        ("beta_2", ctypes.c_float),
        ("epsilon", ctypes.c_float),
        ("beta_1_power", ctypes.c_float),
        ("beta_2_power", ctypes.c_float),
        ("clip_norm", ctypes.c_float),
        ("reserved", ctypes.c_int32),
    ]


class Sph1dParams(ctypes.Structure):
    """struct dmcf_sph1d_params (include/dmcf_hip.h)."""
    _fields_ = [
        ("struct_size", ctypes.c_uint32),
        ("bcnt", ctypes.c_int32),
        ("max_iter", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
        ("h", ctypes.c_double),
        ("rest_dens", ctypes.c_double),
        ("stiffness", ctypes.c_double),
        ("visc", ctypes.c_double),
        ("gravity", ctypes.c_double),
        ("dt", ctypes.c_double),
        ("eps", ctypes.c_double),
    ]


class Camera(ctypes.Structure):
    """struct dmcf_camera (include/dmcf_hip.h): 80 bytes."""
    _fields_ = [
        ("view", ctypes.c_float * 12),
        ("focal", ctypes.c_float),
        ("cx", ctypes.c_float),
        ("cy", ctypes.c_float),
        ("near", ctypes.c_float),
        ("orthographic", ctypes.c_int32),
        ("reserved", ctypes.c_int32 * 3),
    ]


class SplatLayer(ctypes.Structure):
    """struct dmcf_splat_layer (include/dmcf_hip.h): 48 bytes."""
    _fields_ = [
        ("keys", ctypes.c_void_p),
        ("xyz", ctypes.c_void_p),
        ("n_points", ctypes.c_int64),
        ("frame_stride", ctypes.c_int64),
        ("radius", ctypes.c_float),
        ("color_argb", ctypes.c_uint32),
        ("flags", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
    ]


SPLAT_FARTHEST = 1    # DMCF_SPLAT_FARTHEST
SPLAT_MAX_LAYERS = 4  # DMCF_SPLAT_MAX_LAYERS


# names every entry point include/dmcf_hip.h declares (tests/test_abi.py cross-checks against the header)
SYMBOLS = [
    "dmcf_version", "dmcf_error_string", "dmcf_last_hip_error",
    "dmcf_frs_workspace_bytes", "dmcf_frs_build", "dmcf_frs_count", "dmcf_frs_write", "dmcf_frs_search_padded", "dmcf_frs_window_sum",
    "dmcf_radius_search_count", "dmcf_radius_search_write",
    "dmcf_cconv_workspace_bytes", "dmcf_cconv_forward", "dmcf_cconv_kernel_name",
    "dmcf_cconv_forward_extents", "dmcf_cconv_extents_kernel_name",
    "dmcf_invert_neighbors_list_workspace_bytes", "dmcf_invert_neighbors_list",
    "dmcf_cconv_backward_workspace_bytes", "dmcf_cconv_backward", "dmcf_cconv_backward_kernel_names",
    "dmcf_cconv_backward_extents", "dmcf_cconv_backward_extents_kernel_names",
    "dmcf_cconv_scatter_plan_bytes", "dmcf_cconv_scatter_plan", "dmcf_cconv_scatter_workspace_bytes", "dmcf_cconv_scatter_forward",
    "dmcf_cconv_scatter_backward_workspace_bytes", "dmcf_cconv_scatter_backward",
    "dmcf_lattice_conv_workspace_bytes", "dmcf_lattice_conv_forward",
    "dmcf_lattice_conv_batch_workspace_bytes", "dmcf_lattice_conv_forward_batch",
    "dmcf_lattice_conv_backward_workspace_bytes", "dmcf_lattice_conv_backward",
    "dmcf_reduce_subarrays_sum", "dmcf_points_aabb_workspace_bytes", "dmcf_points_aabb", "dmcf_dense_forward",
    "dmcf_fps_workspace_bytes", "dmcf_farthest_point_sample", "dmcf_gather_point",
    "dmcf_grid_pos_workspace_bytes", "dmcf_grid_pos_bounds", "dmcf_grid_pos_count", "dmcf_grid_pos_write",
    "dmcf_ghost_workspace_bytes", "dmcf_ghost_count", "dmcf_ghost_write",
    "dmcf_nn_distance_workspace_bytes", "dmcf_nn_distance", "dmcf_approx_match_workspace_bytes", "dmcf_approx_match",
    "dmcf_match_cost_workspace_bytes", "dmcf_match_cost", "dmcf_emd_workspace_bytes", "dmcf_emd",
    "dmcf_neighbor_dense_forward", "dmcf_neighbor_dense_backward_workspace_bytes", "dmcf_neighbor_dense_backward",
    "dmcf_neighbor_dense_kernel_names", "dmcf_adam_step_workspace_bytes", "dmcf_adam_step", "dmcf_adam_step_kernel_names",
    "dmcf_raster_workspace_bytes", "dmcf_raster_count", "dmcf_raster_discs",
    "dmcf_nn_distance_backward_workspace_bytes", "dmcf_nn_distance_backward", "dmcf_match_cost_backward_workspace_bytes",
    "dmcf_match_cost_backward", "dmcf_emd_with_levels", "dmcf_emd_backward_workspace_bytes", "dmcf_emd_backward",
    "dmcf_gather_point_backward_workspace_bytes", "dmcf_gather_point_backward",
    "dmcf_frs_window_sum_backward",
    "dmcf_sph1d_rollout",
    "dmcf_sparse_conv_forward", "dmcf_sparse_conv_backward_workspace_bytes", "dmcf_sparse_conv_backward",
    "dmcf_sparse_conv_kernel_names",
    "dmcf_frs_workspace_bytes_batched", "dmcf_frs_build_batched", "dmcf_frs_count_batched", "dmcf_frs_write_batched",
    "dmcf_radius_search_count_batched", "dmcf_radius_search_write_batched",
    "dmcf_grid_pos_workspace_bytes_batched", "dmcf_grid_pos_bounds_batched", "dmcf_grid_pos_count_batched",
    "dmcf_grid_pos_write_batched", "dmcf_points_aabb_batched",
    "dmcf_frs_window_sum_batched", "dmcf_frs_window_sum_backward_batched",
    "dmcf_nn_distance_ragged_workspace_bytes", "dmcf_nn_distance_ragged",
    "dmcf_emd_ragged_workspace_bytes", "dmcf_emd_ragged",
    "dmcf_emd_ragged_with_levels", "dmcf_emd_ragged_backward_workspace_bytes", "dmcf_emd_ragged_backward",
    "dmcf_hist_pair_ragged_workspace_bytes", "dmcf_hist_pair_ragged",
    "dmcf_splat_depth", "dmcf_splat_shade",
]


def build(force=False):
    """Compile dmcf_amd/csrc/*.hip for gfx950 into dmcf_amd/libdmcf_hip.so (hipcc cross-compiles without a GPU)."""
    csrc = os.path.join(_PKG, "csrc")
    args = ["make", "-C", csrc, "-j4"]
    if force:
        args.append("-B")
    subprocess.check_call(args, stdout=subprocess.DEVNULL)
    return LIB_PATH


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise DmcfError(
            f"{LIB_PATH} is missing: the HIP extension has not been built "
            "(run `python -c 'import __graft_entry__ as g; g.build()'`). There is no CPU fallback.")
    L = ctypes.CDLL(LIB_PATH)
    c = ctypes
    L.dmcf_version.restype = c.c_int
    L.dmcf_error_string.restype = c.c_char_p
    L.dmcf_error_string.argtypes = [c.c_int]
    L.dmcf_last_hip_error.restype = c.c_int
    L.dmcf_frs_workspace_bytes.restype = c.c_size_t
    L.dmcf_frs_workspace_bytes.argtypes = [c.c_int64, c.c_int64]
    L.dmcf_frs_build.restype = c.c_int
    L.dmcf_frs_build.argtypes = [c.c_void_p, c.c_int64, c.c_float, c.c_void_p, c.c_size_t, c.c_void_p]
    L.dmcf_frs_count.restype = c.c_int
    L.dmcf_frs_count.argtypes = [c.c_void_p, c.c_int64, c.c_int64, c.c_float, c.c_int, c.c_void_p, c.c_size_t,
                                 c.c_void_p, c.c_void_p]
    L.dmcf_frs_write.restype = c.c_int
    L.dmcf_frs_write.argtypes = [c.c_void_p, c.c_int64, c.c_int64, c.c_float, c.c_int, c.c_void_p, c.c_size_t,
                                 c.c_void_p, c.c_void_p, c.c_void_p, c.c_int64, c.c_void_p]
    L.dmcf_frs_search_padded.restype = c.c_int
    L.dmcf_frs_search_padded.argtypes = [c.c_void_p, c.c_int64, c.c_int64, c.c_float, c.c_int, c.c_void_p, c.c_size_t, c.c_int64,
                                         c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p]
    L.dmcf_frs_window_sum.restype = c.c_int
    L.dmcf_frs_window_sum.argtypes = [c.c_void_p, c.c_int64, c.c_int64, c.c_float, c.c_int, c.c_int, c.c_void_p, c.c_size_t,
                                      c.c_void_p, c.c_void_p]
    L.dmcf_radius_search_count.restype = c.c_int
    L.dmcf_radius_search_count.argtypes = [c.c_void_p, c.c_int64, c.c_int64, c.c_void_p, c.c_float, c.c_int, c.c_void_p, c.c_size_t,
                                           c.c_void_p, c.c_void_p]
    L.dmcf_radius_search_write.restype = c.c_int
    L.dmcf_radius_search_write.argtypes = [c.c_void_p, c.c_int64, c.c_int64, c.c_void_p, c.c_float, c.c_int, c.c_void_p, c.c_size_t,
                                           c.c_void_p, c.c_void_p, c.c_void_p, c.c_int64, c.c_void_p]
    L.dmcf_cconv_workspace_bytes.restype = c.c_size_t
    L.dmcf_cconv_workspace_bytes.argtypes = [c.POINTER(CconvArgs)]
    L.dmcf_cconv_forward.restype = c.c_int
    L.dmcf_cconv_forward.argtypes = [c.POINTER(CconvArgs), c.c_void_p, c.c_size_t, c.c_void_p]
    L.dmcf_cconv_kernel_name.restype = c.c_int
    L.dmcf_cconv_kernel_name.argtypes = [c.POINTER(CconvArgs), c.c_char_p, c.c_size_t]
    L.dmcf_cconv_forward_extents.restype = c.c_int
    L.dmcf_cconv_forward_extents.argtypes = [c.POINTER(CconvArgs), c.c_void_p, c.c_void_p, c.c_size_t, c.c_void_p]
    L.dmcf_cconv_extents_kernel_name.restype = c.c_int
    L.dmcf_cconv_extents_kernel_name.argtypes = [c.POINTER(CconvArgs), c.c_char_p, c.c_size_t]
    L.dmcf_invert_neighbors_list_workspace_bytes.restype = c.c_size_t
    L.dmcf_invert_neighbors_list_workspace_bytes.argtypes = [c.c_int64]
    L.dmcf_invert_neighbors_list.restype = c.c_int
    L.dmcf_invert_neighbors_list.argtypes = [c.c_int64, c.c_void_p, c.c_void_p, c.c_void_p, c.c_int64, c.c_int64, c.c_void_p,
                                             c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_size_t, c.c_void_p]
    L.dmcf_cconv_backward_workspace_bytes.restype = c.c_size_t
    L.dmcf_cconv_backward_workspace_bytes.argtypes = [c.POINTER(CconvArgs), c.POINTER(CconvBackwardArgs)]
    L.dmcf_cconv_backward.restype = c.c_int
    L.dmcf_cconv_backward.argtypes = [c.POINTER(CconvArgs), c.POINTER(CconvBackwardArgs), c.c_void_p, c.c_size_t, c.c_void_p]
    L.dmcf_cconv_backward_kernel_names.restype = c.c_int
    L.dmcf_cconv_backward_kernel_names.argtypes = [c.POINTER(CconvArgs), c.POINTER(CconvBackwardArgs), c.c_char_p, c.c_size_t]
    # gradients through per-point extents (ABI 2.15)
    L.dmcf_cconv_backward_extents.restype = c.c_int
    L.dmcf_cconv_backward_extents.argtypes = [c.POINTER(CconvArgs), c.POINTER(CconvBackwardArgs), c.c_void_p, c.c_void_p, c.c_size_t,
                                              c.c_void_p]
    L.dmcf_cconv_backward_extents_kernel_names.restype = c.c_int
    L.dmcf_cconv_backward_extents_kernel_names.argtypes = [c.POINTER(CconvArgs), c.POINTER(CconvBackwardArgs), c.c_char_p, c.c_size_t]
    L.dmcf_cconv_scatter_plan_bytes.restype = c.c_size_t
    L.dmcf_cconv_scatter_plan_bytes.argtypes = [c.c_int64]
    L.dmcf_cconv_scatter_plan.restype = c.c_int
    L.dmcf_cconv_scatter_plan.argtypes = [c.c_void_p, c.c_int64, c.c_void_p, c.c_int64, c.c_float, c.c_float, c.c_int32, c.c_void_p,
                                          c.c_size_t, c.c_void_p]
    L.dmcf_cconv_scatter_workspace_bytes.restype = c.c_size_t
    L.dmcf_cconv_scatter_workspace_bytes.argtypes = [c.POINTER(CconvScatterArgs)]
    L.dmcf_cconv_scatter_forward.restype = c.c_int
    L.dmcf_cconv_scatter_forward.argtypes = [c.POINTER(CconvScatterArgs), c.c_void_p, c.c_size_t, c.c_void_p]
    # the backward of the scatter form (ABI 2.19)
    L.dmcf_cconv_scatter_backward_workspace_bytes.restype = c.c_size_t
    L.dmcf_cconv_scatter_backward_workspace_bytes.argtypes = [c.POINTER(CconvScatterArgs), c.POINTER(CconvScatterBackwardArgs)]
    L.dmcf_cconv_scatter_backward.restype = c.c_int
    L.dmcf_cconv_scatter_backward.argtypes = [c.POINTER(CconvScatterArgs), c.POINTER(CconvScatterBackwardArgs), c.c_void_p, c.c_size_t,
                                              c.c_void_p]
    L.dmcf_lattice_conv_workspace_bytes.restype = c.c_size_t
    L.dmcf_lattice_conv_workspace_bytes.argtypes = [c.POINTER(LatticeConvArgs)]
    L.dmcf_lattice_conv_forward.restype = c.c_int
    L.dmcf_lattice_conv_forward.argtypes = [c.POINTER(LatticeConvArgs), c.c_void_p, c.c_size_t, c.c_void_p]
    L.dmcf_lattice_conv_batch_workspace_bytes.restype = c.c_size_t
    L.dmcf_lattice_conv_batch_workspace_bytes.argtypes = [c.POINTER(LatticeConvArgs), c.c_int32]
    L.dmcf_lattice_conv_forward_batch.restype = c.c_int
    L.dmcf_lattice_conv_forward_batch.argtypes = [c.POINTER(LatticeConvArgs), c.c_int32, c.c_void_p, c.c_size_t, c.c_void_p]
    # gradients of the lattice form (ABI 2.16)
    L.dmcf_lattice_conv_backward_workspace_bytes.restype = c.c_size_t
    L.dmcf_lattice_conv_backward_workspace_bytes.argtypes = [c.POINTER(LatticeConvArgs), c.c_int32]
    L.dmcf_lattice_conv_backward.restype = c.c_int
    L.dmcf_lattice_conv_backward.argtypes = [c.POINTER(LatticeConvArgs), c.c_int32, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p,
                                             c.c_size_t, c.c_void_p]
    L.dmcf_dense_forward.restype = c.c_int
    L.dmcf_dense_forward.argtypes = [c.c_void_p, c.c_int64, c.c_int32, c.c_void_p, c.c_int32, c.c_void_p, c.c_void_p, c.c_void_p,
                                     c.c_void_p]
    L.dmcf_ghost_workspace_bytes.restype = c.c_size_t
    L.dmcf_ghost_workspace_bytes.argtypes = [c.c_int64, c.c_int32, c.c_int32]
    L.dmcf_ghost_count.restype = c.c_int
    L.dmcf_ghost_count.argtypes = [c.c_void_p, c.c_int64, c.c_void_p, c.c_int32, c.c_void_p, c.c_int32, c.c_void_p, c.c_void_p,
                                   c.c_size_t, c.c_void_p]
    L.dmcf_ghost_write.restype = c.c_int
    L.dmcf_ghost_write.argtypes = [c.c_void_p, c.c_int64, c.c_void_p, c.c_int32, c.c_void_p, c.c_int32, c.c_void_p, c.c_void_p,
                                   c.c_void_p, c.c_void_p, c.c_size_t, c.c_void_p]
    L.dmcf_points_aabb_workspace_bytes.restype = c.c_size_t
    L.dmcf_points_aabb_workspace_bytes.argtypes = []
    L.dmcf_points_aabb.restype = c.c_int
    L.dmcf_points_aabb.argtypes = [c.c_void_p, c.c_int64, c.c_void_p, c.c_void_p, c.c_size_t, c.c_void_p]
    L.dmcf_reduce_subarrays_sum.restype = c.c_int
    L.dmcf_reduce_subarrays_sum.argtypes = [c.c_void_p, c.c_void_p, c.c_int64, c.c_void_p, c.c_void_p]
    L.dmcf_fps_workspace_bytes.restype = c.c_size_t
    L.dmcf_fps_workspace_bytes.argtypes = [c.c_int64]
    L.dmcf_farthest_point_sample.restype = c.c_int
    L.dmcf_farthest_point_sample.argtypes = [c.c_void_p, c.c_int64, c.c_int64, c.c_void_p, c.c_size_t, c.c_void_p, c.c_void_p]
    L.dmcf_gather_point.restype = c.c_int
    L.dmcf_gather_point.argtypes = [c.c_void_p, c.c_void_p, c.c_int64, c.c_int, c.c_void_p, c.c_void_p]
    L.dmcf_grid_pos_workspace_bytes.restype = c.c_size_t
    L.dmcf_grid_pos_workspace_bytes.argtypes = [c.c_int64]
    f3 = c.POINTER(c.c_float)
    L.dmcf_grid_pos_bounds.restype = c.c_int
    L.dmcf_grid_pos_bounds.argtypes = [c.c_void_p, c.c_int64, f3, c.c_int, c.c_void_p, c.c_int, c.c_float, c.c_void_p,
                                       c.c_size_t, c.c_void_p]
    L.dmcf_grid_pos_count.restype = c.c_int
    L.dmcf_grid_pos_count.argtypes = [c.c_void_p, c.c_int64, f3, c.c_int, c.c_int, c.c_float, c.c_void_p, c.c_size_t,
                                      c.c_void_p, c.c_int64, c.c_void_p]
    L.dmcf_grid_pos_write.restype = c.c_int
    L.dmcf_grid_pos_write.argtypes = [c.c_void_p, c.c_int64, f3, c.c_int, c.c_int, c.c_float, c.c_void_p, c.c_size_t,
                                      c.c_void_p, c.c_int64, c.c_void_p, c.c_int64, c.c_void_p]
    for q in ("dmcf_nn_distance_workspace_bytes", "dmcf_approx_match_workspace_bytes", "dmcf_match_cost_workspace_bytes",
              "dmcf_emd_workspace_bytes"):
        getattr(L, q).restype = c.c_size_t
        getattr(L, q).argtypes = [c.c_int64, c.c_int64, c.c_int64]
    L.dmcf_nn_distance.restype = c.c_int
    L.dmcf_nn_distance.argtypes = [c.c_void_p, c.c_void_p, c.c_int64, c.c_int64, c.c_int64, c.c_void_p, c.c_void_p, c.c_void_p,
                                   c.c_void_p, c.c_void_p, c.c_size_t, c.c_void_p]
    i32p = c.POINTER(c.c_int32)
    for f in ("dmcf_approx_match", "dmcf_emd"):
        getattr(L, f).restype = c.c_int
        getattr(L, f).argtypes = [c.c_void_p, c.c_void_p, c.c_int64, c.c_int64, c.c_int64, i32p, i32p, c.c_void_p, c.c_void_p,
                                  c.c_size_t, c.c_void_p]
    L.dmcf_match_cost.restype = c.c_int
    L.dmcf_match_cost.argtypes = [c.c_void_p, c.c_void_p, c.c_int64, c.c_int64, c.c_int64, c.c_void_p, c.c_void_p, c.c_void_p,
                                  c.c_size_t, c.c_void_p]
    L.dmcf_neighbor_dense_forward.restype = c.c_int
    L.dmcf_neighbor_dense_forward.argtypes = [c.POINTER(NeighborDenseArgs), c.c_void_p]
    L.dmcf_neighbor_dense_backward_workspace_bytes.restype = c.c_size_t
    L.dmcf_neighbor_dense_backward_workspace_bytes.argtypes = [c.POINTER(NeighborDenseBackwardArgs)]
    L.dmcf_neighbor_dense_backward.restype = c.c_int
    L.dmcf_neighbor_dense_backward.argtypes = [c.POINTER(NeighborDenseBackwardArgs), c.c_void_p, c.c_size_t, c.c_void_p]
    L.dmcf_neighbor_dense_kernel_names.restype = c.c_int
    L.dmcf_neighbor_dense_kernel_names.argtypes = [c.POINTER(NeighborDenseArgs), c.POINTER(NeighborDenseBackwardArgs), c.c_char_p,
                                                   c.c_size_t]
    L.dmcf_adam_step_workspace_bytes.restype = c.c_size_t
    L.dmcf_adam_step_workspace_bytes.argtypes = [c.POINTER(AdamArgs)]
    L.dmcf_adam_step.restype = c.c_int
    L.dmcf_adam_step.argtypes = [c.POINTER(AdamArgs), c.c_void_p, c.c_size_t, c.c_void_p]
    L.dmcf_adam_step_kernel_names.restype = c.c_int
    L.dmcf_adam_step_kernel_names.argtypes = [c.POINTER(AdamArgs), c.c_char_p, c.c_size_t]
    L.dmcf_raster_workspace_bytes.restype = c.c_size_t
    L.dmcf_raster_workspace_bytes.argtypes = [c.c_int64, c.c_int64, c.c_int64, c.c_int32, c.c_int32]
    L.dmcf_raster_count.restype = c.c_int
    L.dmcf_raster_count.argtypes = [c.c_void_p, c.c_int64, c.c_int64, c.c_int64, c.c_float, c.c_int32, c.c_int32, c.c_void_p, c.c_size_t,
                                    c.c_void_p, c.c_void_p]
    L.dmcf_raster_discs.restype = c.c_int
    L.dmcf_raster_discs.argtypes = [c.c_void_p, c.c_int64, c.c_int64, c.c_int64, c.c_float, c.c_uint32, c.c_int32, c.c_int32, c.c_void_p,
                                    c.c_void_p, c.c_size_t, c.c_void_p, c.c_int64, c.c_void_p]
    # metric gradients (ABI 2.13)
    for q in ("dmcf_nn_distance_backward_workspace_bytes", "dmcf_match_cost_backward_workspace_bytes",
              "dmcf_emd_backward_workspace_bytes"):
        getattr(L, q).restype = c.c_size_t
        getattr(L, q).argtypes = [c.c_int64, c.c_int64, c.c_int64]
    L.dmcf_nn_distance_backward.restype = c.c_int
    L.dmcf_nn_distance_backward.argtypes = [c.c_void_p, c.c_void_p, c.c_int64, c.c_int64, c.c_int64, c.c_void_p, c.c_void_p,
                                            c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_size_t, c.c_void_p]
    L.dmcf_match_cost_backward.restype = c.c_int
    L.dmcf_match_cost_backward.argtypes = [c.c_void_p, c.c_void_p, c.c_int64, c.c_int64, c.c_int64, c.c_void_p, c.c_void_p,
                                           c.c_void_p, c.c_void_p, c.c_void_p, c.c_size_t, c.c_void_p]
    L.dmcf_emd_with_levels.restype = c.c_int
    L.dmcf_emd_with_levels.argtypes = [c.c_void_p, c.c_void_p, c.c_int64, c.c_int64, c.c_int64, i32p, i32p, c.c_void_p, c.c_void_p,
                                       c.c_void_p, c.c_size_t, c.c_void_p]
    L.dmcf_emd_backward.restype = c.c_int
    L.dmcf_emd_backward.argtypes = [c.c_void_p, c.c_void_p, c.c_int64, c.c_int64, c.c_int64, i32p, i32p, c.c_void_p, c.c_void_p,
                                    c.c_void_p, c.c_void_p, c.c_void_p, c.c_size_t, c.c_void_p]
    L.dmcf_gather_point_backward_workspace_bytes.restype = c.c_size_t
    L.dmcf_gather_point_backward_workspace_bytes.argtypes = [c.c_int64, c.c_int64]
    L.dmcf_gather_point_backward.restype = c.c_int
    L.dmcf_gather_point_backward.argtypes = [c.c_void_p, c.c_void_p, c.c_int64, c.c_int, c.c_int64, c.c_void_p, c.c_void_p,
                                             c.c_size_t, c.c_void_p]
    # gradient of the window sum (ABI 2.14)
    L.dmcf_frs_window_sum_backward.restype = c.c_int
    L.dmcf_frs_window_sum_backward.argtypes = [c.c_void_p, c.c_int64, c.c_int64, c.c_float, c.c_int, c.c_int, c.c_void_p, c.c_void_p,
                                               c.c_void_p, c.c_size_t, c.c_void_p, c.c_void_p]
    # the column datasets' 1-D SPH solver (ABI 2.17)
    L.dmcf_sph1d_rollout.restype = c.c_int
    L.dmcf_sph1d_rollout.argtypes = [c.c_void_p, c.c_void_p, c.c_int64, c.c_int32, c.POINTER(Sph1dParams), c.c_int32, c.c_void_p,
                                     c.c_void_p, c.c_void_p, c.c_void_p]
    # the voxel convolution of SparseConv / SparseConvTranspose (ABI 2.18)
    L.dmcf_sparse_conv_forward.restype = c.c_int
    L.dmcf_sparse_conv_forward.argtypes = [c.POINTER(SparseConvArgs), c.c_void_p]
    L.dmcf_sparse_conv_backward_workspace_bytes.restype = c.c_size_t
    L.dmcf_sparse_conv_backward_workspace_bytes.argtypes = [c.POINTER(SparseConvArgs), c.c_int]
    L.dmcf_sparse_conv_backward.restype = c.c_int
    L.dmcf_sparse_conv_backward.argtypes = [c.POINTER(SparseConvArgs), c.c_void_p, c.c_void_p, c.c_void_p, c.c_int64, c.c_void_p,
                                            c.c_void_p, c.c_void_p, c.c_size_t, c.c_void_p]
    L.dmcf_sparse_conv_kernel_names.restype = c.c_int
    L.dmcf_sparse_conv_kernel_names.argtypes = [c.POINTER(SparseConvArgs), c.c_int, c.c_char_p, c.c_size_t]
    # both searches with points_row_splits / queries_row_splits (ABI 2.20)
    L.dmcf_frs_workspace_bytes_batched.restype = c.c_size_t
    L.dmcf_frs_workspace_bytes_batched.argtypes = [c.c_int64, c.c_int64, c.c_int64]
    L.dmcf_frs_build_batched.restype = c.c_int
    L.dmcf_frs_build_batched.argtypes = [c.c_void_p, c.c_int64, c.c_void_p, c.c_int64, c.c_float, c.c_void_p, c.c_size_t, c.c_void_p]
    L.dmcf_frs_count_batched.restype = c.c_int
    L.dmcf_frs_count_batched.argtypes = [c.c_void_p, c.c_int64, c.c_void_p, c.c_int64, c.c_int64, c.c_float, c.c_int, c.c_void_p,
                                         c.c_size_t, c.c_void_p, c.c_void_p]
    L.dmcf_frs_write_batched.restype = c.c_int
    L.dmcf_frs_write_batched.argtypes = [c.c_void_p, c.c_int64, c.c_void_p, c.c_int64, c.c_int64, c.c_float, c.c_int, c.c_void_p,
                                         c.c_size_t, c.c_void_p, c.c_void_p, c.c_void_p, c.c_int64, c.c_void_p]
    L.dmcf_radius_search_count_batched.restype = c.c_int
    L.dmcf_radius_search_count_batched.argtypes = [c.c_void_p, c.c_int64, c.c_void_p, c.c_int64, c.c_int64, c.c_void_p, c.c_float,
                                                   c.c_int, c.c_void_p, c.c_size_t, c.c_void_p, c.c_void_p]
    L.dmcf_radius_search_write_batched.restype = c.c_int
    L.dmcf_radius_search_write_batched.argtypes = [c.c_void_p, c.c_int64, c.c_void_p, c.c_int64, c.c_int64, c.c_void_p, c.c_float,
                                                   c.c_int, c.c_void_p, c.c_size_t, c.c_void_p, c.c_void_p, c.c_void_p, c.c_int64,
                                                   c.c_void_p]
    # grid_pos and the fluid box with row splits (ABI 2.21)
    L.dmcf_grid_pos_workspace_bytes_batched.restype = c.c_size_t
    L.dmcf_grid_pos_workspace_bytes_batched.argtypes = [c.c_int64, c.c_int64]
    L.dmcf_grid_pos_bounds_batched.restype = c.c_int
    L.dmcf_grid_pos_bounds_batched.argtypes = [c.c_void_p, c.c_int64, c.c_void_p, c.c_int64, f3, c.c_int, c.c_void_p, c.c_int,
                                               c.c_float, c.c_void_p, c.c_size_t, c.c_void_p]
    L.dmcf_grid_pos_count_batched.restype = c.c_int
    L.dmcf_grid_pos_count_batched.argtypes = [c.c_void_p, c.c_int64, c.c_void_p, c.c_int64, f3, c.c_int, c.c_int, c.c_float,
                                              c.c_void_p, c.c_size_t, c.c_void_p, c.c_int64, c.c_void_p, c.c_void_p]
    L.dmcf_grid_pos_write_batched.restype = c.c_int
    L.dmcf_grid_pos_write_batched.argtypes = [c.c_void_p, c.c_int64, c.c_void_p, c.c_int64, f3, c.c_int, c.c_int, c.c_float,
                                              c.c_void_p, c.c_size_t, c.c_void_p, c.c_int64, c.c_void_p, c.c_int64, c.c_void_p]
    L.dmcf_points_aabb_batched.restype = c.c_int
    L.dmcf_points_aabb_batched.argtypes = [c.c_void_p, c.c_int64, c.c_void_p, c.c_int64, c.c_void_p, c.c_void_p]
    # the window sum and its gradient with row splits (ABI 2.22)
    L.dmcf_frs_window_sum_batched.restype = c.c_int
    L.dmcf_frs_window_sum_batched.argtypes = [c.c_void_p, c.c_int64, c.c_void_p, c.c_int64, c.c_int64, c.c_float, c.c_int, c.c_int,
                                              c.c_void_p, c.c_size_t, c.c_void_p, c.c_void_p, c.c_void_p]
    L.dmcf_frs_window_sum_backward_batched.restype = c.c_int
    L.dmcf_frs_window_sum_backward_batched.argtypes = [c.c_void_p, c.c_int64, c.c_void_p, c.c_int64, c.c_int64, c.c_float, c.c_int,
                                                       c.c_int, c.c_void_p, c.c_void_p, c.c_void_p, c.c_size_t, c.c_void_p,
                                                       c.c_void_p]
    # nn_distance over a ragged batch (ABI 2.23): HOST row splits
    L.dmcf_nn_distance_ragged_workspace_bytes.restype = c.c_size_t
    L.dmcf_nn_distance_ragged_workspace_bytes.argtypes = [c.c_int64, c.c_int64, c.c_int64]
    i64p = c.POINTER(c.c_int64)
    L.dmcf_nn_distance_ragged.restype = c.c_int
    L.dmcf_nn_distance_ragged.argtypes = [c.c_void_p, c.c_int64, i64p, c.c_void_p, c.c_int64, i64p, c.c_int64, c.c_void_p,
                                          c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_size_t, c.c_void_p]
    # the fused EMD over a ragged batch (ABI 2.24): HOST row splits, read by the workspace query too
    L.dmcf_emd_ragged_workspace_bytes.restype = c.c_size_t
    L.dmcf_emd_ragged_workspace_bytes.argtypes = [c.c_int64, i64p, c.c_int64, i64p, c.c_int64]
    L.dmcf_emd_ragged.restype = c.c_int
    L.dmcf_emd_ragged.argtypes = [c.c_void_p, c.c_int64, i64p, c.c_void_p, c.c_int64, i64p, c.c_int64, c.c_void_p, c.c_void_p,
                                  c.c_size_t, c.c_void_p]
    # the gradient of the ragged EMD (ABI 2.25): the recording forward, and the backward with its own workspace query
    L.dmcf_emd_ragged_with_levels.restype = c.c_int
    L.dmcf_emd_ragged_with_levels.argtypes = [c.c_void_p, c.c_int64, i64p, c.c_void_p, c.c_int64, i64p, c.c_int64, c.c_void_p,
                                              c.c_void_p, c.c_void_p, c.c_size_t, c.c_void_p]
    L.dmcf_emd_ragged_backward_workspace_bytes.restype = c.c_size_t
    L.dmcf_emd_ragged_backward_workspace_bytes.argtypes = [c.c_int64, i64p, c.c_int64, i64p, c.c_int64]
    L.dmcf_emd_ragged_backward.restype = c.c_int
    L.dmcf_emd_ragged_backward.argtypes = [c.c_void_p, c.c_int64, i64p, c.c_void_p, c.c_int64, i64p, c.c_int64, c.c_void_p,
                                           c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_size_t, c.c_void_p]
    # the percentiles and histograms of compare_dist over a ragged batch (ABI 2.26): HOST row splits and plan
    L.dmcf_hist_pair_ragged_workspace_bytes.restype = c.c_size_t
    L.dmcf_hist_pair_ragged_workspace_bytes.argtypes = [c.c_int64, c.c_int64, c.c_int64]
    L.dmcf_hist_pair_ragged.restype = c.c_int
    L.dmcf_hist_pair_ragged.argtypes = [c.c_void_p, c.c_void_p, c.c_int64, i64p, c.c_int64, c.POINTER(HistPlan), c.c_int64,
                                        c.c_void_p, c.c_void_p, c.c_void_p, c.c_size_t, c.c_void_p]
    # the depth-tested sphere splat of the 3-D renderer (ABI 2.27)
    L.dmcf_splat_depth.restype = c.c_int
    L.dmcf_splat_depth.argtypes = [c.c_void_p, c.c_int64, c.c_int64, c.c_int64, c.c_float, c.c_float, c.POINTER(Camera), c.c_int32,
                                   c.c_int32, c.c_int32, c.c_void_p, c.c_void_p]
    L.dmcf_splat_shade.restype = c.c_int
    L.dmcf_splat_shade.argtypes = [c.POINTER(SplatLayer), c.c_int32, c.POINTER(Camera), c.c_float, c.c_float, c.c_int32, c.c_int32,
                                   c.c_int64, c.c_void_p, c.c_void_p, c.c_void_p]
    _lib = L
    return L


def check(rc, what):
    if rc != 0:
        L = lib()
        raise DmcfError(f"{what}: {L.dmcf_error_string(rc).decode()} (code {rc}, hip error {L.dmcf_last_hip_error()})")
