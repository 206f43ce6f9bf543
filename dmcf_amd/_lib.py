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


_int, _i32, _u32, _i64, _f32, _size = (ctypes.c_int, ctypes.c_int32, ctypes.c_uint32, ctypes.c_int64, ctypes.c_float,
                                        ctypes.c_size_t)
_ptr, _str, _P = ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER  # (_ptr: device and host pointers, and dmcf_stream_t)

# signatures several entry points share: (restype, argtypes) where they are the same call, the leading arguments otherwise
_BYTES_N = (_size, (_i64,))                 # (n) -> size_t
_BYTES_NM = (_size, (_i64, _i64))           # (n, m) -> size_t
_BYTES_BNM = (_size, (_i64, _i64, _i64))    # (b, n, m) -> size_t, and the other queries over three counts
_BYTES_RAGGED = (_size, (_i64, _P(_i64), _i64, _P(_i64), _i64))  # (n_total, HOST row_splits1, m_total, HOST row_splits2, batch)
_ITEMS = (_ptr, _i64)                       # row_splits, batch: what a *_batched entry point takes after (points, n)
_FRS = (_ptr, _i64, _i64, _f32, _int, _ptr, _size)  # queries, n_queries, n_points, radius, flags, workspace, workspace_bytes
_FRS_BATCHED = (_ptr, _i64, *_ITEMS, _i64, _f32, _int, _ptr, _size)
_RADIUS = (_ptr, _i64, _i64, _ptr, _f32, _int, _ptr, _size)  # queries, n_queries, n_points, radii, max_radius, flags, workspace, ..
_RADIUS_BATCHED = (_ptr, _i64, *_ITEMS, _i64, _ptr, _f32, _int, _ptr, _size)
_WINDOW_SUM = (_ptr, _i64, _i64, _f32, _int, _int)  # queries, n_queries, n_points, radius, flags, window
_WINDOW_SUM_BATCHED = (_ptr, _i64, *_ITEMS, _i64, _f32, _int, _int)
_GRID = (_P(_f32), _int, _int, _f32, _ptr, _size, _ptr, _i64)  # HOST voxel_size, centralize, pad, hyst, workspace, .., cell_table, ..
_GHOST = (_ptr, _i64, _ptr, _i32, _ptr, _i32, _ptr)  # points, n, boxes, n_boxes, widths2, n_widths, totals / rows
_PADDED = (_ptr, _ptr, _i64, _i64, _i64)    # xyz1, xyz2, b, n, m: the metrics on padded batches
_RAGGED = (_ptr, _i64, _P(_i64), _ptr, _i64, _P(_i64), _i64)  # xyz1, n_total, HOST row_splits1, xyz2, m_total, HOST row_splits2, batch
_COUNTS = (_P(_i32), _P(_i32))              # HOST count1, count2 (or NULL)
_MATCH = (_int, (*_PADDED, *_COUNTS, _ptr, _ptr, _size, _ptr))  # .., match / cost, workspace, workspace_bytes, stream
_NAME = (_str, _size)                       # name(s), name_bytes: the diagnostics' output
_RASTER = (_ptr, _i64, _i64, _i64, _f32)    # xy, n_points, n_frames, frame_stride, radius

# Every entry point include/dmcf_hip.h declares, in the header's order: name -> (restype, argtypes).  tests/test_abi.py holds
# the header, this table and the struct mirrors above together.
PROTOTYPES = {
    "dmcf_version": (_int, ()),
    "dmcf_error_string": (_str, (_int,)),
    "dmcf_last_hip_error": (_int, ()),
    "dmcf_frs_workspace_bytes": _BYTES_NM,
    "dmcf_frs_build": (_int, (_ptr, _i64, _f32, _ptr, _size, _ptr)),
    "dmcf_frs_count": (_int, (*_FRS, _ptr, _ptr)),
    "dmcf_frs_write": (_int, (*_FRS, _ptr, _ptr, _ptr, _i64, _ptr)),
    "dmcf_frs_search_padded": (_int, (*_FRS, _i64, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr)),
    "dmcf_frs_window_sum": (_int, (*_WINDOW_SUM, _ptr, _size, _ptr, _ptr)),
    # gradient of the window sum (ABI 2.14)
    "dmcf_frs_window_sum_backward": (_int, (*_WINDOW_SUM, _ptr, _ptr, _ptr, _size, _ptr, _ptr)),
    "dmcf_radius_search_count": (_int, (*_RADIUS, _ptr, _ptr)),
    "dmcf_radius_search_write": (_int, (*_RADIUS, _ptr, _ptr, _ptr, _i64, _ptr)),
    # both searches with points_row_splits / queries_row_splits (ABI 2.20)
    "dmcf_frs_workspace_bytes_batched": _BYTES_BNM,
    "dmcf_frs_build_batched": (_int, (_ptr, _i64, *_ITEMS, _f32, _ptr, _size, _ptr)),
    "dmcf_frs_count_batched": (_int, (*_FRS_BATCHED, _ptr, _ptr)),
    "dmcf_frs_write_batched": (_int, (*_FRS_BATCHED, _ptr, _ptr, _ptr, _i64, _ptr)),
    "dmcf_radius_search_count_batched": (_int, (*_RADIUS_BATCHED, _ptr, _ptr)),
    "dmcf_radius_search_write_batched": (_int, (*_RADIUS_BATCHED, _ptr, _ptr, _ptr, _i64, _ptr)),
    # the window sum and its gradient with row splits (ABI 2.22)
    "dmcf_frs_window_sum_batched": (_int, (*_WINDOW_SUM_BATCHED, _ptr, _size, _ptr, _ptr, _ptr)),
    "dmcf_frs_window_sum_backward_batched": (_int, (*_WINDOW_SUM_BATCHED, _ptr, _ptr, _ptr, _size, _ptr, _ptr)),
    "dmcf_cconv_workspace_bytes": (_size, (_P(CconvArgs),)),
    "dmcf_cconv_forward": (_int, (_P(CconvArgs), _ptr, _size, _ptr)),
    "dmcf_cconv_kernel_name": (_int, (_P(CconvArgs), *_NAME)),
    "dmcf_cconv_forward_extents": (_int, (_P(CconvArgs), _ptr, _ptr, _size, _ptr)),
    "dmcf_cconv_extents_kernel_name": (_int, (_P(CconvArgs), *_NAME)),
    "dmcf_invert_neighbors_list_workspace_bytes": _BYTES_N,
    "dmcf_invert_neighbors_list": (_int, (_i64, _ptr, _ptr, _ptr, _i64, _i64, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _size, _ptr)),
    "dmcf_cconv_backward_workspace_bytes": (_size, (_P(CconvArgs), _P(CconvBackwardArgs))),
    "dmcf_cconv_backward": (_int, (_P(CconvArgs), _P(CconvBackwardArgs), _ptr, _size, _ptr)),
    "dmcf_cconv_backward_kernel_names": (_int, (_P(CconvArgs), _P(CconvBackwardArgs), *_NAME)),
    # gradients through per-point extents (ABI 2.15)
    "dmcf_cconv_backward_extents": (_int, (_P(CconvArgs), _P(CconvBackwardArgs), _ptr, _ptr, _size, _ptr)),
    "dmcf_cconv_backward_extents_kernel_names": (_int, (_P(CconvArgs), _P(CconvBackwardArgs), *_NAME)),
    "dmcf_cconv_scatter_plan_bytes": _BYTES_N,
    "dmcf_cconv_scatter_plan": (_int, (_ptr, _i64, _ptr, _i64, _f32, _f32, _i32, _ptr, _size, _ptr)),
    # splat S's reach, box limit and instantiation, host only (ABI 2.28)
    "dmcf_cconv_scatter_reach": (_i32, (_f32, _f32)),
    "dmcf_cconv_scatter_kernel_name": (_int, (_i32 * 5, _i32, _i32, *_NAME)),
    "dmcf_cconv_scatter_workspace_bytes": (_size, (_P(CconvScatterArgs),)),
    "dmcf_cconv_scatter_forward": (_int, (_P(CconvScatterArgs), _ptr, _size, _ptr)),
    # the backward of the scatter form (ABI 2.19)
    "dmcf_cconv_scatter_backward_workspace_bytes": (_size, (_P(CconvScatterArgs), _P(CconvScatterBackwardArgs))),
    "dmcf_cconv_scatter_backward": (_int, (_P(CconvScatterArgs), _P(CconvScatterBackwardArgs), _ptr, _size, _ptr)),
    "dmcf_lattice_conv_workspace_bytes": (_size, (_P(LatticeConvArgs),)),
    "dmcf_lattice_conv_forward": (_int, (_P(LatticeConvArgs), _ptr, _size, _ptr)),
    "dmcf_lattice_conv_batch_workspace_bytes": (_size, (_P(LatticeConvArgs), _i32)),
    "dmcf_lattice_conv_forward_batch": (_int, (_P(LatticeConvArgs), _i32, _ptr, _size, _ptr)),
    # gradients of the lattice form (ABI 2.16)
    "dmcf_lattice_conv_backward_workspace_bytes": (_size, (_P(LatticeConvArgs), _i32)),
    "dmcf_lattice_conv_backward": (_int, (_P(LatticeConvArgs), _i32, _ptr, _ptr, _ptr, _ptr, _size, _ptr)),
    "dmcf_reduce_subarrays_sum": (_int, (_ptr, _ptr, _i64, _ptr, _ptr)),
    "dmcf_dense_forward": (_int, (_ptr, _i64, _i32, _ptr, _i32, _ptr, _ptr, _ptr, _ptr)),
    "dmcf_points_aabb_workspace_bytes": (_size, ()),
    "dmcf_points_aabb": (_int, (_ptr, _i64, _ptr, _ptr, _size, _ptr)),
    "dmcf_points_aabb_batched": (_int, (_ptr, _i64, *_ITEMS, _ptr, _ptr)),  # (ABI 2.21, with grid_pos below)
    "dmcf_ghost_workspace_bytes": (_size, (_i64, _i32, _i32)),
    "dmcf_ghost_count": (_int, (*_GHOST, _ptr, _size, _ptr)),
    "dmcf_ghost_write": (_int, (*_GHOST, _ptr, _ptr, _ptr, _size, _ptr)),
    "dmcf_grid_pos_workspace_bytes": _BYTES_N,
    "dmcf_grid_pos_bounds": (_int, (_ptr, _i64, _P(_f32), _int, _ptr, _int, _f32, _ptr, _size, _ptr)),
    "dmcf_grid_pos_count": (_int, (_ptr, _i64, *_GRID, _ptr)),
    "dmcf_grid_pos_write": (_int, (_ptr, _i64, *_GRID, _ptr, _i64, _ptr)),
    # grid_pos and the fluid box with row splits (ABI 2.21)
    "dmcf_grid_pos_workspace_bytes_batched": _BYTES_NM,
    "dmcf_grid_pos_bounds_batched": (_int, (_ptr, _i64, *_ITEMS, _P(_f32), _int, _ptr, _int, _f32, _ptr, _size, _ptr)),
    "dmcf_grid_pos_count_batched": (_int, (_ptr, _i64, *_ITEMS, *_GRID, _ptr, _ptr)),
    "dmcf_grid_pos_write_batched": (_int, (_ptr, _i64, *_ITEMS, *_GRID, _ptr, _i64, _ptr)),
    "dmcf_fps_workspace_bytes": _BYTES_N,
    "dmcf_farthest_point_sample": (_int, (_ptr, _i64, _i64, _ptr, _size, _ptr, _ptr)),
    "dmcf_gather_point": (_int, (_ptr, _ptr, _i64, _int, _ptr, _ptr)),
    "dmcf_nn_distance_workspace_bytes": _BYTES_BNM,
    "dmcf_nn_distance": (_int, (*_PADDED, _ptr, _ptr, _ptr, _ptr, _ptr, _size, _ptr)),
    # nn_distance over a ragged batch (ABI 2.23): HOST row splits
    "dmcf_nn_distance_ragged_workspace_bytes": _BYTES_BNM,
    "dmcf_nn_distance_ragged": (_int, (*_RAGGED, _ptr, _ptr, _ptr, _ptr, _ptr, _size, _ptr)),
    "dmcf_approx_match_workspace_bytes": _BYTES_BNM,
    "dmcf_approx_match": _MATCH,
    "dmcf_match_cost_workspace_bytes": _BYTES_BNM,
    "dmcf_match_cost": (_int, (*_PADDED, _ptr, _ptr, _ptr, _size, _ptr)),
    "dmcf_emd_workspace_bytes": _BYTES_BNM,
    "dmcf_emd": _MATCH,
    # the fused EMD over a ragged batch (ABI 2.24): HOST row splits, read by the workspace query too
    "dmcf_emd_ragged_workspace_bytes": _BYTES_RAGGED,
    "dmcf_emd_ragged": (_int, (*_RAGGED, _ptr, _ptr, _size, _ptr)),
    # metric gradients (ABI 2.13)
    "dmcf_nn_distance_backward_workspace_bytes": _BYTES_BNM,
    "dmcf_nn_distance_backward": (_int, (*_PADDED, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _size, _ptr)),
    "dmcf_match_cost_backward_workspace_bytes": _BYTES_BNM,
    "dmcf_match_cost_backward": (_int, (*_PADDED, _ptr, _ptr, _ptr, _ptr, _ptr, _size, _ptr)),
    "dmcf_emd_with_levels": (_int, (*_PADDED, *_COUNTS, _ptr, _ptr, _ptr, _size, _ptr)),
    "dmcf_emd_backward_workspace_bytes": _BYTES_BNM,
    "dmcf_emd_backward": (_int, (*_PADDED, *_COUNTS, _ptr, _ptr, _ptr, _ptr, _ptr, _size, _ptr)),
    # the gradient of the ragged EMD (ABI 2.25): the recording forward, and the backward with its own workspace query
    "dmcf_emd_ragged_with_levels": (_int, (*_RAGGED, _ptr, _ptr, _ptr, _size, _ptr)),
    "dmcf_emd_ragged_backward_workspace_bytes": _BYTES_RAGGED,
    "dmcf_emd_ragged_backward": (_int, (*_RAGGED, _ptr, _ptr, _ptr, _ptr, _ptr, _size, _ptr)),
    # the percentiles and histograms of compare_dist over a ragged batch (ABI 2.26): HOST row splits and plan
    "dmcf_hist_pair_ragged_workspace_bytes": _BYTES_BNM,
    "dmcf_hist_pair_ragged": (_int, (_ptr, _ptr, _i64, _P(_i64), _i64, _P(HistPlan), _i64, _ptr, _ptr, _ptr, _size, _ptr)),
    "dmcf_gather_point_backward_workspace_bytes": _BYTES_NM,  # (ABI 2.13)
    "dmcf_gather_point_backward": (_int, (_ptr, _ptr, _i64, _int, _i64, _ptr, _ptr, _size, _ptr)),
    "dmcf_neighbor_dense_forward": (_int, (_P(NeighborDenseArgs), _ptr)),
    "dmcf_neighbor_dense_backward_workspace_bytes": (_size, (_P(NeighborDenseBackwardArgs),)),
    "dmcf_neighbor_dense_backward": (_int, (_P(NeighborDenseBackwardArgs), _ptr, _size, _ptr)),
    "dmcf_neighbor_dense_kernel_names": (_int, (_P(NeighborDenseArgs), _P(NeighborDenseBackwardArgs), *_NAME)),
    "dmcf_adam_step_workspace_bytes": (_size, (_P(AdamArgs),)),
    "dmcf_adam_step": (_int, (_P(AdamArgs), _ptr, _size, _ptr)),
    "dmcf_adam_step_kernel_names": (_int, (_P(AdamArgs), *_NAME)),
    "dmcf_raster_workspace_bytes": (_size, (_i64, _i64, _i64, _i32, _i32)),
    "dmcf_raster_count": (_int, (*_RASTER, _i32, _i32, _ptr, _size, _ptr, _ptr)),
    "dmcf_raster_discs": (_int, (*_RASTER, _u32, _i32, _i32, _ptr, _ptr, _size, _ptr, _i64, _ptr)),
    # the depth-tested sphere splat of the 3-D renderer (ABI 2.27)
    "dmcf_splat_depth": (_int, (*_RASTER, _f32, _P(Camera), _i32, _i32, _i32, _ptr, _ptr)),
    "dmcf_splat_shade": (_int, (_P(SplatLayer), _i32, _P(Camera), _f32, _f32, _i32, _i32, _i64, _ptr, _ptr, _ptr)),
    # the column datasets' 1-D SPH solver (ABI 2.17)
    "dmcf_sph1d_rollout": (_int, (_ptr, _ptr, _i64, _i32, _P(Sph1dParams), _i32, _ptr, _ptr, _ptr, _ptr)),
    # the voxel convolution of SparseConv / SparseConvTranspose (ABI 2.18)
    "dmcf_sparse_conv_forward": (_int, (_P(SparseConvArgs), _ptr)),
    "dmcf_sparse_conv_backward_workspace_bytes": (_size, (_P(SparseConvArgs), _int)),
    "dmcf_sparse_conv_backward": (_int, (_P(SparseConvArgs), _ptr, _ptr, _ptr, _i64, _ptr, _ptr, _ptr, _size, _ptr)),
    "dmcf_sparse_conv_kernel_names": (_int, (_P(SparseConvArgs), _int, *_NAME)),
}
SYMBOLS = list(PROTOTYPES)  # (tests and tools import the names under this one)


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
    for name, (restype, argtypes) in PROTOTYPES.items():
        entry = getattr(L, name)
        entry.restype, entry.argtypes = restype, list(argtypes)
    _lib = L
    return L


def call(name, *args):
    """Call the entry point `name`, which returns a DMCF_* status; anything but DMCF_OK raises DmcfError."""
    rc = getattr(lib(), name)(*args)
    if rc != 0:
        check(rc, name)


def check(rc, what):
    if rc != 0:
        L = lib()
        raise DmcfError(f"{what}: {L.dmcf_error_string(rc).decode()} (code {rc}, hip error {L.dmcf_last_hip_error()})")
