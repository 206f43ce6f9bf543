/*
 * dmcf_hip.h -- C ABI of libdmcf_hip.so: the MI355X (gfx950) implementation of DMCF's per-step
 * particle hot path.  This is the drop-in boundary: these entry points are what the reference's
 * Python layer binds in place of the Open3D (open3d==0.15.2) TensorFlow operators it calls.
 * Paths below are relative to the reference tree (tum-pbs/DMCF).
 *
 *   reference operator (call site)                               replaced by
 *   ------------------------------------------------------------ -------------------------------
 *   ml3d.layers.FixedRadiusSearch = build_spatial_hash_table +   dmcf_frs_build / dmcf_frs_count /
 *     fixed_radius_search  (utils/convolutions.py:207-210,        dmcf_frs_write
 *     354-358; utils/tools/losses.py:296-298,339-341)
 *   window functions (utils/tools/losses.py:8-44) applied at     DMCF_WINDOW_* fused into
 *     utils/convolutions.py:359-379                               dmcf_cconv_forward
 *   ml3d.ops.continuous_conv (utils/convolutions.py:414-431)     dmcf_cconv_forward
 *   ASCC: mirror :410-412 + second continuous_conv :433-458      dmcf_cconv_forward(DMCF_FLAG_SYMMETRIC)
 *   ml3d.layers.RadiusSearch (utils/convolutions.py:212-216,     dmcf_frs_build / dmcf_radius_search_count /
 *     366-370, 1006-1010: extents of rank 1)                      dmcf_radius_search_write
 *   both searches with points_row_splits / queries_row_splits    dmcf_frs_build_batched / dmcf_frs_count_batched /
 *     (a batch of point sets in one call; ABI 2.20)               dmcf_frs_write_batched, dmcf_radius_search_*_batched
 *   compute_density per sample of a training batch               dmcf_frs_window_sum_batched /
 *     (pipelines/simulator.py:227-243 inside the warm-up loop)    dmcf_frs_window_sum_backward_batched (ABI 2.22)
 *   nn_distance per scene of a validation split                  dmcf_nn_distance_ragged (ABI 2.23: one call for
 *     (pipelines/simulator.py:222-248, utils/evaluation_helper.py)  scenes of different particle counts)
 *   emd_loss per scene of a validation split                     dmcf_emd_ragged (ABI 2.24: the same, with
 *     (pipelines/simulator.py:247-249, utils/tools/losses.py:401-409)  dmcf_emd's bits for every scene)
 *   EmdLoss / ChamferLoss terms per sample of a training batch   dmcf_emd_ragged_with_levels / dmcf_emd_ragged_backward
 *     (utils/tools/losses.py:401-414)                             (ABI 2.25: the ragged EMD's gradient, 4 launches
 *                                                                 whatever the batch)
 *   compare_dist per scene of a validation split                 dmcf_hist_pair_ragged (ABI 2.26: percentiles and
 *     (pipelines/simulator.py:250-251, utils/evaluation_helper.py:43-75)  histograms of all scenes, the host's bits)
 *   (no reference counterpart: the reference renders 2-D         dmcf_splat_depth / dmcf_splat_shade (ABI 2.27: a
 *     results only, utils/draw_sim2d.py)                           depth-tested sphere splat for 3-D result files)
 *   continuous_conv with extents [n_out,1] (:397-399)            dmcf_cconv_forward_extents (gradients:
 *                                                                 dmcf_cconv_backward_extents)
 *   continuous_conv between grid_pos lattices                    dmcf_lattice_conv_forward (gradients, ABI 2.16:
 *     (models/hrnet.py:85-92)                                     dmcf_lattice_conv_backward)
 *   continuous_conv from particles onto a grid_pos lattice,      dmcf_cconv_scatter_forward (gradients, ABI 2.19:
 *     4 or 8 output channels (models/hrnet.py:83-93)              dmcf_cconv_scatter_backward)
 *   o3dml.ops.reduce_subarrays_sum (models/pbf_model.py:450-453) dmcf_reduce_subarrays_sum
 *   tf.keras.layers.Dense (models/hrnet.py:49,93-99;             dmcf_dense_forward
 *     models/pbf_model.py:134-152)
 *   tf.reduce_min / reduce_max of the positions                  dmcf_points_aabb
 *     (models/pbf_model.py:330-336)
 *   farthest_point_sample / gather_point (utils/tools/sampling.cu) dmcf_farthest_point_sample / dmcf_gather_point
 *   grid_pos: candidate cells + tf.unique + decode               dmcf_grid_pos_bounds / _count / _write
 *     (utils/tools/losses.py:136-181, called from :266-272)
 *   grid_pos and the fluid box of a BATCH of point sets          dmcf_grid_pos_bounds_batched / _count_batched /
 *     (row splits; no reference counterpart: the reference         _write_batched, dmcf_points_aabb_batched (ABI 2.21)
 *     loops over the samples of a training batch)
 *   SPH1D.step in gen_data's time loop                           dmcf_sph1d_rollout (ABI 2.17: the column
 *     (datasets/column_gen.py:159-186, 305-312)                    datasets' generator)
 *   SparseConv / SparseConvTranspose: FixedRadiusSearch('Linf')  DMCF_FRS_METRIC_LINF, dmcf_sparse_conv_forward /
 *     + continuous_conv / continuous_conv_transpose with         dmcf_sparse_conv_backward (ABI 2.18)
 *     nearest-neighbour cells (utils/convolutions.py:476-885)
 *
 * Conventions
 *   - plain C: raw DEVICE pointers, sizes, a stream handle (hipStream_t passed as void*); no
 *     torch / HIP types in any signature.
 *   - every function returns DMCF_OK (0) or a negative DMCF_E* code; nothing throws; arguments are
 *     validated on the host; kernels are enqueued on `stream` and NOT synchronised.
 *   - ownership: the caller owns every buffer.  The library never allocates device memory; scratch
 *     comes from a caller-supplied workspace whose size the *_workspace_bytes functions report.
 *   - stateless and re-entrant: ordering only through `stream`.
 *   - layouts: positions [n,3] float32 row-major xyz (z = 0 in 2-D scenes); features [n,C] float32
 *     row-major; filters [D(z),H(y),W(x),Cin,Cout] float32 row-major; CSR neighbour lists with
 *     int32 indices and int64 row splits (the dtypes of Open3D 0.15.2's op); distances are
 *     squared L2.
 *   - two-phase search because the number of pairs is data dependent:
 *       build -> count (fills row_splits) -> caller reads row_splits[m], allocates -> write.
 */
#ifndef DMCF_HIP_H_
#define DMCF_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DMCF_OK 0
#define DMCF_EINVAL (-1)      /* bad argument (null pointer, negative size, unsupported option) */
#define DMCF_EWORKSPACE (-2)  /* workspace too small */
#define DMCF_ELAUNCH (-3)     /* HIP reported an error when enqueuing (see dmcf_last_hip_error) */
#define DMCF_EUNSUPPORTED (-4) /* valid in the reference, not implemented on this path yet */

typedef void* dmcf_stream_t; /* hipStream_t */

/* library / ABI version (major*10000 + minor*100 + patch) and error text */
int dmcf_version(void);
const char* dmcf_error_string(int code);
int dmcf_last_hip_error(void); /* hipError_t of the last failed enqueue on this thread */

/* ------------------------------------------------------------------------------------------------
 * Fixed-radius search.  Replaces ml3d.layers.FixedRadiusSearch(metric='L2', ignore_query_point,
 * return_distances)(points, queries, radius)  (utils/convolutions.py:207-210, 354-358).
 * Result contract (what the reference's callers observe): for every query i the SET
 *   { j : ((dx*dx + dy*dy) + dz*dz) <= radius*radius }     float32, un-fused, inclusive,
 * minus points whose coordinates equal the query's when DMCF_FRS_IGNORE_QUERY_POINT is set.
 * The order inside a row is implementation defined in the reference (hash-bin order, atomics);
 * here it is deterministic: ascending grid cell (z, y, x), then ascending point index.
 * ---------------------------------------------------------------------------------------------- */
#define DMCF_FRS_IGNORE_QUERY_POINT 1
/* Opt-in emulations of what open3d 0.15.2's hash walk can SEE in float arithmetic.  The library hashes the points into voxels
 * of edge 2 R and visits, for a query, the bins of its own voxel and of the 8 voxels holding the corners q +- R (SURVEY.md
 * section 8 row a1).  In exact arithmetic those voxels cover the search sphere: the set above, which is what the search returns
 * WITHOUT either flag -- symmetric lists, on which the ASCC layer's momentum conservation rests (models/sym_net.py:42-53).  In
 * float, for about one query in 10^6 (q a rounding step from the middle of a voxel) the corner voxels of an axis are TWO
 * apart and the walk misses part of the sphere; a pair at distance R within rounding can sit one voxel outside as well.
 *   DMCF_FRS_OPEN3D_VOXEL_WALK     a hit counts only if the point's voxel hashes into the bin of the query's own voxel or of
 *                                  one of the 8 corner voxels (table of clamp(n_points / 64, 1, 2^25) bins, the layer's
 *                                  default) -- such a query keeps what lies in its own voxel;
 *   DMCF_FRS_OPEN3D_CORNER_VOXELS  the same with the 8 corner voxels alone (round 3's reading of the library: such a query's
 *                                  row comes out nearly empty).
 * Each is bit-exact against the restatement of that walk in oracle/ (dmcf_ref_fixed_radius_search, bin_set); which of the two
 * the library implements is one of the questions tools/capture_golden.py settles.  At most one of them may be set. */
#define DMCF_FRS_OPEN3D_CORNER_VOXELS 2
#define DMCF_FRS_OPEN3D_VOXEL_WALK 4
/* ABI 2.18: the max-norm search of ml3d.layers.FixedRadiusSearch(metric='Linf') (utils/convolutions.py:561-562, 760-761):
 *   { j : max(|dx|, |dy|, |dz|) <= radius }     float32 differences, inclusive,
 * on the structure of dmcf_frs_build(points, radius), rows in the same order.  dmcf_frs_count and dmcf_frs_write only, index
 * lists only: with this flag a distance output, an OPEN3D_* flag, dmcf_frs_search_padded and dmcf_frs_window_sum are
 * DMCF_EUNSUPPORTED (dmcf_frs_window_sum_backward, which has always refused every flag it does not know, keeps answering
 * DMCF_EINVAL). */
#define DMCF_FRS_METRIC_LINF 8

/* bytes of workspace for a search structure over n_points that will serve up to n_queries queries */
size_t dmcf_frs_workspace_bytes(int64_t n_points, int64_t n_queries);

/* build the cell-sorted uniform grid of `points` in `workspace` (device memory, 256-B aligned) */
int dmcf_frs_build(const float* points, int64_t n_points, float radius, void* workspace,
                   size_t workspace_bytes, dmcf_stream_t stream);

/* count neighbours of each query and write the int64 exclusive prefix sum to row_splits[0..m];
 * n_points / radius / workspace must be the ones given to dmcf_frs_build */
int dmcf_frs_count(const float* queries, int64_t n_queries, int64_t n_points, float radius, int flags,
                   void* workspace, size_t workspace_bytes, int64_t* row_splits, dmcf_stream_t stream);

/* write neighbors_index[P] (int32) and, if not NULL, neighbors_distance[P] (squared L2).  pair_capacity = number
 * of entries the two output buffers hold.  A caller that read row_splits[m] passes exactly that.  A caller that
 * wants NO host round trip allocates from an estimate (e.g. the previous time step's count plus slack), enqueues
 * count + write back to back and checks row_splits[m] <= pair_capacity later: rows that would not fit are skipped
 * as a whole, never written out of bounds. */
int dmcf_frs_write(const float* queries, int64_t n_queries, int64_t n_points, float radius, int flags,
                   const void* workspace, size_t workspace_bytes, const int64_t* row_splits,
                   int32_t* neighbors_index, float* neighbors_distance, int64_t pair_capacity,
                   dmcf_stream_t stream);

/* Single-pass search into PADDED rows, for callers that know an upper bound of the row lengths (a rollout takes the
 * largest row of the previous time step + slack): row i is written at neighbors_index[i * row_stride ...], its length
 * (clamped to row_stride) goes to row_count[i], row_begin[i] = i * row_stride for i = 0..n_queries, and the largest
 * unclamped length is max-ed into *max_count (a device int32 the caller zeroed) -- max_count > row_stride means rows
 * were truncated and the caller must repeat with a larger stride or with dmcf_frs_count / dmcf_frs_write.  No count
 * pass, no prefix scan: one candidate scan per query.  Same neighbours in the same order per row as dmcf_frs_write;
 * dmcf_cconv_forward consumes the result through args->neighbors_row_count. */
int dmcf_frs_search_padded(const float* queries, int64_t n_queries, int64_t n_points, float radius, int flags,
                           const void* workspace, size_t workspace_bytes, int64_t row_stride, int64_t* row_begin,
                           int32_t* row_count, int32_t* neighbors_index, float* neighbors_distance, int32_t* max_count,
                           dmcf_stream_t stream);

/* compute_density (utils/tools/losses.py:285-306; models/pbf_model.py:351-355, pipelines/simulator.py:227-243):
 *   out[q] = sum over the points p within `radius` of query q of window(|p - q|^2 / radius^2)
 * evaluated inside the candidate scan of the search -- the pair list is never materialised.  `window` is a
 * DMCF_WINDOW_* id (DMCF_WINDOW_NONE counts the neighbours, DMCF_WINDOW_EXPLICIT sums the squared distances);
 * flags as for dmcf_frs_count.  Uses the workspace of dmcf_frs_build(points). */
int dmcf_frs_window_sum(const float* queries, int64_t n_queries, int64_t n_points, float radius, int flags, int window,
                        const void* workspace, size_t workspace_bytes, float* out, dmcf_stream_t stream);

/* Gradient of dmcf_frs_window_sum w.r.t. the positions (ABI 2.14): the same candidate scan -- one wavefront per query on the
 * workspace of dmcf_frs_build(points) -- with three sums instead of one.  For every query q it WRITES
 *   grad[3 q .. 3 q + 2] = 2 * sum over the points p with |p - q|^2 <= radius^2 of
 *                          (coef_queries[q] + coef_points[p]) * dw/d(d^2)(|p - q|^2) * (q - p)
 * coef_queries [n_queries] and coef_points [n_points] (indexed by the point's ORIGINAL index) are the gradients arriving at the
 * sums; either may be NULL, meaning 0, both NULL: DMCF_EINVAL.  One entry gives all three gradients of out = window_sum(points,
 * queries):
 *   d/d queries:  this workspace, coef_queries = grad_out;
 *   d/d points:   the workspace of dmcf_frs_build(QUERIES), scanned from the points, coef_points = grad_out (the distance test
 *                 is bit-symmetric in its two arguments, so the pairs are the forward's);
 *   points and queries the same array: ONE call with coef_queries = coef_points = grad_out.
 * dw/d(d^2) = w'(s) / radius^2 at s = d^2 / radius^2 for the named windows (poly6: -3 (1 - s)^2 / radius^2), 1 for
 * DMCF_WINDOW_EXPLICIT (the sum of squared distances), and follows autodiff of utils/tools/losses.py:8-44 where a formula is
 * clamped.  DMCF_WINDOW_NONE, the count, has no gradient: DMCF_EUNSUPPORTED.  The sqrt-based windows (cubic, linear, peak,
 * cubic_grad) are singular at d^2 = 0, where the reference's autodiff yields NaN for the pair of a point with itself: HERE A
 * COINCIDENT PAIR (d^2 == 0) CONTRIBUTES 0.
 * flags: DMCF_FRS_IGNORE_QUERY_POINT as in the forward.  The DMCF_FRS_OPEN3D_* flags make the pair set asymmetric, so the swap
 * of roles above would not reproduce the forward's pairs: DMCF_EUNSUPPORTED (differentiate on the explicit pair list).
 * No atomics: identical calls give identical bits.  Arguments are validated before anything is enqueued. */
int dmcf_frs_window_sum_backward(const float* queries, int64_t n_queries, int64_t n_points, float radius, int flags, int window,
                                 const float* coef_queries, const float* coef_points, const void* workspace,
                                 size_t workspace_bytes, float* grad, dmcf_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Radius search: one radius per query.  Replaces ml3d.layers.RadiusSearch(metric='L2', ignore_query_point,
 * return_distances, normalize_distances)(points, queries, radii)  (utils/convolutions.py:212-216, 366-370 and
 * 1006-1010: the layers' branch for extents of rank 1, radii = 0.5 * extents).
 * Result contract: for every query i the SET
 *   { j : ((dx*dx + dy*dy) + dz*dz) <= r_i*r_i },  r_i = radii[i]     float32, un-fused, inclusive,
 * minus points whose coordinates equal the query's when DMCF_FRS_IGNORE_QUERY_POINT is set.  Rows come out in the order of
 * dmcf_frs_write (ascending grid cell, then ascending point index); neighbors_distance holds SQUARED distances (the
 * library's normalize_distances -- d^2 / r_i^2 for L2 -- is the caller's job).  pair_capacity: as for dmcf_frs_write.
 * A radius that is negative, NaN or larger than max_radius gives an empty row.
 * Uses the workspace of dmcf_frs_build(points, n_points, max_radius): max_radius MUST be the radius of that build, the
 * grid's cells are sized for it and every query scans cells of that size (a query of radius r visits ~(r + cell)^3 of them).
 * flags: DMCF_FRS_IGNORE_QUERY_POINT only.  The DMCF_FRS_OPEN3D_* flags are DMCF_EINVAL: they emulate the hash walk of
 * FixedRadiusSearch, and Open3D's RadiusSearch is a different structure (a KD-tree).
 * ---------------------------------------------------------------------------------------------- */
int dmcf_radius_search_count(const float* queries, int64_t n_queries, int64_t n_points, const float* radii,
                             float max_radius, int flags, void* workspace, size_t workspace_bytes,
                             int64_t* row_splits, dmcf_stream_t stream);
int dmcf_radius_search_write(const float* queries, int64_t n_queries, int64_t n_points, const float* radii,
                             float max_radius, int flags, const void* workspace, size_t workspace_bytes,
                             const int64_t* row_splits, int32_t* neighbors_index, float* neighbors_distance,
                             int64_t pair_capacity, dmcf_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Batched search (ABI 2.20): the points_row_splits / queries_row_splits arguments of ml3d.layers.FixedRadiusSearch and
 * ml3d.layers.RadiusSearch.  `points` holds the point sets of `batch` items one after the other, item b being
 * points[points_row_splits[b] .. points_row_splits[b + 1]); `queries` likewise with queries_row_splits.  Both row-splits
 * arrays are DEVICE int64 [batch + 1], start at 0, do not decrease and end at n_points / n_queries; the caller vouches for
 * that (they cannot be read here without a host round trip).  Arrays that break the promise give wrong rows, never an access
 * outside the workspace.  Items may be empty.
 * Result contract: a query of item b finds exactly the points j of item b with ((dx*dx + dy*dy) + dz*dz) <= r*r -- the value
 * and the test of the un-batched searches -- wherever the items lie: they may overlap or coincide.  neighbors_index indexes
 * the concatenated `points`, row_splits runs over all queries, DMCF_FRS_IGNORE_QUERY_POINT is decided by position equality,
 * rows are deterministic (ascending grid cell of the item's slab, then ascending point index).
 * One grid geometry serves the whole call -- its box and cell edge come from all points together -- with the item as the
 * outermost digit of the cell index (dmcf_amd/csrc/frs.hip); no host round trip in the build.  A structure built here is
 * searched with the *_batched entry points only, with the same n_points, batch and radius, and a workspace of
 * dmcf_frs_workspace_bytes_batched (0 for a negative size or a batch outside [1, 2^26]).
 * A single point set is a batch of one item: the un-batched entry points run the same host code and the same kernels per
 * phase (the instantiation that takes the item as 0 and reads no row splits), and dmcf_frs_build_batched(points, [0, n])
 * leaves the bytes of dmcf_frs_build's general path.  The two families keep their own argument validation.
 * flags: DMCF_FRS_IGNORE_QUERY_POINT only.  The DMCF_FRS_OPEN3D_* flags are DMCF_EINVAL, DMCF_FRS_METRIC_LINF is
 * DMCF_EUNSUPPORTED (DMCF_EINVAL in the radius search, as in dmcf_radius_search_count).  Null row splits and a batch outside
 * [1, 2^26] are DMCF_EINVAL.  Arguments are validated before anything is enqueued.  Otherwise every argument is the one of
 * the un-batched entry point of the same name.
 * ---------------------------------------------------------------------------------------------- */
size_t dmcf_frs_workspace_bytes_batched(int64_t n_points, int64_t n_queries, int64_t batch);
int dmcf_frs_build_batched(const float* points, int64_t n_points, const int64_t* points_row_splits, int64_t batch, float radius,
                           void* workspace, size_t workspace_bytes, dmcf_stream_t stream);
int dmcf_frs_count_batched(const float* queries, int64_t n_queries, const int64_t* queries_row_splits, int64_t batch,
                           int64_t n_points, float radius, int flags, void* workspace, size_t workspace_bytes,
                           int64_t* row_splits, dmcf_stream_t stream);
int dmcf_frs_write_batched(const float* queries, int64_t n_queries, const int64_t* queries_row_splits, int64_t batch,
                           int64_t n_points, float radius, int flags, const void* workspace, size_t workspace_bytes,
                           const int64_t* row_splits, int32_t* neighbors_index, float* neighbors_distance,
                           int64_t pair_capacity, dmcf_stream_t stream);
/* a radius per query on the structure of dmcf_frs_build_batched(points, ..., max_radius) */
int dmcf_radius_search_count_batched(const float* queries, int64_t n_queries, const int64_t* queries_row_splits, int64_t batch,
                                     int64_t n_points, const float* radii, float max_radius, int flags, void* workspace,
                                     size_t workspace_bytes, int64_t* row_splits, dmcf_stream_t stream);
int dmcf_radius_search_write_batched(const float* queries, int64_t n_queries, const int64_t* queries_row_splits, int64_t batch,
                                     int64_t n_points, const float* radii, float max_radius, int flags, const void* workspace,
                                     size_t workspace_bytes, const int64_t* row_splits, int32_t* neighbors_index,
                                     float* neighbors_distance, int64_t pair_capacity, dmcf_stream_t stream);

/* The window sum and its gradient on the structure of dmcf_frs_build_batched (ABI 2.22): dmcf_frs_window_sum and
 * dmcf_frs_window_sum_backward with the sums of a query running over the points of the query's OWN item only.  The arguments
 * are the un-batched ones with (queries_row_splits, batch) after n_queries; coef_points is indexed by the point's index in
 * the concatenated array.  For the gradient w.r.t. the points, build the batched structure over the QUERIES (with the
 * queries' row splits) and scan it from the points with the points' row splits.
 * item_max (forward only; may be NULL): DEVICE float [batch], receives the largest out[q] of every item; the entry point
 * clears it first, so an item without queries gives 0.  Lane 0 of a query's wave raises it with an integer atomic max on the
 * float's bits, which orders non-negative floats only: with DMCF_WINDOW_CUBIC_GRAD, whose sums can be negative, a non-NULL
 * item_max is DMCF_EUNSUPPORTED.  A maximum does not depend on the order of the atomics: identical calls give identical bits.
 * The backward uses no atomics at all.
 * flags: DMCF_FRS_IGNORE_QUERY_POINT only; DMCF_FRS_OPEN3D_* are DMCF_EINVAL, DMCF_FRS_METRIC_LINF is DMCF_EUNSUPPORTED.
 * batch outside [1, 2^26], NULL row splits and a window id out of range are DMCF_EINVAL; in the backward both coefficient
 * arrays NULL are DMCF_EINVAL and DMCF_WINDOW_NONE is DMCF_EUNSUPPORTED; a workspace below
 * dmcf_frs_workspace_bytes_batched(n_points, n_queries, batch) is DMCF_EWORKSPACE; n_queries == 0 is DMCF_OK without a
 * kernel launch.  Arguments are validated before anything is enqueued. */
int dmcf_frs_window_sum_batched(const float* queries, int64_t n_queries, const int64_t* queries_row_splits, int64_t batch,
                                int64_t n_points, float radius, int flags, int window, const void* workspace,
                                size_t workspace_bytes, float* out, float* item_max, dmcf_stream_t stream);
int dmcf_frs_window_sum_backward_batched(const float* queries, int64_t n_queries, const int64_t* queries_row_splits,
                                         int64_t batch, int64_t n_points, float radius, int flags, int window,
                                         const float* coef_queries, const float* coef_points, const void* workspace,
                                         size_t workspace_bytes, float* grad, dmcf_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Continuous convolution (CConv) and its antisymmetric variant (ASCC).
 * Replaces ml3d.ops.continuous_conv(filters, out_positions, extents[1,1], offset=0, inp_positions,
 * inp_features, inp_importance, neighbors_index, neighbors_row_splits, neighbors_importance,
 * align_corners, coordinate_mapping, interpolation, normalize)  (utils/convolutions.py:414-431):
 *     out[i,:] = 1/psi_i * sum_{p in row i} a_p * s_j * sum_c f_j[c] * g(Lambda(x_j - x_i))[c,:]
 * with j = neighbors_index[p], a_p the per-neighbour importance, s_j the per-point importance,
 * psi_i = sum_p a_p when DMCF_FLAG_NORMALIZE (else 1).
 * With DMCF_FLAG_SYMMETRIC the call computes the whole ASCC layer body
 * (utils/convolutions.py:410-412 and 433-458) in one pass:
 *     g = concat([-flip_zyx(filters), filters], axis=sym_axis);
 *     out[i,:] = sum_p a_p * sum_c (f_j[c] + f_i[c]) * g(Lambda(x_j - x_i))[c,:]
 * which requires the output points to be the input points 0..n_out-1 (the reference passes the same set
 * for both, models/sym_net.py:66; n_inp > n_out is the sharded case: owned points first, ghosts after).
 * ---------------------------------------------------------------------------------------------- */
enum dmcf_mapping {
    DMCF_MAP_BALL_TO_CUBE_RADIAL = 0,
    DMCF_MAP_BALL_TO_CUBE_VOLUME_PRESERVING = 1,
    DMCF_MAP_IDENTITY = 2
};
enum dmcf_interpolation { DMCF_INTERP_LINEAR = 0, DMCF_INTERP_LINEAR_BORDER = 1, DMCF_INTERP_NEAREST = 2 };
/* how the per-neighbour importance a_p is obtained from `neighbors_value` */
enum dmcf_window {
    DMCF_WINDOW_NONE = 0,       /* a_p = 1; neighbors_value ignored (may be NULL) */
    DMCF_WINDOW_EXPLICIT = 1,   /* a_p = neighbors_value[p] (user supplied importance) */
    /* a_p = w(q), q = neighbors_value[p] / radius^2, neighbors_value = squared distances
     * (utils/convolutions.py:359-362, 375-379; formulas utils/tools/losses.py:8-44).
     * neighbors_value == NULL: the squared distance is re-formed from the two positions, with the operations and the order
     * dmcf_frs_write / dmcf_frs_search_padded use for the distances they return -- bit-identical results, and the list needs
     * no distance array. */
    DMCF_WINDOW_POLY6 = 2,
    DMCF_WINDOW_CUBIC = 3,
    DMCF_WINDOW_LINEAR = 4,
    DMCF_WINDOW_PEAK = 5,
    DMCF_WINDOW_CUBIC_GRAD = 6
};
#define DMCF_FLAG_ALIGN_CORNERS 1
#define DMCF_FLAG_NORMALIZE 2
#define DMCF_FLAG_SYMMETRIC 4  /* ASCC: filters is the stored half kernel, see above */
#define DMCF_FLAG_ACCUMULATE 8 /* out += result instead of out = result (add_merge, models/hrnet.py:115-116) */
#define DMCF_FLAG_FILTER_PACKED 32 /* the caller's promise that `workspace` still holds what the previous dmcf_cconv_forward with
                                      the SAME filters (values included), filter_dims, flags & (SYMMETRIC | sym_axis) and kernel
                                      choice (dmcf_cconv_kernel_name returns the same string for both calls) left there: the
                                      filter is not packed again (one launch less per layer; inference weights do not change from
                                      step to step, and a step of a 2,000-particle scene is paced by its launches).  The library
                                      keeps no state: whoever sets the flag owns the workspace between the calls. */
#define DMCF_FLAG_SKIP_SELF 16 /* pairs with neighbors_index[p] == the output row -- and pairs whose two positions are EQUAL, which
                                  is the test the search applies (ignore_query_point drops every point at the query position) --
                                  carry weight zero: a list searched WITH the query points serves a layer that ignores them (radius_search_ignore_query_points,
                                  utils/convolutions.py:207-210) when its outputs are its first n_out inputs -- the ASCC
                                  head then shares the list of the trunk's same-scale layers instead of searching again.
                                  Only the kernel for <= 4 output channels and large filters implements it
                                  (dmcf_cconv_kernel_name: "cconv_direct_kernel..."); DMCF_EUNSUPPORTED otherwise */

typedef struct dmcf_cconv_args {
    const float* filters;      /* [D,H,W,Cin,Cout]; with SYMMETRIC: dims[sym_axis] is the stored half size */
    int32_t filter_dims[5];    /* D(z), H(y), W(x), Cin, Cout of `filters` as passed */
    int32_t sym_axis;          /* 0..2, index into (z,y,x); only with DMCF_FLAG_SYMMETRIC */
    const float* out_positions; /* [n_out,3] */
    int64_t n_out;
    const float* inp_positions; /* [n_inp,3] */
    int64_t n_inp;
    const float* inp_features;   /* [n_inp,Cin] */
    const float* inp_importance; /* [n_inp] or NULL (always NULL in DMCF: models/hrnet.py:91-92) */
    const int32_t* neighbors_index;       /* [P] */
    const int64_t* neighbors_row_splits;  /* [n_out+1] */
    const float* neighbors_value;         /* [P] squared distances (or NULL) or importances, see dmcf_window */
    float extent;              /* scalar filter extent (diameter); radius = extent/2 */
    float window_fac;          /* multiplier of the window function ("fac", losses.py:8), normally 1 */
    int32_t window;            /* enum dmcf_window */
    int32_t coordinate_mapping; /* enum dmcf_mapping */
    int32_t interpolation;      /* enum dmcf_interpolation */
    int32_t flags;              /* DMCF_FLAG_* */
    const float* bias;          /* [Cout] or NULL; added after normalisation (convolutions.py:466-467) */
    float* out;                 /* [n_out,Cout] */
    int64_t n_pairs;            /* entries in neighbors_index / neighbors_value (>= P = neighbors_row_splits[n_out]);
                                 * rows reaching past it are treated as empty (see dmcf_frs_write pair_capacity) */
    const int32_t* neighbors_row_count; /* optional [n_out]: PADDED lists as written by dmcf_frs_search_padded -- row i is
                                   neighbors_index[row_splits[i] .. row_splits[i] + row_count[i]); NULL = CSR rows
                                   [row_splits[i], row_splits[i+1]) */
    uint32_t filter_tile_mask; /* optional hint about filter blocks that are ALL ZERO (the block-diagonal filters of two layers
                                  launched as one, models/hrnet.py:85-92 twice on one list): bit 4 * (c / 4) + o / 16 is set
                                  when input channels 4 (c / 4) .. + 3 have a non-zero weight into output channels
                                  16 (o / 16) .. + 15 in some filter cell (c < 32, o < 64).  0 = no hint (every block is
                                  multiplied).  Kernels may skip the fetch and the products of unset blocks; results are
                                  identical for finite features (a skipped product is an exact zero). */
    int32_t row_length_hint;   /* optional, a property of the LAYER the caller knows from its configuration (the dispatch never
                                  looks at the neighbour list itself: the same step gives the same bits on CSR and on padded
                                  lists): 0 = unknown, 1 = rows of tens of neighbours (a layer at the network's base radius,
                                  models/hrnet.py:86 with inp_scale = out_scale = 0), 2 = rows of hundreds or more (any wider
                                  radius).  With 2, layers of 17 .. 32 input channels and 4 x 4 x 4 filters take the
                                  pair-per-instruction kernel ("cconv_pair_kernel..."), which needs long rows to pay for
                                  its per-point merge; with 1, layers of 24 .. 32 input channels and at most 32 output
                                  channels take the wave-specialised kernel ("cconv_ws_kernel...": that splat in producer
                                  waves, the contraction in consumer waves of a persistent workgroup), which pays when a
                                  row's contraction is as much work as its splat. */
} dmcf_cconv_args;

size_t dmcf_cconv_workspace_bytes(const dmcf_cconv_args* args);

int dmcf_cconv_forward(const dmcf_cconv_args* args, void* workspace, size_t workspace_bytes,
                       dmcf_stream_t stream);
/* Diagnostics: the name of the device kernel dmcf_cconv_forward dispatches these arguments to (the dispatch looks at the
 * layer -- filter shape, channel counts, flags -- never at the neighbour list), as rocprofv3 prints it without the
 * namespace, e.g. "cconv_z3_kernel<1, true>".  bench.py groups its per-launch HIP-event timings by it.  The same selection
 * as dmcf_cconv_forward's, so also the same code where that one dispatches nowhere: DMCF_EUNSUPPORTED for DMCF_FLAG_SKIP_SELF on
 * arguments the direct kernel does not take (`name` is then left as it was). */
int dmcf_cconv_kernel_name(const dmcf_cconv_args* args, char* name, size_t name_bytes);

/* CConv with INDIVIDUAL extents: ml3d.ops.continuous_conv with extents of shape [n_out, 1] (utils/convolutions.py:397-399
 * after the rank-1 branch :366-370).  Output row i uses its own filter extent e_i = out_extents[i] (device, [n_out]):
 * Lambda maps x_j - x_i with 1 / e_i, and a distance window is evaluated on d^2 / (e_i / 2)^2.  args->extent is ignored.
 * Everything else is dmcf_cconv_forward's contract: every mapping / interpolation, ALIGN_CORNERS, NORMALIZE, ACCUMULATE,
 * windows (neighbors_value == NULL included), bias, padded lists (neighbors_row_count).
 *   SYMMETRIC  each pair is evaluated at the extent of its OUTPUT row: the two-pass form :433-458 with extents_rank2 =
 *              [n_out, 1].  Pair (i, j) and pair (j, i) then see different extents, so the layer no longer conserves
 *              momentum (models/sym_net.py:42-53 relies on equal extents).
 *   An extent that is not positive and finite gives a zero row (plus the bias).
 *   out_extents == NULL with n_out > 0: DMCF_EINVAL.  DMCF_FLAG_SKIP_SELF: DMCF_EUNSUPPORTED.  DMCF_FLAG_FILTER_PACKED is
 *   ignored (the call always packs the filter).
 * One generic kernel serves every call ("cconv_ext_kernel<CC>"); workspace: dmcf_cconv_workspace_bytes(args), which asks for
 * a positive args->extent (any value: the size does not depend on it). */
int dmcf_cconv_forward_extents(const dmcf_cconv_args* args, const float* out_extents, void* workspace,
                               size_t workspace_bytes, dmcf_stream_t stream);
/* the name of the kernel dmcf_cconv_forward_extents launches for these arguments (see dmcf_cconv_kernel_name) */
int dmcf_cconv_extents_kernel_name(const dmcf_cconv_args* args, char* name, size_t name_bytes);

/* ------------------------------------------------------------------------------------------------
 * Backward pass of dmcf_cconv_forward (training).  Replaces the gradients Open3D 0.15.2 registers for
 * ml3d.ops.continuous_conv: continuous_conv_backprop_filter (d filters) and invert_neighbors_list + continuous_conv_transpose
 * (d inp_features).  Positions, extents and importances get no gradient, as there.
 *
 * dmcf_invert_neighbors_list replaces ml3d.ops.invert_neighbors_list(num_points = n_inp, inp_neighbors_index,
 * inp_neighbors_row_splits, inp_neighbors_attributes): for every input point j the forward pairs that reference it.
 *   inv_row_splits [n_inp + 1]: row j = entries [inv_row_splits[j], inv_row_splits[j+1]); inv_row_splits[n_inp] = the pairs
 *                               of the list (rows reaching past n_pairs, as in dmcf_cconv_forward, and indices outside
 *                               [0, n_inp) are not pairs).  Inside a row: ascending forward pair index (deterministic).
 *   inv_index [n_pairs]         the output row i of each entry (-1 past inv_row_splits[n_inp])
 *   inv_pair  [n_pairs]         the forward pair index p of each entry (-1 past the end); required
 *   inv_values [n_pairs]        optional: values[p] permuted the same way (the attributes; NULL = not wanted)
 * neighbors_row_count: optional [n_out], padded lists as in dmcf_cconv_args.  A stable radix sort (rocPRIM) keyed by j.
 * ---------------------------------------------------------------------------------------------- */
size_t dmcf_invert_neighbors_list_workspace_bytes(int64_t n_pairs);
int dmcf_invert_neighbors_list(int64_t n_inp, const int32_t* neighbors_index, const int64_t* neighbors_row_splits,
                               const int32_t* neighbors_row_count, int64_t n_out, int64_t n_pairs, const float* values,
                               int32_t* inv_index, int64_t* inv_row_splits, int32_t* inv_pair, float* inv_values,
                               void* workspace, size_t workspace_bytes, dmcf_stream_t stream);

/* dmcf_cconv_backward(fwd, bwd): with the forward's arguments `fwd` (out, bias and DMCF_FLAG_ACCUMULATE / FILTER_PACKED are
 * ignored) and G = bwd->grad_out = dL/d out [n_out, Cout]:
 *     grad_inp_features[j,:] = sum_{p -> j} (a_p / psi_i) sum_c w_c(p) W_c G[i,:]          (continuous_conv_transpose)
 *     grad_filters[c]        = sum_p (a_p / psi_i) w_c(p) f_j (x) G[i]                      (continuous_conv_backprop_filter)
 * a_p the pair weight times s_j, psi_i the forward's normaliser (1 without NORMALIZE or where it is 0).  With SYMMETRIC (ASCC)
 * the pair features are f_j + f_i, grad_inp_features gets the centre term sum_p (a_p / psi_i) sum_c w_c(p) g_c G[i,:] as well,
 * and grad_filters is the gradient of the stored HALF kernel (the full kernel's gradient folded back:
 * dHalf = dFull[upper] - flip_zyx(dFull[lower])); n_inp != n_out (the sharded layout) is DMCF_EUNSUPPORTED.
 * Every option of dmcf_cconv_forward is supported: mappings, interpolations, ALIGN_CORNERS, windows (neighbors_value == NULL
 * included), NORMALIZE, inp_importance, SYMMETRIC, SKIP_SELF, padded lists.  Per-point extents: dmcf_cconv_backward_extents.
 * The geometry of each pair is formed as in the generic forward kernel; only the order of the sums differs.  No float
 * atomics: two identical calls give identical bits.  K * Cin and K * Cout above 16384 (K the full kernel's cells):
 * DMCF_EUNSUPPORTED.
 * ---------------------------------------------------------------------------------------------- */
#define DMCF_BWD_ACCUMULATE 1 /* grad_* += result instead of grad_* = result (a weight shared by several calls) */
typedef struct dmcf_cconv_backward_args {
    uint32_t struct_size;           /* sizeof(dmcf_cconv_backward_args) of the caller; smaller: DMCF_EINVAL */
    int32_t flags;                  /* DMCF_BWD_* */
    const float* grad_out;          /* [n_out, Cout] */
    const int32_t* inv_index;       /* dmcf_invert_neighbors_list of the forward list (needed for grad_inp_features only) */
    const int32_t* inv_pair;
    const int64_t* inv_row_splits;  /* [inv_n_rows + 1] */
    int64_t inv_n_rows;             /* must equal fwd->n_inp */
    int64_t inv_n_pairs;            /* entries inv_index / inv_pair hold */
    float* grad_filters;            /* shape of fwd->filters, or NULL = not wanted */
    float* grad_inp_features;       /* [n_inp, Cin], or NULL = not wanted */
} dmcf_cconv_backward_args;

size_t dmcf_cconv_backward_workspace_bytes(const dmcf_cconv_args* fwd, const dmcf_cconv_backward_args* bwd);
int dmcf_cconv_backward(const dmcf_cconv_args* fwd, const dmcf_cconv_backward_args* bwd, void* workspace,
                        size_t workspace_bytes, dmcf_stream_t stream);
/* Diagnostics: the device kernels dmcf_cconv_backward launches for these arguments, in launch order, separated by ';'
 * (names as rocprofv3 prints them without the namespace, e.g. "cconv_bwd_input") */
int dmcf_cconv_backward_kernel_names(const dmcf_cconv_args* fwd, const dmcf_cconv_backward_args* bwd, char* names,
                                     size_t name_bytes);

/* Backward pass of dmcf_cconv_forward_extents (ABI 2.15): dmcf_cconv_backward with INDIVIDUAL extents.  Every pair of output
 * row i is evaluated at e_i = out_extents[i] (device, [n_out]): 1 / e_i and 1 / (e_i / 2)^2, formed with the forward's
 * operations, take the place of the scalar's two constants, so the gradients are those of the function the forward computed.
 * The extents themselves get no gradient.  fwd->extent is ignored.  Everything else is dmcf_cconv_backward's contract: the same
 * options, the struct_size check, the K * Cin / K * Cout limits, no float atomics (two identical calls give identical bits),
 * and the workspace of dmcf_cconv_backward_workspace_bytes(fwd, bwd), which asks for a positive fwd->extent (any value: the
 * size does not depend on it).
 *   SYMMETRIC  each pair at the extent of its OUTPUT row, as in the forward: pair (i, j) and pair (j, i) see different extents;
 *              the centre term of row i uses e_i; grad_filters is folded onto the stored half as in dmcf_cconv_backward.
 *   A row whose extent is not positive and finite is an empty row, as in the forward: it adds nothing to grad_filters nor to
 *   any row of grad_inp_features (the centre term included), and its psi_i is 0.
 *   out_extents == NULL with n_out > 0: DMCF_EINVAL.  DMCF_FLAG_SKIP_SELF: DMCF_EUNSUPPORTED (the forward rejects it too).
 *   Every argument error is returned before anything is enqueued.
 * The kernels that form a pair's geometry run in their individual-extent form, which dmcf_cconv_backward_extents_kernel_names
 * reports with the suffix _ext ("cconv_bwd_norm_ext", "cconv_bwd_input_ext", "cconv_bwd_filter_splat_ext"); the others are
 * dmcf_cconv_backward's. */
int dmcf_cconv_backward_extents(const dmcf_cconv_args* fwd, const dmcf_cconv_backward_args* bwd, const float* out_extents,
                                void* workspace, size_t workspace_bytes, dmcf_stream_t stream);
int dmcf_cconv_backward_extents_kernel_names(const dmcf_cconv_args* fwd, const dmcf_cconv_backward_args* bwd, char* names,
                                             size_t name_bytes);

/* ------------------------------------------------------------------------------------------------
 * ml3d.ops.continuous_conv (utils/convolutions.py:414-431) FROM particles ONTO a coarse grid_pos lattice with few output
 * channels -- the layers models/hrnet.py:83-93 builds for (input scale 0, output scale >= 1) with layer_channels[..][scale] of
 * 4 or 8 (configs/Liquid3d.yml:11: [[16], [8], [4]] / [[32], [16], [8]]).  Same operator, other order of evaluation ("filter
 * first", input stationary; dmcf_amd/csrc/cconv_sct.hip):  G_j = f_j . W once per INPUT point, then per pair the trilinear
 * interpolation of G_j added into the output point.  It walks the TRANSPOSED neighbour list: row j = the output points within
 * extent / 2 of input point j -- the list FixedRadiusSearch returns for (points = out_positions, queries = inp_positions), which
 * holds the same pairs as the forward list when the search's neighbour set is symmetric (the default set of this library).
 * Sums are formed in 64-bit fixed point (a term c enters as round(c * 2^s), 2^s * max_j |f_j|_1 * max |W| <= 2^46, both maxima
 * formed on the device inside the call), so the result does not depend on the order of the additions: bit reproducible like
 * every other kernel here, with LDS and global atomics doing the adds.
 *
 * dmcf_cconv_scatter_plan (once per pair of point sets and radius; every layer between them shares it) counting-sorts the input
 * points by the block of block_cells^3 lattice cells they lie in (cell of a point = floor((x - out_positions[0]) / voxel)); all
 * outputs a block reaches lie in a box of (block_cells + 2 reach + 1)^3 lattice cells whose 64-bit accumulators live in LDS and
 * are flushed once per block.  No host round trip; points far outside the bulk (beyond a 128^3-block region around the mean) are
 * handled one by one.  `plan` is caller-owned device memory of dmcf_cconv_scatter_plan_bytes(n_inp) bytes.
 *
 * Restrictions (DMCF_EUNSUPPORTED otherwise): 4x4x4 filters, cout 4 or 8, cin <= 32, DMCF_WINDOW_NONE / POLY6 evaluated from the
 * positions, volume-preserving map, linear interpolation; flags: DMCF_FLAG_ALIGN_CORNERS (required) | DMCF_FLAG_ACCUMULATE;
 * block_cells + 2 reach + 1 <= 13 at cout 4 (11 at cout 8): the box must fit the CU's LDS.
 *
 * Two host-only queries (ABI 2.28: no device, no HIP call) answer what a caller would otherwise restate:
 * dmcf_cconv_scatter_reach(extent, voxel): the `reach` the plan made with this extent and voxel holds, and the value of that field
 *   of dmcf_cconv_scatter_args: ceilf(0.5f * extent / voxel - 1e-4f) in float32; 0 for an argument that is not positive and finite.
 * dmcf_cconv_scatter_kernel_name(filter_dims, block_cells, reach, name, name_bytes): the instantiation dmcf_cconv_scatter_forward
 *   launches for this filter shape and box, as a profiler prints it ("cconv_sct_kernel<4, 16>"); DMCF_EUNSUPPORTED where the
 *   shape or the box is outside the restrictions above, DMCF_EINVAL for block_cells or reach <= 0, a NULL filter_dims or a name
 *   buffer too short.  name == NULL with name_bytes == 0 asks only whether the form takes the shape.
 * workspace: dmcf_cconv_scatter_workspace_bytes (the 64-bit sums; zeroed by the call).  error_flag (optional device int32, the
 * caller zeroes it): set to 1 when a pair fell outside its block's box, i.e. the plan was not made from these positions,
 * voxel and radius -- the pair is then dropped.
 * ---------------------------------------------------------------------------------------------- */
size_t dmcf_cconv_scatter_plan_bytes(int64_t n_inp);
int dmcf_cconv_scatter_plan(const float* inp_positions, int64_t n_inp, const float* out_positions, int64_t n_out, float voxel,
                            float extent, int32_t block_cells, void* plan, size_t plan_bytes, dmcf_stream_t stream);
int32_t dmcf_cconv_scatter_reach(float extent, float voxel);
int dmcf_cconv_scatter_kernel_name(const int32_t filter_dims[5], int32_t block_cells, int32_t reach, char* name, size_t name_bytes);

typedef struct dmcf_cconv_scatter_args {
    const float* filters;          /* [4][4][4][cin][cout] */
    int32_t filter_dims[5];
    const float* out_positions;    /* [n_out][3], a lattice of spacing voxel */
    int64_t n_out;
    const float* inp_positions;    /* [n_inp][3] */
    int64_t n_inp;
    const float* inp_features;     /* [n_inp][cin] */
    const int32_t* t_index;        /* transposed list: output indices, row j = input point j */
    const int64_t* t_row_begin;    /* [n_inp + 1] CSR row splits, or [n_inp] row begins when t_row_count is given */
    const int32_t* t_row_count;    /* optional [n_inp] (padded rows); NULL = CSR */
    int64_t t_capacity;            /* entries t_index holds */
    const void* plan;              /* dmcf_cconv_scatter_plan's output for these positions */
    int32_t block_cells;           /* as passed to the plan */
    int32_t reach;                 /* dmcf_cconv_scatter_reach(extent, voxel), voxel as passed to the plan */
    float extent;
    float window_fac;
    int32_t window;
    int32_t flags;
    const float* bias;             /* [cout] or NULL */
    float* out;                    /* [n_out][cout] */
    int32_t* error_flag;
} dmcf_cconv_scatter_args;

size_t dmcf_cconv_scatter_workspace_bytes(const dmcf_cconv_scatter_args* args);
int dmcf_cconv_scatter_forward(const dmcf_cconv_scatter_args* args, void* workspace, size_t workspace_bytes,
                               dmcf_stream_t stream);

/* Backward pass of the scatter form (ABI 2.19; dmcf_amd/csrc/cconv_sct_bwd.inc): the gradients of the function
 * dmcf_cconv_scatter_forward computes, with respect to the filters and the input features, in the forward's order of evaluation
 * run backwards.  Per input point j one walk over row j of the TRANSPOSED list forms T_j[cell][o] = sum_pairs a_p w_k(p)
 * grad_out[i][o] (64 x cout values, in LDS), then grad_inp_features[j] = W . T_j and grad_filters += f_j (x) T_j on the matrix
 * cores: no list inversion, nothing of size pairs x channels in memory.  Positions get no gradient.
 *
 * `fwd` carries the forward's arguments.  plan, block_cells, reach, out, bias, error_flag and DMCF_FLAG_ACCUMULATE are ignored
 * (plan and out may be NULL: the backward needs no plan).  Restrictions as the forward's (DMCF_EUNSUPPORTED otherwise): 4x4x4
 * filters, cout 4 or 8, cin <= 32, DMCF_WINDOW_NONE / POLY6 evaluated from the positions, volume-preserving map, linear
 * interpolation, DMCF_FLAG_ALIGN_CORNERS required.  Row conventions as the forward's: CSR, or t_row_begin + t_row_count; a row
 * that reaches past t_capacity is empty.  Each pair's geometry is formed by the device functions the forward kernel calls.
 *
 * Sums into T_j are 64-bit fixed point, as the forward's: a term enters as round(term * 2^s), 2^s * max |grad_out| * max(1,
 * |window_fac|) <= 2^46, the maximum formed on the device inside the call.  The filter gradient is reduced from per-workgroup
 * partial sums in workgroup order, rows are assigned to workgroups statically, and the number of workgroups depends on n_inp
 * only: no float atomics, two identical calls return identical bits.
 *
 * grad_out must be aligned to 16 bytes (its rows of 4 or 8 floats are read with 16-byte loads).
 *
 * Every argument error is returned before anything is enqueued: DMCF_EINVAL for a NULL operand, grad_out == NULL or not aligned
 * to 16 bytes, both outputs NULL, n_out / n_inp <= 0, extent <= 0, struct_size smaller than the struct, flags != 0;
 * DMCF_EWORKSPACE for a workspace
 * smaller than dmcf_cconv_scatter_backward_workspace_bytes; DMCF_EINVAL for a missing workspace or one not aligned to 256
 * bytes.  Nothing is allocated. */
typedef struct dmcf_cconv_scatter_backward_args {
    uint32_t struct_size;        /* sizeof of the caller's struct; smaller: DMCF_EINVAL */
    int32_t flags;               /* must be 0 */
    const float* grad_out;       /* [n_out][cout], aligned to 16 bytes */
    float* grad_filters;         /* [4][4][4][cin][cout] or NULL; written in full */
    float* grad_inp_features;    /* [n_inp][cin] or NULL; written in full, zero rows for inputs without pairs */
} dmcf_cconv_scatter_backward_args;

size_t dmcf_cconv_scatter_backward_workspace_bytes(const dmcf_cconv_scatter_args* fwd, const dmcf_cconv_scatter_backward_args* bwd);
int dmcf_cconv_scatter_backward(const dmcf_cconv_scatter_args* fwd, const dmcf_cconv_scatter_backward_args* bwd,
                                void* workspace, size_t workspace_bytes, dmcf_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * ml3d.ops.continuous_conv (utils/convolutions.py:414-431) between two point sets on ALIGNED REGULAR LATTICES -- the
 * coarse scales of the multi-scale models: models/hrnet.py:85-92 convolves between the outputs of grid_pos
 * (utils/tools/losses.py:136-181, via get_dilated_pos :266-272), which share one centre and whose voxel sizes are integer
 * multiples of each other.  Input point j sits at centre + inp_cell_j * voxel, output point i at
 * centre + out_cell_i * (output spacing); every per-pair quantity of the operator depends only on the integer offset
 * of the input cell from the output point, so no neighbour list is needed: the caller passes the offsets inside the
 * radius, the input features laid out by lattice cell (a dense volume over the bounding box of the input lattice) and
 * a cell -> output point table of the output lattice.  Same filters / extent / window / mapping / interpolation /
 * ALIGN_CORNERS / bias / ACCUMULATE semantics as dmcf_cconv_forward; SYMMETRIC, NORMALIZE, DMCF_WINDOW_EXPLICIT and
 * importances are not supported (DMCF_EUNSUPPORTED: use the neighbour-list form).  Results agree with the neighbour-list
 * form to the rounding of the positions (the reference subtracts rounded positions, this form uses d * voxel).
 * ---------------------------------------------------------------------------------------------- */
typedef struct dmcf_lattice_conv_args {
    const float* filters;        /* [D,H,W,Cin,Cout] */
    int32_t filter_dims[5];
    const float* inp_volume;     /* [inp_dims z][y][x][Cin]: the input features by lattice cell, zeros where no point is */
    int32_t inp_min[3];          /* (x,y,z) cell of entry 0 of inp_volume, in units of the input lattice */
    int32_t inp_dims[3];         /* (x,y,z) */
    const int32_t* out_table;    /* [out_dims z][y][x]: index of the output point in that cell of the OUTPUT lattice, or -1 */
    int32_t out_min[3];          /* (x,y,z) cell of entry 0 of out_table, in units of the output lattice */
    int32_t out_dims[3];
    int64_t n_out;               /* rows of `out` */
    /* The launch covers the output cells  o = a * out_stride + out_phase  for the integer vectors a of the box
     * [base_min, base_min + base_dims); the stencil of such a cell is the input cells  a * inp_step + d.
     *   same lattice:            inp_step = out_stride = 1, phase 0;
     *   outputs 2x coarser:      inp_step = 2, out_stride = 1, phase 0;
     *   outputs 2x finer:        inp_step = 1, out_stride = 2, one launch per phase in {0,1}^3, and the output sits
     *                            rel_shift = phase * (output spacing) away from the input cell a * inp_step. */
    int32_t inp_step;
    int32_t out_stride;
    int32_t out_phase[3];
    int32_t base_min[3], base_dims[3];
    float rel_shift[3];          /* x_in - x_out = d * voxel - rel_shift */
    float voxel[3];              /* (x,y,z) spacing of the input lattice */
    const int32_t* offsets;      /* [n_offsets,4]: (dx,dy,dz,0) with |d * voxel - rel_shift| <= extent / 2 */
    int64_t n_offsets;
    int32_t reach[3];            /* max |d| per axis over `offsets`.  The volume must hold EVERY cell the launch can touch --
                                  * a * inp_step + d for a in the base box (its x extent rounded up to a multiple of 16)
                                  * and |d| <= reach -- so the kernel reads without bounds checks (DMCF_EINVAL otherwise):
                                  * the caller pads the volume with zero cells */
    float extent;
    float window_fac;
    int32_t window;              /* enum dmcf_window (applied to |d * voxel|^2 / radius^2) */
    int32_t coordinate_mapping;
    int32_t interpolation;
    int32_t flags;               /* DMCF_FLAG_ALIGN_CORNERS | DMCF_FLAG_ACCUMULATE */
    const float* bias;           /* [Cout] or NULL */
    float* out;                  /* [n_out,Cout]; rows of points that are in out_table are written */
} dmcf_lattice_conv_args;

size_t dmcf_lattice_conv_workspace_bytes(const dmcf_lattice_conv_args* args);
int dmcf_lattice_conv_forward(const dmcf_lattice_conv_args* args, void* workspace, size_t workspace_bytes,
                              dmcf_stream_t stream);
/* Up to 8 launches of the same layer (same filters, volume, output; e.g. the eight parity classes of outputs on the finer
 * lattice) as ONE grid: each alone is too small to fill the chip. */
size_t dmcf_lattice_conv_batch_workspace_bytes(const dmcf_lattice_conv_args* parts, int32_t n_parts);
int dmcf_lattice_conv_forward_batch(const dmcf_lattice_conv_args* parts, int32_t n_parts, void* workspace,
                                    size_t workspace_bytes, dmcf_stream_t stream);

/* Backward pass of the lattice form (ABI 2.16; dmcf_amd/csrc/cconv_lat_bwd.inc).  `parts` are exactly the structs of the
 * forward call: 1 for outputs on the same or a coarser lattice, up to 8 -- the parity classes of
 * dmcf_lattice_conv_forward_batch -- for outputs on the 2x finer lattice.  All parts share filters, inp_volume (pointer, min,
 * dims), the steps and n_out (DMCF_EINVAL otherwise); bias, out and DMCF_FLAG_ACCUMULATE are ignored (the bias gradient is a
 * column sum of grad_out the caller forms).  With out_i = sum_d W_d^T f_{cell(i)+d}:
 *   grad_volume  [inp_dims z][y][x][Cin] or NULL: df_v = sum_d W_d grad_out_{row of the output cell that reaches v through d};
 *                written in full, zero in cells nothing reaches;
 *   grad_filters [D][H][W][Cin][Cout] or NULL: the transpose of the forward's filter interpolation applied to
 *                dW_d = sum_i f_{cell(i)+d} (x) grad_out_i, summed over all parts; written in full.
 * Rows of grad_out whose point is not in out_table (or outside a part's base box) contribute nothing: the forward leaves those
 * rows untouched.  W_d are the forward's own matrices (same device code, same bits).  No float atomics: partial sums over
 * slabs of 1024 output rows go to buffers of their own and are added in slab order, the fold onto the filter walks parts and
 * offsets in ascending order -- two identical calls return identical bits.
 * Errors mirror the forward: DMCF_EUNSUPPORTED for the options it refuses (SYMMETRIC, NORMALIZE, DMCF_WINDOW_EXPLICIT,
 * Cin other than 4 or 8, Cout > 32) and for (inp_step, out_stride) other than (1,1), (2,1), (1,2); DMCF_EINVAL for n_parts
 * outside 1..8, parts that do not belong together, a volume that does not hold every reachable cell, grad_out == NULL with
 * n_out > 0, or both outputs NULL; DMCF_EWORKSPACE for a short workspace.  Nothing is allocated. */
size_t dmcf_lattice_conv_backward_workspace_bytes(const dmcf_lattice_conv_args* parts, int32_t n_parts);
int dmcf_lattice_conv_backward(const dmcf_lattice_conv_args* parts, int32_t n_parts, const float* grad_out,
                               float* grad_volume, float* grad_filters, void* workspace, size_t workspace_bytes,
                               dmcf_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * o3dml.ops.reduce_subarrays_sum(values, row_splits) (models/pbf_model.py:450-453):
 *   out[i] = sum(values[row_splits[i] : row_splits[i+1]]);  values == NULL means all ones.
 * ---------------------------------------------------------------------------------------------- */
int dmcf_reduce_subarrays_sum(const float* values, const int64_t* row_splits, int64_t n_rows, float* out,
                              dmcf_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * tf.keras.layers.Dense of the networks (models/pbf_model.py:134-152 fluid_dense / obs_dense, models/hrnet.py:49 the
 * same-scale branch :93-99, models/cconv.py:44):  out[n, m] = x[n, k] W[k, m] (+ bias[m]) (+ residual[n, m]) -- a million rows,
 * a few tens of columns: a wavefront keeps the filter as matrix-instruction fragments and walks 16-row tiles.  k a multiple of 4
 * up to 64, m up to 64, x 16-byte aligned; anything else: DMCF_EUNSUPPORTED (the caller keeps its library GEMM).  out may not
 * alias x; it may be the residual.
 * ---------------------------------------------------------------------------------------------- */
int dmcf_dense_forward(const float* x, int64_t n, int32_t k, const float* W, int32_t m, const float* bias,
                       const float* residual, float* out, dmcf_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * The fluid's axis-aligned bounding box, tf.reduce_min / reduce_max(pos, axis=0) of the boundary crop every step begins with
 * (models/pbf_model.py:330-336): out[0..2] = min x, y, z, out[3..5] = max.  n == 0: +inf / -inf.  A NaN coordinate makes both
 * bounds of its axis NaN, as the reference's reductions do.  Workspace: dmcf_points_aabb_workspace_bytes() bytes.
 * ---------------------------------------------------------------------------------------------- */
size_t dmcf_points_aabb_workspace_bytes(void);
int dmcf_points_aabb(const float* points, int64_t n, float* out, void* workspace, size_t workspace_bytes,
                     dmcf_stream_t stream);
/* ABI 2.21: the box of every item of a batch in one launch.  Item b is points[row_splits[b] .. row_splits[b + 1]) (row_splits:
 * DEVICE int64 [batch + 1], starting at 0, not decreasing, ending at n -- the caller has validated it); out [batch][6] as above.
 * A non-empty item's bounds are those of dmcf_points_aabb on its slice, bit for bit (NaN rule included); an EMPTY item gives
 * +3.0e38 / -3.0e38 -- the model's box of "no fluid" (models/pbf_model.py) -- not +-inf.  One workgroup per item, no workspace:
 * intended for items of up to ~1e5 points (a training batch); a larger item is a serial strided loop of that one workgroup.
 * batch < 1: DMCF_EINVAL. */
int dmcf_points_aabb_batched(const float* points, int64_t n, const int64_t* row_splits, int64_t batch, float* out,
                             dmcf_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Ghost selection of the block-sharded rollout (no reference counterpart: tum-pbs/DMCF has no distributed code -- SURVEY.md
 * section 8e; the caller is dmcf_amd/parallel.py): which points lie within a halo width of which axis-aligned block, for
 * several widths at once.
 *   level(i, b) = number of w with gap2(points[i], boxes[b]) <= widths2[w]     (widths2: HOST array, DESCENDING, <= 8 entries)
 *   list(w)     = for b = 0 .. n_boxes - 1 (<= 64): the i with level(i, b) > w, in ascending i
 * gap2 = squared Euclidean distance to the box, per axis max(lo - x, x - hi, 0), un-fused float32; boxes [n_boxes][6] =
 * lo x, y, z, hi x, y, z on the DEVICE, +-inf on open sides.
 *   count : totals[w * n_boxes + b] = entries box b contributes to list(w) (DEVICE int64)
 *   write : list(w) -> rows[list_start[w] ..) (DEVICE int64 point indices), at most list_capacity[w] entries (HOST arrays); must
 *           follow a count with the same arguments and the same workspace.
 * OWNERSHIP: n_widths == 1 with widths2[0] < 0 replaces the test by "lo <= x < hi on every axis" (half-open blocks: a point has one
 * owner); list(0) is then the stable order of the points by owning box and totals[b] the points box b owns.  A NaN or infinite
 * coordinate is in no box: the totals then sum to less than n.
 * Workspace: dmcf_ghost_workspace_bytes(n, n_boxes, n_widths).
 * ---------------------------------------------------------------------------------------------- */
size_t dmcf_ghost_workspace_bytes(int64_t n, int32_t n_boxes, int32_t n_widths);
int dmcf_ghost_count(const float* points, int64_t n, const float* boxes, int32_t n_boxes, const float* widths2, int32_t n_widths,
                     int64_t* totals, void* workspace, size_t workspace_bytes, dmcf_stream_t stream);
int dmcf_ghost_write(const float* points, int64_t n, const float* boxes, int32_t n_boxes, const float* widths2, int32_t n_widths,
                     int64_t* rows, const int64_t* list_start, const int64_t* list_capacity, void* workspace, size_t workspace_bytes,
                     dmcf_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * grid_pos(pos, voxel_size, centralize, pad, hyst) (utils/tools/losses.py:136-181; the coarse point sets of the
 * multi-scale models, called through get_dilated_pos :249-284): the corners of every voxel a particle touches
 * (with +-hyst hysteresis), de-duplicated in tf.unique order (first appearance in the candidate list), decoded to
 * positions.  Three phases because two sizes are data dependent:
 *   bounds : lattice origin (mean of the positions when `centralize` and `center` == NULL, else *center), integer
 *            bounding box of the candidates -> 64-byte header at the start of `workspace`:
 *              int32 minp[3], int32 dims[3], int64 cells (= dims product, -1 if a position is not finite),
 *              int64 total, float center[3]
 *            the caller reads `cells` and provides a table of that many uint32
 *   count  : fills the table, counts the lattice points -> header.total; the caller reads it and allocates out
 *   write  : out[total,3] float32
 * `voxel_size` is a HOST pointer to 3 floats (axes below 1e-5 collapse, :139-141); `center` a DEVICE pointer to 3
 * floats or NULL.  The same (positions, voxel_size, centralize, pad, hyst, workspace) must be passed to all
 * three calls.  Candidate ranks are 32-bit: 2 * n_points * (2 + 2 pad)^3 must stay below 2^32
 * (DMCF_EUNSUPPORTED otherwise).
 * SPARSE scenes (a few particles far from the rest: `cells` in the billions for a million occupied ones): pass
 * table_cells = -S to count / write, S a power of two >= twice the number of candidates 2 * n_points * (2 + 2 pad)^3 at most
 * occupied, and a table of 12 * S bytes: the kernels then hash the cell index into S slots (open addressing) instead of
 * indexing a dense table.  Same points, same order.
 * Workspace: dmcf_grid_pos_workspace_bytes(n_points), always queried, never assumed: it is the layout of the batched
 * phases below for ONE item, dmcf_grid_pos_workspace_bytes_batched(n_points, 1) -- since the two families share their
 * kernels and their layout the value is no longer what earlier builds of ABI 2.x returned (the header is still at
 * offset 0, its fields where they were).
 * ---------------------------------------------------------------------------------------------- */
size_t dmcf_grid_pos_workspace_bytes(int64_t n_points);
int dmcf_grid_pos_bounds(const float* positions, int64_t n_points, const float* voxel_size, int centralize,
                         const float* center, int pad, float hyst, void* workspace, size_t workspace_bytes,
                         dmcf_stream_t stream);
int dmcf_grid_pos_count(const float* positions, int64_t n_points, const float* voxel_size, int centralize, int pad,
                        float hyst, void* workspace, size_t workspace_bytes, void* cell_table, int64_t table_cells,
                        dmcf_stream_t stream);
int dmcf_grid_pos_write(const float* positions, int64_t n_points, const float* voxel_size, int centralize, int pad,
                        float hyst, void* workspace, size_t workspace_bytes, const void* cell_table, int64_t table_cells,
                        float* out, int64_t out_capacity, dmcf_stream_t stream);
/*
 * grid_pos with row splits (ABI 2.21): the three phases for a BATCH of point sets.  Item b is positions[row_splits[b] ..
 * row_splits[b + 1]); `row_splits` is a DEVICE int64 [batch + 1] array (starts at 0, does not decrease, ends at n_points: the
 * caller has validated it).  The result is the concatenation, item after item, of what the un-batched phases return for each
 * item's slice: item b's rows are BIT-IDENTICAL to them, values and order (tf.unique order within the item's own candidate
 * list).  Empty items are legal and contribute no rows.  The un-batched phases ARE these phases for one item: the same reduction
 * kernels (instantiated without the row-split loads for the un-batched entry points), one workspace layout, one host function
 * per phase; only the pass over the candidates is a kernel of its own for one item.
 *   bounds : per item the lattice origin (the item's own mean, summed over the item's local index with the block count a call
 *            on the item alone launches; or
 *            centers[b], `centers` a DEVICE [batch][3] array or NULL) and the item's own integer box ->
 *            `batch` 64-byte headers at the start of `workspace`, each laid out as above.  An item's cell index is local to
 *            its own box and offset by the cells of the items before it: two items at the same coordinates never share a cell.
 *            The caller reads the headers: the dense table has sum_b max(cells_b, 0) uint32; cells_b = -1: item b holds a
 *            position that is not finite.
 *   count  : fills the table; header b's `total` = lattice points of item b; out_row_splits (DEVICE int64 [batch + 1]) =
 *            their exclusive prefix sum, the row splits of the output
 *   write  : out[out_row_splits[batch], 3]
 * Hashed table: table_cells = -S as above, the key is the offset cell index (item and cell).  The candidate ranks of all items
 * share the 32 bits: 2 * n_points * (2 + 2 pad)^3 < 2^32 for the whole batch.  batch < 1: DMCF_EINVAL; batch > 65535:
 * DMCF_EUNSUPPORTED (the workspace size function then returns 0).  Workspace: dmcf_grid_pos_workspace_bytes_batched.
 */
size_t dmcf_grid_pos_workspace_bytes_batched(int64_t n_points, int64_t batch);
int dmcf_grid_pos_bounds_batched(const float* positions, int64_t n_points, const int64_t* row_splits, int64_t batch,
                                 const float* voxel_size, int centralize, const float* centers, int pad, float hyst,
                                 void* workspace, size_t workspace_bytes, dmcf_stream_t stream);
int dmcf_grid_pos_count_batched(const float* positions, int64_t n_points, const int64_t* row_splits, int64_t batch,
                                const float* voxel_size, int centralize, int pad, float hyst, void* workspace,
                                size_t workspace_bytes, void* cell_table, int64_t table_cells, int64_t* out_row_splits,
                                dmcf_stream_t stream);
int dmcf_grid_pos_write_batched(const float* positions, int64_t n_points, const int64_t* row_splits, int64_t batch,
                                const float* voxel_size, int centralize, int pad, float hyst, void* workspace,
                                size_t workspace_bytes, const void* cell_table, int64_t table_cells, float* out,
                                int64_t out_capacity, dmcf_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * farthest_point_sample(npoint, inp[1,n,3]) and gather_point(inp, idx) (utils/tools/sampling.py / sampling.cu:125-201):
 * the sub-sampling of get_dilated_pos for multi-scale configs without voxel_size (utils/tools/losses.py:274-282) and
 * the index lists of HRNet's cross-scale Dense branch (models/hrnet.py:100-113).  One point set per call (the
 * reference's batch dimension is always 1 on this path).  sample_index[0] = 0; sample j maximises the float32
 * squared distance to samples 0..j-1; equal maxima resolve as in the reference's 512-thread kernel (smallest
 * index mod 512, then smallest index).  Sequential in the samples by definition: O(n_points * n_samples).
 * ---------------------------------------------------------------------------------------------- */
size_t dmcf_fps_workspace_bytes(int64_t n_points);
int dmcf_farthest_point_sample(const float* points, int64_t n_points, int64_t n_samples, void* workspace,
                               size_t workspace_bytes, int32_t* sample_index, dmcf_stream_t stream);
int dmcf_gather_point(const float* inp, const int32_t* index, int64_t n_index, int channels, float* out,
                      dmcf_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Validation metrics (pipelines/simulator.py:167-285, run_valid): the reference's custom CUDA ops
 * utils/tools/nn_distance.py:nn_distance (Chamfer, utils/evaluation_helper.py:25-28) and
 * utils/tools/tf_approxmatch.py:approx_match / match_cost (EMD, utils/tools/losses.py:401-409).
 * Point sets are float32 [b, n, 3] / [b, m, 3] (2-D scenes: z = 0).  Every pass is a row-parallel reduction over the other
 * set, spread over the whole device (rows x column splits), with per-split partials combined in a fixed order: no float
 * atomics, and the split plan depends on the sizes only, so two identical calls give identical bits.  b = 0: DMCF_OK,
 * nothing enqueued.  The workspace is the caller's; its size comes from the matching *_workspace_bytes query.
 * ---------------------------------------------------------------------------------------------- */
/* nn_distance(xyz1, xyz2) (nn_distance.py:40-53): dist1 [b, n] = squared distance from each point of xyz1 to its nearest
 * point of xyz2, idx1 [b, n] its index; dist2 / idx2 [b, m] the same from xyz2 to xyz1.  Equal distances: the lowest index.
 * A direction is skipped when both its pointers are NULL (one NULL of a pair, or both directions skipped: DMCF_EINVAL).
 * Squared distances in float32 as (dx*dx + dy*dy) + dz*dz without fused multiply-adds.  n or m == 0 with b > 0, or
 * b > 65535: DMCF_EINVAL. */
size_t dmcf_nn_distance_workspace_bytes(int64_t b, int64_t n, int64_t m);
int dmcf_nn_distance(const float* xyz1, const float* xyz2, int64_t b, int64_t n, int64_t m, float* dist1, int32_t* idx1,
                     float* dist2, int32_t* idx2, void* workspace, size_t workspace_bytes, dmcf_stream_t stream);
/* nn_distance over a RAGGED batch (ABI 2.23): `batch` items of different sizes in one call.  xyz1 [n_total, 3] and xyz2
 * [m_total, 3] hold the items' point sets one after the other; item b is xyz1[row_splits1[b] .. row_splits1[b + 1]) against
 * xyz2[row_splits2[b] .. row_splits2[b + 1]).  Both row-splits arrays are HOST int64 [batch + 1] and are validated here, before
 * anything is enqueued: they start at 0, do not decrease and end at n_total / m_total.  (The *_batched searches take DEVICE row
 * splits the caller vouches for.  Here the kernel reads no row splits at all: the entry point cuts every item's rows into
 * tiles of 64, writes one 16-byte record per tile -- its rows and its item's range of the other set -- from the validated
 * splits and copies that table into the workspace, so nothing on the device can disagree with what was checked.)
 * Result contract: dist1 [n_total] / idx1 [n_total] hold, for every row, what dmcf_nn_distance gives for its item alone, bit
 * for bit -- (dx*dx + dy*dy) + dz*dz un-fused, a strict < over the columns in ascending order, so equal distances go to the
 * lowest index -- with idx1 = the per-item index + row_splits2[b], the row in the concatenated xyz2; dist2 / idx2 [m_total]
 * the same from xyz2 to xyz1.  A direction is skipped when both its pointers are NULL (one NULL of a pair, or both directions
 * skipped: DMCF_EINVAL).  One launch per wanted direction, one wavefront per tile walking its item's other set through LDS: no
 * combine pass, no atomics, nothing that depends on the device, so identical calls give identical bits.  Sized for many items
 * of tens to a few thousand rows; an item of any size is correct, but one large set is dmcf_nn_distance's case.
 * An item with both sets empty contributes nothing; an item with exactly ONE empty set is DMCF_EINVAL (as n == 0 || m == 0
 * is above).  batch == 0 with n_total == m_total == 0, or every item empty: DMCF_OK, nothing enqueued.  batch < 0 or > 2^26,
 * NULL row splits, n_total or m_total >= 2^31 - 257: DMCF_EINVAL.  Workspace: dmcf_nn_distance_ragged_workspace_bytes (0 for a
 * negative size or a batch outside [1, 2^26]); the table reaches it by one asynchronous copy from pageable host memory. */
size_t dmcf_nn_distance_ragged_workspace_bytes(int64_t n_total, int64_t m_total, int64_t batch);
int dmcf_nn_distance_ragged(const float* xyz1, int64_t n_total, const int64_t* row_splits1, const float* xyz2, int64_t m_total,
                            const int64_t* row_splits2, int64_t batch, float* dist1, int32_t* idx1, float* dist2, int32_t* idx2,
                            void* workspace, size_t workspace_bytes, dmcf_stream_t stream);
/* approx_match(xyz1, xyz2, n, m) (tf_approxmatch.py:40-54): match [b, m, n] of the approximate EMD assignment (the algorithm
 * is restated in dmcf_amd/csrc/metrics.hip: ten levels of three all-pairs passes, __expf weights, the reference's 1e-9 terms,
 * clamps and integer division).  count1 / count2: HOST arrays of b int32 point counts (n_i <= n, m_i <= m; NULL = all
 * n / m), validated before anything is enqueued; rows and columns past a count are 0 and play no part.  The workspace is
 * O(n + m) and is reused by the batch items, which run one after another. */
size_t dmcf_approx_match_workspace_bytes(int64_t b, int64_t n, int64_t m);
int dmcf_approx_match(const float* xyz1, const float* xyz2, int64_t b, int64_t n, int64_t m, const int32_t* count1,
                      const int32_t* count2, float* match, void* workspace, size_t workspace_bytes, dmcf_stream_t stream);
/* match_cost(xyz1, xyz2, match) (tf_approxmatch.py:60-69): cost [b] = sum_{l,k} match[l, k] * |xyz2[l] - xyz1[k]|. */
size_t dmcf_match_cost_workspace_bytes(int64_t b, int64_t n, int64_t m);
int dmcf_match_cost(const float* xyz1, const float* xyz2, int64_t b, int64_t n, int64_t m, const float* match, float* cost,
                    void* workspace, size_t workspace_bytes, dmcf_stream_t stream);
/* match_cost(approx_match(...)) fused (the cost of emd_loss, losses.py:401-409): pass C adds w_kl * |d_kl| into per-row
 * partials instead of forming match, so memory stays O(n + m) (a dense match at n = m = 1e5 would be 40 GB).  Same
 * arguments as dmcf_approx_match; cost [b]. */
size_t dmcf_emd_workspace_bytes(int64_t b, int64_t n, int64_t m);
int dmcf_emd(const float* xyz1, const float* xyz2, int64_t b, int64_t n, int64_t m, const int32_t* count1, const int32_t* count2,
             float* cost, void* workspace, size_t workspace_bytes, dmcf_stream_t stream);
/* dmcf_emd over a RAGGED batch (ABI 2.24): `batch` items of different sizes in one call, laid out as for
 * dmcf_nn_distance_ragged -- xyz1 [n_total, 3], xyz2 [m_total, 3], item b being xyz1[row_splits1[b] .. row_splits1[b + 1])
 * against xyz2[row_splits2[b] .. row_splits2[b + 1]), both row-splits arrays HOST int64 [batch + 1], validated here before
 * anything is enqueued.  Result contract: cost[b] has exactly the bits dmcf_emd gives for item b alone (b = 1, no counts).
 * Every item keeps the column chunks of its own split plan, the column order inside a chunk, the split-order sums of the
 * finish steps, the multipliers (integer division included) and the order of the final sum; what changes is that each pass,
 * each finish step, the init and the totals are ONE launch over the tiles or rows of all items, so the call enqueues one
 * table copy and 62 launches whatever the batch (dmcf_emd: 62 per item).  The entry point writes the tables -- a record per
 * (item, 256 rows, column chunk), per (item, 256 rows) and per item -- from the validated splits and copies them into the
 * workspace in one asynchronous copy from pageable host memory; no kernel reads row splits, and no float atomics are used.
 * An item with either set empty costs 0 (as a zero count does in dmcf_emd; dmcf_nn_distance_ragged refuses such an item).
 * batch == 0 with n_total == m_total == 0: DMCF_OK.  Every item empty on both sides (n_total == m_total == 0): DMCF_OK with
 * nothing enqueued and no pointer but the splits looked at -- cost is NOT written, the caller holds its zeros.  batch < 0 or
 * > 2^26, NULL or malformed row splits, n_total or m_total >= 2^31 - 257, NULL cost or workspace, NULL points of a non-empty
 * set: DMCF_EINVAL.  The workspace holds the tables, five state arrays over the concatenated rows and the partials of every
 * item's plan, which is why its query takes the splits; the query returns 0 for arguments the call refuses. */
size_t dmcf_emd_ragged_workspace_bytes(int64_t n_total, const int64_t* row_splits1, int64_t m_total, const int64_t* row_splits2,
                                       int64_t batch);
int dmcf_emd_ragged(const float* xyz1, int64_t n_total, const int64_t* row_splits1, const float* xyz2, int64_t m_total,
                    const int64_t* row_splits2, int64_t batch, float* cost, void* workspace, size_t workspace_bytes,
                    dmcf_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Gradients of the point-cloud ops (ABI 2.13; dmcf_amd/csrc/metrics_bwd.hip): nn_distance (NnDistanceGrad,
 * nn_distance.cu:158-183), match_cost (MatchCostGrad, tf_approxmatch.cu:346-430), the fused EMD with the match held constant
 * (approx_match has no gradient) and gather_point (GatherPointGrad).  No float atomics: scattered terms are gathered through
 * a stable sort of the index list (each target sums its sources in ascending source order, or, past 256 of them, in one
 * workgroup's fixed order), all-pairs sums run in a fixed
 * order with a size-only split plan, so two identical calls give identical bits.  Every call validates its arguments and
 * workspace (DMCF_EINVAL / DMCF_EWORKSPACE) before anything is enqueued; an output pointer of NULL means "not wanted"
 * (both NULL: DMCF_EINVAL).  Gradients are written, not accumulated.  Workspace queries return 0 for sizes < 0 (and for
 * empty sets, where nothing is read).
 * ---------------------------------------------------------------------------------------------- */
/* nn_distance: idx1 [b, n] / idx2 [b, m] are the forward's indices; grad_dist1 [b, n] / grad_dist2 [b, m] may be NULL (zero;
 * then its idx may be NULL too).  With g = 2 grad_dist1[i]:  grad_xyz1[i] += g (x1_i - x2_{idx1[i]}),
 * grad_xyz2[idx1[i]] -= g (x1_i - x2_{idx1[i]}); the terms of dist2 are the same with the sets swapped.  Each point takes its
 * own term first, then subtracts the scattered ones.  b n and b m < 2^31. */
size_t dmcf_nn_distance_backward_workspace_bytes(int64_t b, int64_t n, int64_t m);
int dmcf_nn_distance_backward(const float* xyz1, const float* xyz2, int64_t b, int64_t n, int64_t m, const int32_t* idx1,
                              const int32_t* idx2, const float* grad_dist1, const float* grad_dist2, float* grad_xyz1,
                              float* grad_xyz2, void* workspace, size_t workspace_bytes, dmcf_stream_t stream);
/* match_cost with a dense match [b, m, n] and grad_cost [b] (device):
 *   grad_xyz1[k] = g_b sum_l match[l, k] (x1_k - x2_l) rsqrt(max(d2_kl, 1e-20)),
 *   grad_xyz2[l] = g_b sum_k match[l, k] (x2_l - x1_k) rsqrt(max(d2_kl, 1e-20)). */
size_t dmcf_match_cost_backward_workspace_bytes(int64_t b, int64_t n, int64_t m);
int dmcf_match_cost_backward(const float* xyz1, const float* xyz2, int64_t b, int64_t n, int64_t m, const float* match,
                             const float* grad_cost, float* grad_xyz1, float* grad_xyz2, void* workspace, size_t workspace_bytes,
                             dmcf_stream_t stream);
/* dmcf_emd that also records the state its gradient needs: levels [b, 10, n + m] holds, for level j (in the order of the
 * passes, -4^7 first, 0 last), ratioL after pass A in [0, n_i) and ratioR after pass B in [n, n + m_i); zeros elsewhere.  The
 * launches of dmcf_emd plus asynchronous copies, so cost has dmcf_emd's bits.  Workspace: dmcf_emd_workspace_bytes. */
int dmcf_emd_with_levels(const float* xyz1, const float* xyz2, int64_t b, int64_t n, int64_t m, const int32_t* count1,
                         const int32_t* count2, float* cost, float* levels, void* workspace, size_t workspace_bytes,
                         dmcf_stream_t stream);
/* Gradient of dmcf_emd with the match held constant, never forming it: w_kl = sum_j (e^(level_j d2_kl) ratioR_j[l]) ratioL_j[k]
 * is recomputed per pair with the float32 expression of the forward's pass C (so it has the bits of dmcf_approx_match's
 * match[l, k]), then the formulas of dmcf_match_cost_backward.  count1 / count2: the HOST counts given to
 * dmcf_emd_with_levels; rows past a count get exact zeros.  Batch items run one after another, each with the split plan of
 * its own counts (a padded item gives the bits of the same item alone). */
size_t dmcf_emd_backward_workspace_bytes(int64_t b, int64_t n, int64_t m);
int dmcf_emd_backward(const float* xyz1, const float* xyz2, int64_t b, int64_t n, int64_t m, const int32_t* count1,
                      const int32_t* count2, const float* levels, const float* grad_cost, float* grad_xyz1, float* grad_xyz2,
                      void* workspace, size_t workspace_bytes, dmcf_stream_t stream);
/* The gradient of dmcf_emd_ragged (ABI 2.25): the recording forward and the match-free backward over a RAGGED batch, laid out
 * as for dmcf_emd_ragged (xyz1 [n_total, 3], xyz2 [m_total, 3], both row-splits arrays HOST int64 [batch + 1], validated
 * here before anything is enqueued).
 * dmcf_emd_ragged_with_levels enqueues the launches of dmcf_emd_ragged, so cost has its bits, and records levels
 * [10, n_total + m_total]: levels[L * (n_total + m_total) + row] is ratioL of row `row` of xyz1 after finish step A of level L,
 * levels[L * (n_total + m_total) + n_total + row] ratioR of row `row` of xyz2 after finish step B (the finish steps write them;
 * levels is zeroed first, so the rows of an item with either set empty hold exact zeros).  Workspace:
 * dmcf_emd_ragged_workspace_bytes.  The refusals of dmcf_emd_ragged, and NULL levels: DMCF_EINVAL; every item empty on both
 * sides: DMCF_OK with nothing written.
 * dmcf_emd_ragged_backward: grad_xyz1 [n_total, 3] / grad_xyz2 [m_total, 3] from those levels and grad_cost [batch] (device).
 * Result contract: item b's rows have exactly the bits dmcf_emd_backward gives for item b alone (b = 1, no counts, its own
 * levels).  Every item keeps the column chunks of its own split plan, both kernels share dmcf_emd_backward's tile walk, and the
 * combine sums in split order before multiplying by grad_cost[b]; what changes is the launch count: one asynchronous table
 * copy and at most 4 launches whatever the batch -- the gradient and the combine of each wanted side (dmcf_emd_backward: 4 per
 * item).  The entry point writes the tables -- a record per (item, 256 rows, column chunk) and per (item, 256 rows) -- from the
 * validated splits; no kernel reads row splits, and no float atomics are used.  Rows of an item whose other set is empty get
 * exact zeros.  batch == 0 with n_total == m_total == 0: DMCF_OK.  No item with a pair: DMCF_OK after the wanted gradients of
 * non-zero length are zeroed, with no other pointer looked at.  batch < 0 or > 2^26, NULL or malformed row splits, n_total or
 * m_total >= 2^31 - 257, more than INT32_MAX tiles on a side, and, when there is work, NULL points, levels, grad_cost or
 * workspace: DMCF_EINVAL.  The workspace holds the tables and every item's partials [nsplit, 3, rows], which is why its query
 * takes the splits; the query returns 0 for arguments the call refuses. */
int dmcf_emd_ragged_with_levels(const float* xyz1, int64_t n_total, const int64_t* row_splits1, const float* xyz2, int64_t m_total,
                                const int64_t* row_splits2, int64_t batch, float* cost, float* levels, void* workspace,
                                size_t workspace_bytes, dmcf_stream_t stream);
size_t dmcf_emd_ragged_backward_workspace_bytes(int64_t n_total, const int64_t* row_splits1, int64_t m_total,
                                                const int64_t* row_splits2, int64_t batch);
int dmcf_emd_ragged_backward(const float* xyz1, int64_t n_total, const int64_t* row_splits1, const float* xyz2, int64_t m_total,
                             const int64_t* row_splits2, int64_t batch, const float* levels, const float* grad_cost,
                             float* grad_xyz1, float* grad_xyz2, void* workspace, size_t workspace_bytes, dmcf_stream_t stream);
/* The velocity histograms of compare_dist (utils/evaluation_helper.py:43-75) for a RAGGED batch (ABI 2.26): x and y
 * [n_total, 3] share the HOST int64 row splits [batch + 1] (validated here before anything is enqueued; every item has at
 * least one row).  Per item b with cnt rows the call writes
 *   percentiles[b][0][a], percentiles[b][1][a]   the 5th and 95th percentile of the 2 cnt values x[:, a] u y[:, a] as
 *                                                np.percentile gives them for float32 data: numpy's _lerp in float32 between
 *                                                the order statistics plan[b].rank[0], [1] (weight gamma[0]) and rank[2], [3]
 *                                                (weight gamma[1]);
 *   counts[off_b + f], counts[off_b + bins_b + f] the number of rows of x, and of y, in flat bin f of the (per + 1)^3 grid:
 *                                                idx_a = clamp(trunc((v_a - min_a) / bin_w_a), 0, per), bin_w_a =
 *                                                ((max_a - min_a) + 1e-6f) / per with correctly rounded float32 divisions,
 *                                                f = (idx_0 (per + 1) + idx_1)(per + 1) + idx_2; per == 0: every row in bin 0;
 * bins_b = (plan[b].per + 1)^3, off_b = 2 (bins_0 + ... + bins_{b-1}); bins_total is their sum and counts has 2 bins_total
 * entries.  The plan depends on the items' sizes alone, so the host writes it (ops.percentile_plan); it is validated here:
 * 0 <= per <= 1023, 0 <= rank < 2 cnt, 0 <= gamma <= 1, the bins summing to bins_total.  The order statistics come from a
 * radix select (8-bit digits, four passes, integer atomics), the counts from integer atomics: all sums are integer sums, two
 * calls give identical bits, and the results are those of the host function bit for bit.  -0.0 selects as +0.0.  Inputs must
 * be finite: NaN is NOT looked for and is out of scope (the host function returns NaN percentiles for it); a quotient beyond
 * int32 saturates into the clamp where the host's cast is platform-defined.
 * One memset (the selection state in the workspace), one table copy from pageable host memory and 9 launches whatever the
 * batch; counts is zeroed by the call.  batch < 1 or > 2^26, n_total >= 2^31 - 257, an item without rows, NULL or malformed
 * splits, a bad plan, any NULL pointer: DMCF_EINVAL; a short workspace: DMCF_EWORKSPACE; all before anything is enqueued.
 * The workspace query returns 0 for sizes the call refuses. */
#define DMCF_HIST_TILE_ROWS 1024 /* rows of x and of y a workgroup takes in the digit and count launches */
typedef struct dmcf_hist_plan {
    int32_t per;     /* bins per axis minus one: int((cnt // bin_size) ** (1 / 3)) */
    int32_t rank[4]; /* k5, its upper neighbour, k95, its upper neighbour: 0-based ranks among the 2 cnt values */
    float gamma[2];  /* the interpolation weights of the two percentiles */
    int32_t reserved;
} dmcf_hist_plan;
size_t dmcf_hist_pair_ragged_workspace_bytes(int64_t n_total, int64_t batch, int64_t bins_total);
int dmcf_hist_pair_ragged(const float* x, const float* y, int64_t n_total, const int64_t* row_splits, int64_t batch,
                          const dmcf_hist_plan* plan, int64_t bins_total, float* percentiles, int32_t* counts, void* workspace,
                          size_t workspace_bytes, dmcf_stream_t stream);
/* gather_point: grad_inp [n_inp, channels] = sum over s with index[s] == t of grad_out[s, :] (repeated indices sum; indices
 * outside [0, n_inp) contribute nothing). */
size_t dmcf_gather_point_backward_workspace_bytes(int64_t n_index, int64_t n_inp);
int dmcf_gather_point_backward(const float* grad_out, const int32_t* index, int64_t n_index, int channels, int64_t n_inp,
                               float* grad_inp, void* workspace, size_t workspace_bytes, dmcf_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * PointNet's layer (models/pointnet.py:137-145): tf.keras.layers.Dense, tf.gather by neighbors_index and the ragged
 * tf.reduce_sum over the row splits, with the relu before the Dense and the residual after it.  Per output row r:
 *     out_r = (sum_{p in row r, 0 <= idx[p] < n_in} act(x_{idx[p]})) W + c_r b (+ residual_r)       (+ mask, below)
 * c_r the number of those pairs; act = relu (DMCF_ND_RELU) or the identity; the bias is summed once per neighbour, as the
 * reference's Dense-then-gather does.  A neighbour index outside [0, n_in) contributes nothing, neither features nor bias:
 * what TensorFlow's GPU gather returns for out-of-range rows (zeros) and what its gradient does with them (drops them).
 * One launch: gather, relu, contraction on the matrix cores (v_mfma_f32_16x16x4_f32), bias and residual.  Row sums are
 * formed in pair order and no float atomics are used: two identical calls give identical bits.
 * Rows reaching outside [0, n_pairs) are empty.  Cin, Cout <= 128 (DMCF_EUNSUPPORTED beyond).  Sizes, pointers and, when
 * host_row_splits is given, the row splits are validated on the host before anything is enqueued (DMCF_EINVAL).
 * ---------------------------------------------------------------------------------------------- */
#define DMCF_ND_RELU 1          /* act = relu (forward); the backward masks the input gradient with x > 0 */
#define DMCF_ND_W_TRANSPOSED 2  /* kernel is stored [Cout, Cin] (the backward's input gradient uses W^T) */
typedef struct dmcf_neighbor_dense_args {
    uint32_t struct_size;                 /* sizeof(dmcf_neighbor_dense_args) of the caller; smaller: DMCF_EINVAL */
    int32_t flags;                        /* DMCF_ND_* */
    const float* x;                       /* [n_in, cin]; may be NULL when n_in == 0 */
    int64_t n_in;
    int32_t cin;
    int32_t cout;
    const float* kernel;                  /* [cin, cout] ([cout, cin] with DMCF_ND_W_TRANSPOSED) */
    const float* bias;                    /* [cout] or NULL */
    const float* residual;                /* [n_out, cout] or NULL */
    const float* mask;                    /* [n_out, cout] or NULL: out = 0 where mask <= 0 (the backward's relu) */
    const int32_t* neighbors_index;       /* [n_pairs] */
    const int64_t* neighbors_row_splits;  /* [n_out + 1] CSR, or [n_out] row begins with neighbors_row_count */
    const int32_t* neighbors_row_count;   /* optional [n_out]: padded lists (dmcf_frs_search_padded); NULL = CSR */
    int64_t n_out;
    int64_t n_pairs;                      /* entries neighbors_index holds */
    const int64_t* host_row_splits;       /* optional HOST copy of neighbors_row_splits: checked (CSR: starts at 0, monotone,
                                             ends at n_pairs; padded: begins inside [0, n_pairs]) */
    float* out;                           /* [n_out, cout]; may not alias x or mask */
    float* record_s;                      /* optional [n_out, cin]: the aggregate S (the backward's operand) */
    float* record_count;                  /* [n_out] c_r, given together with record_s */
} dmcf_neighbor_dense_args;

int dmcf_neighbor_dense_forward(const dmcf_neighbor_dense_args* args, dmcf_stream_t stream);

/* Backward of dmcf_neighbor_dense_forward for G = grad_out = dL/d out [n_out, cout]:
 *     grad_x_j    = act'(x_j) (sum_{r : j in row r} G_r) W^T   (nd_gather_mfma on the inverted list, W^T, mask x > 0)
 *     grad_kernel = S^T G,   grad_bias = sum_r c_r G_r         (per-slab partials on the matrix cores, summed in slab order)
 * with S and c as dmcf_neighbor_dense_forward recorded them.  inv_*: dmcf_invert_neighbors_list(n_in, ...) of the forward
 * list (out-of-range indices are dropped there).  Each output is optional (NULL = not wanted).  The residual's gradient is
 * G itself (the caller's).  No float atomics: two identical calls give identical bits. */
typedef struct dmcf_neighbor_dense_backward_args {
    uint32_t struct_size;                 /* sizeof(dmcf_neighbor_dense_backward_args) of the caller; smaller: DMCF_EINVAL */
    int32_t flags;                        /* DMCF_ND_RELU: the forward applied relu */
    const float* x;                       /* [n_in, cin] the forward's input (read for the relu mask only) */
    int64_t n_in;
    int32_t cin;
    int32_t cout;
    const float* kernel;                  /* [cin, cout] */
    const float* grad_out;                /* [n_out, cout] */
    int64_t n_out;
    const float* s;                       /* [n_out, cin] record_s of the forward */
    const float* count;                   /* [n_out] record_count of the forward */
    const int32_t* inv_index;             /* [inv_n_pairs] */
    const int64_t* inv_row_splits;        /* [n_in + 1] */
    int64_t inv_n_pairs;
    float* grad_x;                        /* [n_in, cin] or NULL */
    float* grad_kernel;                   /* [cin, cout] or NULL */
    float* grad_bias;                     /* [cout] or NULL */
} dmcf_neighbor_dense_backward_args;

size_t dmcf_neighbor_dense_backward_workspace_bytes(const dmcf_neighbor_dense_backward_args* args);
int dmcf_neighbor_dense_backward(const dmcf_neighbor_dense_backward_args* args, void* workspace, size_t workspace_bytes,
                                 dmcf_stream_t stream);
/* Diagnostics: the device kernels the forward (fwd) and / or the backward (bwd) launch for these arguments, in launch
 * order, separated by ';' (names as rocprofv3 prints them, e.g. "nd_gather_mfma<2>"); either argument may be NULL */
int dmcf_neighbor_dense_kernel_names(const dmcf_neighbor_dense_args* fwd, const dmcf_neighbor_dense_backward_args* bwd,
                                     char* names, size_t name_bytes);

/* ------------------------------------------------------------------------------------------------
 * The training loop's optimizer step (ABI 2.11): tf.keras.optimizers.Adam(epsilon=...) of models/pbf_model.py:511-517 over
 * every trainable tensor of a model in one launch, in the order of operations of TensorFlow's ApplyAdam GPU functor:
 *     alpha = lr sqrt(1 - beta_2_power) / (1 - beta_1_power)
 *     m += (1 - beta_1)(g - m);   v += (1 - beta_2)(g g - v);   param -= alpha m / (epsilon + sqrt(v))
 * Keras' coefficients for optimizer iteration t (counted from 0): lr = the schedule at t, beta_*_power = pow(beta_*, t + 1)
 * in float32 -- computed by the caller.  clip_norm > 0: every gradient is first clipped per tensor as tf.clip_by_norm does,
 * g c / max(|g|_2, c) (|g|_2 = 0 when the l2 sum is 0), with the l2 sums reduced in a fixed order (per-block partials in
 * the workspace, one combine): two launches; one without clipping.  No float atomics: two identical calls give identical
 * bits.  Gradients are read only; param, m and v are updated in place and may not alias each other or a gradient.
 * ---------------------------------------------------------------------------------------------- */
typedef struct dmcf_adam_tensor {
    float* param;                          /* [n] */
    const float* grad;                     /* [n] */
    float* m;                              /* [n] first-moment slot */
    float* v;                              /* [n] second-moment slot */
    int64_t n;                             /* elements; 0: skipped (the pointers may then be NULL) */
} dmcf_adam_tensor;

typedef struct dmcf_adam_args {
    uint32_t struct_size;                  /* sizeof(dmcf_adam_args) of the caller; smaller: DMCF_EINVAL */
    int32_t n_tensors;                     /* 0 .. 65535 */
    const dmcf_adam_tensor* tensors;       /* HOST array [n_tensors]: validated, and sizes the launch */
    const dmcf_adam_tensor* device_tensors; /* the same n_tensors records in DEVICE memory: what the kernels read */
    float lr;
    float beta_1;
    float beta_2;
    float epsilon;
    float beta_1_power;
    float beta_2_power;
    float clip_norm;                       /* <= 0: no clipping */
    int32_t reserved;                      /* 0 */
} dmcf_adam_args;

size_t dmcf_adam_step_workspace_bytes(const dmcf_adam_args* args);
int dmcf_adam_step(const dmcf_adam_args* args, void* workspace, size_t workspace_bytes, dmcf_stream_t stream);
/* Diagnostics: the kernels dmcf_adam_step launches for these arguments, in launch order, separated by ';'
 * ("adam_sumsq;adam_update" with clipping, "adam_update" without, "" when no tensor holds an element) */
int dmcf_adam_step_kernel_names(const dmcf_adam_args* args, char* names, size_t name_bytes);

/* ------------------------------------------------------------------------------------------------
 * Disc rasterizer of the renderer (ABI 2.12; dmcf_amd/utils/draw_sim2d.py, the reference's utils/draw_sim2d.py:11-45, where
 * skia's canvas.drawCircle draws one anti-aliased circle per particle).  Filled discs of ONE colour and radius r (pixels)
 * composited over F frames of a float32 RGB image [F, H, W, 3] (values in [0, 1]).  Pixel model:
 *   - pixel (i, j) (column i, row j) has its centre at (i + 0.5, j + 0.5) in the coordinates of the disc centres;
 *   - a disc with centre p covers the pixel by  cov = clamp(r + 0.5 - |p - centre|, 0, 1) * min(1, 2 r);
 *   - per pixel and call  T = prod over the discs of (1 - a cov),  a = alpha / 255 of color_argb (0xAARRGGBB), and
 *     C <- C T + colour (1 - T)  with colour = (R, G, B) / 255; a pixel no disc covers keeps its bits.
 * Discs with a centre that is not finite contribute nothing; discs partly or wholly off the canvas are legal.  A radius that
 * is not finite or <= 0, or alpha 0, draws nothing (no launch).  Since every disc of a call has the same colour, the result
 * does not depend on the order of the discs beyond rounding; T is formed as exp of the sum of log(1 - a cov) in 2^-32 fixed
 * point (int64, exactly associative), so two identical calls, and any binning or launch geometry, give identical bits.  No
 * float atomics.
 * xy: float32 [F, n, 2] pixel coordinates, frame f's points at xy + 2 f frame_stride; frame_stride = 0: the same n points in
 * every frame (binned once); otherwise frame_stride >= n.  8-byte aligned.  Limits (DMCF_EINVAL beyond): 1 <= W, H <= 32768,
 * F <= 65535, n < 2^31.  Two phases, because the size of the tile bins depends on the data:
 *   dmcf_raster_count  bins the discs into 16 x 16-pixel tiles (per source frame) and writes the number of (disc, tile)
 *                      entries to *total (one device int64);
 *   the caller reads *total and allocates bins of 2 * total floats (bin_capacity = total);
 *   dmcf_raster_discs  fills the bins and draws, with the same xy / n / F / frame_stride / radius / W / H and the workspace
 *                      the count left behind.  Entries past bin_capacity are dropped (never written out of bounds).
 * Workspace: dmcf_raster_workspace_bytes(n, F, frame_stride, W, H).
 * ---------------------------------------------------------------------------------------------- */
size_t dmcf_raster_workspace_bytes(int64_t n_points, int64_t n_frames, int64_t frame_stride, int32_t width, int32_t height);
int dmcf_raster_count(const float* xy, int64_t n_points, int64_t n_frames, int64_t frame_stride, float radius, int32_t width,
                      int32_t height, void* workspace, size_t workspace_bytes, int64_t* total, dmcf_stream_t stream);
int dmcf_raster_discs(const float* xy, int64_t n_points, int64_t n_frames, int64_t frame_stride, float radius, uint32_t color_argb,
                      int32_t width, int32_t height, float* image, void* workspace, size_t workspace_bytes, float* bins,
                      int64_t bin_capacity, dmcf_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Depth-tested sphere splat of the 3-D renderer (ABI 2.27; dmcf_amd/csrc/splat.hip, dmcf_amd/utils/draw_sim3d.py; no reference
 * counterpart).  Every point is a sphere of world radius r seen through a camera; a DEPTH pass per point group records, per
 * pixel, which sphere is visible, in a uint64 key; one SHADE pass over up to DMCF_SPLAT_MAX_LAYERS groups writes the image.
 *
 * Camera (struct dmcf_camera, sizeof = 80): view is a row-major 3 x 4 matrix, world -> camera; the camera looks along +z, x is
 * right, y is DOWN (as image rows are).  focal: pixels per world unit at z = 1 (perspective), or pixels per world unit
 * (orthographic != 0).  (cx, cy): the principal point in pixels.  near >= 0.  All values finite, focal > 0 (else DMCF_EINVAL).
 *
 * Pixel model.  Every operation below is ONE float32 round-to-nearest operation, un-fused, in the order written (a * b + c is a
 * product, rounded, then a sum, rounded; quotients and square roots are the correctly rounded IEEE ones), so that a float32
 * restatement reproduces every bit (tests/splat_ref.py):
 *   centre c = (x, y, z), row i of view = (v_i0, v_i1, v_i2, v_i3):
 *     xc = ((v00 x + v01 y) + v02 z) + v03        yc, zc alike from rows 1 and 2
 *     m  = focal / zc  (perspective)   or   m = focal  (orthographic)
 *     sx = cx + m xc        sy = cy + m yc
 *     R  = max(m r, min_px)        R2 = R R
 *   pixel (px, py) (column, row), its centre at (px + 0.5, py + 0.5) (exact in float32):
 *     dx = (px + 0.5) - sx      dy = (py + 0.5) - sy      d2 = dx dx + dy dy
 *     the sphere covers the pixel iff d2 < R2
 *     z  = zc - sqrt(R2 - d2) / m          (the impostor: the sphere is orthographic within itself)
 *   the sample is dropped when z is not finite or z <= near; the sphere is skipped when x, y or z is not finite or
 *   zc <= near; footprints are clipped to the image.  min_px (finite, >= 0) keeps sub-pixel spheres visible: with
 *   R >= 0.75 > sqrt(1/2) every on-screen sphere covers at least one pixel centre.
 *
 * dmcf_splat_depth: for every sample  atomicMin(keys[f, py, px], key)  with
 *     key = (uint64(bits(z)) << 32) | index            the NEAREST sphere, or with DMCF_SPLAT_FARTHEST
 *     key = (uint64(~bits(z)) << 32) | index           the FARTHEST one;
 *   z > near >= 0, so bits(z) orders as z does; index is the point's index within its frame.  An all-ones key means "empty":
 *   the CALLER initialises keys (the call never clears them, so several groups can be splatted into one buffer).  A minimum
 *   over integers is associative and commutative: the key map is the same bits whatever the launch geometry or the arrival
 *   order, and equal depths go to the lowest index.  No float atomics, no sort, no workspace, one launch.
 *   xyz: float32 [F, n, 3], frame f's points at xyz + 3 f frame_stride; frame_stride = 0: the same n points into every frame;
 *   otherwise frame_stride >= n.  keys: uint64 [F, H, W], 8-byte aligned.  Limits (DMCF_EINVAL beyond): 1 <= W, H <= 32768,
 *   F <= 65535, n < 2^31.  n = 0, F = 0, or a radius that is not finite or <= 0: nothing is launched, keys stay as they are.
 *
 * dmcf_splat_shade: per pixel, every layer's non-empty key is decoded to its depth (the high word, complemented first for a
 *   FARTHEST layer) and the layer with the smallest depth wins; equal depths go to the lowest layer number.  For the winning
 *   sphere (xyz, radius of ITS layer) sx, sy, R, R2, dx, dy, d2 are recomputed as above, then
 *     nz = sqrt(max(R2 - d2, 0)) / R        shade = ambient + (1 - ambient) nz          (a headlight Lambert term)
 *     C  = C (1 - a) + (colour shade) a     per channel, a = alpha / 255, colour = (R, G, B) / 255 of color_argb (0xAARRGGBB)
 *   image: float32 [F, H, W, 3], composited in place; a pixel without a sample keeps its bits.  depth: float32 [F, H, W] or
 *   NULL; it receives the winning depth, +inf where there is no sample.  0 <= ambient <= 1.  One lane per pixel, one launch.
 *   A layer whose n_points is 0 or whose radius is not finite or <= 0 is ignored; more than DMCF_SPLAT_MAX_LAYERS layers is
 *   DMCF_EINVAL.  The camera, min_px and each layer's xyz / n_points / frame_stride / radius must be those of the depth calls.
 * ---------------------------------------------------------------------------------------------- */
#define DMCF_SPLAT_FARTHEST 1
#define DMCF_SPLAT_MAX_LAYERS 4
typedef struct dmcf_camera {
    float view[12];       /* row-major 3 x 4, world -> camera (+z forward, x right, y down) */
    float focal;          /* pixels per world unit at z = 1, or per world unit when orthographic */
    float cx, cy;         /* principal point, pixels */
    float near;           /* >= 0 */
    int32_t orthographic; /* 0: perspective */
    int32_t reserved[3];  /* 0; sizeof(dmcf_camera) = 80 */
} dmcf_camera;
typedef struct dmcf_splat_layer {
    const uint64_t* keys; /* [F, H, W], as dmcf_splat_depth left them */
    const float* xyz;     /* the points of that depth call */
    int64_t n_points;
    int64_t frame_stride;
    float radius;
    uint32_t color_argb;
    int32_t flags;        /* DMCF_SPLAT_FARTHEST as in the depth call */
    int32_t reserved;     /* 0; sizeof(dmcf_splat_layer) = 48 */
} dmcf_splat_layer;

int dmcf_splat_depth(const float* xyz, int64_t n_points, int64_t n_frames, int64_t frame_stride, float radius, float min_px,
                     const dmcf_camera* camera, int32_t width, int32_t height, int32_t flags, uint64_t* keys, dmcf_stream_t stream);
int dmcf_splat_shade(const dmcf_splat_layer* layers, int32_t n_layers, const dmcf_camera* camera, float min_px, float ambient,
                     int32_t width, int32_t height, int64_t n_frames, float* image, float* depth, dmcf_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * The 1-D SPH solver that generates the column datasets (ABI 2.17; dmcf_amd/csrc/sph1d.hip): SPH1D.step of
 * datasets/column_gen.py:159-186 for a batch of independent scenes, n_frames steps per call.  One 64-lane wavefront per
 * scene, lane = point, so a scene holds at most 64 points: max_points > 64 is DMCF_EINVAL.
 *
 * A point is (x, v, m), float32; the first bcnt points of a scene are the boundary and never move.  With d = x_i - x_j
 * (float32), the splines W(|d|) and W'(d) of column_gen.py:51-54 and :68-73 evaluated in float32 on the RAW distance (not
 * d / h; the factor 4 / (3 h) and the softening 0.01 h^2 rounded to float32), and sums over j in float64, one step is
 *   dens_i = sum_j m_j W(|d|)
 *   f_visc = visc * 2 sum_j m_j / dens_j (v_i - v_j) d W'(d) / (d^2 + 0.01 h^2)
 *   v += dt (gravity + f_visc);  x += dt v  (this one in float32)                                   fluid points only
 *   up to max_iter times:
 *     dens_i as above;  p_i = max(stiffness ((dens_i / rest_dens)^7 - 1), 0), boundary points: p of the first fluid point
 *     err = max over the fluid points of max(dens_i - rest_dens, 0)
 *     f_i = -(m_i / dens_i) dens_i sum_j m_j (p_i / dens_i^2 + p_j / dens_j^2) W'(d)
 *     v += dt f / m;  x += dt^2 f / m   (formed in float64, rounded to float32 once)                  fluid points only
 *     stop when err < eps -- AFTER the update, so every step runs at least one iteration.
 * The j sums run in index order; numpy's pairwise order is not reproduced, so results agree with the reference to rounding,
 * not bit for bit.  Two calls on equal inputs give equal bits, whatever else is in the batch; and since the whole solver
 * state is the (x, v, m) array, a rollout cut into several calls (state_out of one as the state of the next) gives the bits
 * of one call.
 *
 * state      float32 [n_scenes, max_points, 3]: scene s holds n_tot[s] points, the rest of its slot is ignored
 * n_tot      int32 [n_scenes] (device); values outside [0, max_points] are clamped
 * sequence   float32 [n_frames, n_scenes, max_points, 2]: (x, v) BEFORE each step (gen_data :309-312); zeros past n_tot[s]
 * state_out  float32 [n_scenes, max_points, 3]: the state after the last step; may be `state` itself
 * iterations int32 [n_frames, n_scenes]: pressure iterations of each step, in [1, max_iter]
 * sequence and iterations may be NULL when n_frames == 0.  No workspace.  A step costs up to max_iter iterations of
 * O(n_tot^2) work on one wavefront: callers bound n_frames * max_iter per call (dmcf_amd/ops.py:sph1d_rollout does).
 * ---------------------------------------------------------------------------------------------- */
typedef struct dmcf_sph1d_params {
    uint32_t struct_size; /* sizeof(dmcf_sph1d_params) of the caller; smaller: DMCF_EINVAL */
    int32_t bcnt;         /* boundary points per scene, 0 <= bcnt < max_points */
    int32_t max_iter;     /* >= 1 */
    int32_t reserved;
    double h;             /* > 0 */
    double rest_dens;     /* > 0 */
    double stiffness;
    double visc;
    double gravity;
    double dt;
    double eps;
} dmcf_sph1d_params;

int dmcf_sph1d_rollout(const float* state, const int32_t* n_tot, int64_t n_scenes, int32_t max_points,
                       const dmcf_sph1d_params* params, int32_t n_frames, float* sequence, float* state_out,
                       int32_t* iterations, dmcf_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Voxel convolution (ABI 2.18).  Replaces what SparseConv and SparseConvTranspose (utils/convolutions.py:476-885) ask of
 * ml3d.ops.continuous_conv / continuous_conv_transpose: identity mapping, align_corners = False, nearest-neighbour
 * interpolation, an offset.  Each pair then touches ONE filter cell with weight 1, and both layers and both feature gradients
 * are one row-gather operator over a CSR list (rows r, columns idx[p]):
 *
 *     out[r,:] = row_scale[r] * sum_{p in row r} col_scale[idx[p]] * W[cell(sign * (col_pos[idx[p]] - row_pos[r]))]^T x[idx[p],:]  (+ bias)
 *
 * cell(d), per axis a with k_a cells: t = d_a * (1 / extent) * k_a + k_a / 2 (integer division), minus 0.5 for even k_a -- the
 * operations of dmcf_cconv_forward's identity mapping without ALIGN_CORNERS -- then + offset[a]; the cell is
 * clamp((int)roundf(t), 0, k_a - 1).  offset is (x, y, z); filter_dims is (z, y, x, Cin, Cout) as everywhere.
 *   SparseConv           rows = output points, columns = input points, sign +1, row_scale = 1 / |row| (normalize),
 *                        col_scale = inp_importance
 *   SparseConvTranspose  rows = output points over the INVERTED list, columns = input points, DMCF_SPARSE_NEGATE,
 *                        row_scale = out_importance, col_scale = 1 / |N_T(j)| (normalize)
 *   feature gradients    the same call on the inverted list with rows and columns swapped, the other sign,
 *                        DMCF_SPARSE_W_TRANSPOSED toggled and the two scales swapped (dmcf_sparse_conv_backward does that)
 * Any filter shape and channel count; channels that do not fill a block of the matrix cores are padded inside the kernel.
 * Deterministic: no atomics anywhere, two identical calls give identical bits.
 * ---------------------------------------------------------------------------------------------- */
#define DMCF_SPARSE_NEGATE 1        /* sign = -1: the cell of row_pos - col_pos */
#define DMCF_SPARSE_W_TRANSPOSED 2  /* x has filter_dims[4] channels, out has filter_dims[3]: W[cell] instead of W[cell]^T */
#define DMCF_SPARSE_ACCUMULATE 4    /* out += result */
typedef struct dmcf_sparse_conv_args {
    uint32_t struct_size;                 /* sizeof(dmcf_sparse_conv_args) of the caller; smaller: DMCF_EINVAL */
    int32_t flags;                        /* DMCF_SPARSE_* */
    const float* filters;                 /* [kz][ky][kx][Cin][Cout] */
    int32_t filter_dims[5];
    int32_t reserved;                     /* 0 */
    const float* row_positions;           /* [n_rows, 3] */
    int64_t n_rows;
    const float* col_positions;           /* [n_cols, 3] */
    int64_t n_cols;
    const float* col_features;            /* x: [n_cols, Cin] ([n_cols, Cout] with DMCF_SPARSE_W_TRANSPOSED) */
    const float* row_scale;               /* [n_rows] or NULL = 1 */
    const float* col_scale;               /* [n_cols] or NULL = 1 */
    const int32_t* neighbors_index;       /* [n_pairs] column of each pair; entries outside [0, n_cols) are skipped */
    const int64_t* neighbors_row_splits;  /* [n_rows + 1]; rows reaching past n_pairs are treated as empty */
    int64_t n_pairs;
    float extent;                         /* voxel_size * kernel_size[-1] */
    float offset[3];                      /* (x, y, z), in cells */
    const float* bias;                    /* [channels of out] or NULL */
    float* out;                           /* [n_rows, Cout] ([n_rows, Cin] with DMCF_SPARSE_W_TRANSPOSED) */
} dmcf_sparse_conv_args;

int dmcf_sparse_conv_forward(const dmcf_sparse_conv_args* args, dmcf_stream_t stream);

/* Gradients of dmcf_sparse_conv_forward(fwd) for grad_out = dL/d out (bias and DMCF_SPARSE_ACCUMULATE of fwd are ignored):
 *   grad_filters [shape of filters], or NULL: dW[c] = sum_{p : cell(p) = c} row_scale * col_scale * x_j (x) G_r -- per-slab
 *       partial sums over contiguous pair ranges, added in slab order;
 *   grad_col_features [shape of col_features], or NULL: the forward kernel over the inverted list
 *       (dmcf_invert_neighbors_list(n_cols, ...): inv_index [inv_n_pairs] = the row of each entry, inv_row_splits [n_cols + 1]).
 * The scales and the bias get no gradient here (they are elementwise: the caller's framework forms them). */
size_t dmcf_sparse_conv_backward_workspace_bytes(const dmcf_sparse_conv_args* fwd, int want_grad_filters);
int dmcf_sparse_conv_backward(const dmcf_sparse_conv_args* fwd, const float* grad_out, const int32_t* inv_index,
                              const int64_t* inv_row_splits, int64_t inv_n_pairs, float* grad_filters, float* grad_col_features,
                              void* workspace, size_t workspace_bytes, dmcf_stream_t stream);
/* Diagnostics: the device kernels the forward (backward = 0) or the backward (backward = 1: filter gradient, 2: feature
 * gradient, 3: both) launches, in launch order, separated by ';' */
int dmcf_sparse_conv_kernel_names(const dmcf_sparse_conv_args* args, int backward, char* names, size_t name_bytes);

#ifdef __cplusplus
}
#endif
#endif /* DMCF_HIP_H_ */
