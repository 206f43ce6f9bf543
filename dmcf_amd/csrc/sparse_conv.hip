// Voxel convolution for gfx950: SparseConv and SparseConvTranspose (utils/convolutions.py:476-885) and their gradients.
//
// The two layers call ml3d.ops.continuous_conv / continuous_conv_transpose with the identity mapping, align_corners = False and
// nearest-neighbour interpolation over a max-norm neighbour list: every pair touches ONE filter cell with weight 1.  Both
// layers and both feature gradients are then one row-gather operator (include/dmcf_hip.h):
//
//     out[r] = rs[r] * sum_{p in row r} cs[idx[p]] * W[cell(sign * (colpos[idx[p]] - rowpos[r]))]^T x[idx[p]]
//
//   sparse_conv_kernel    a wave owns a tile of 16 rows (M of v_mfma_f32_16x16x4_f32).  Four lanes per row walk the row's pairs
//                         and ADD each pair's feature row into the one [cell][channel] slot of the row's image in LDS -- one
//                         LDS update per channel where the trilinear splat of the CConv kernels does eight -- then the wave
//                         contracts [16, K * Cin] x [K * Cin, Cout] on the matrix cores, the filter read straight from
//                         memory (L2 resident) with out-of-range channels as zeros.  The image is built in chunks of cells
//                         (and of channels above 240) that fit 15.25 KB per wave; the accumulators live across the chunks.
//                         A k-step whose 64 image values are all zero (a cell none of the 16 rows has a pair in) is skipped.
//   sparse_pair_geometry  (backward) row, cell and scale of every pair, once
//   sparse_filter_grad    dW[c] = sum_{p : cell(p) = c} rs * cs * x_j (x) G_r over a SLAB of consecutive pairs, in pair order,
//                         each thread owning its elements of dW: per-slab partial sums, no atomics
//   sparse_filter_reduce  the partial sums added in slab order
// Every sum has a fixed order: two identical calls give identical bits.
#include <string.h>

#include "cconv_common.h"

namespace dmcf {

struct SparseParams {
    const float* W;
    int kx, ky, kz, K;
    int cw_in, cw_out;  // the filter's channel dims as stored
    int cin, cout;      // channels of x and of out (swapped with DMCF_SPARSE_W_TRANSPOSED)
    int transposed;
    const float* row_pos;
    const float* col_pos;
    const float* x;
    const float* rsc;
    const float* csc;
    const int32_t* idx;
    const int64_t* rs;
    int64_t n_rows, n_cols, n_pairs;
    float inv_extent, sign;
    float off[3];
    const float* bias;
    float* out;
    int accumulate;
    int CW, ncc, cpc;  // channels per chunk (multiple of 4), channel chunks, cells per chunk
};

// filter cell along one axis: the operations of filter_coords' identity, non-align-corners branch, the offset added last
__device__ __forceinline__ int sparse_axis_cell(float d, float inv_extent, int k, float off) {
    float t = d * inv_extent;
    t = t * (float)k + (float)(k / 2);
    if (k % 2 == 0) t -= 0.5f;
    t += off;
    const int c = (int)roundf(t);
    return min(max(c, 0), k - 1);
}

__device__ __forceinline__ int sparse_cell(const SparseParams& p, const float* __restrict__ cpos, float rx, float ry, float rz) {
    const float dx = p.sign * (cpos[0] - rx), dy = p.sign * (cpos[1] - ry), dz = p.sign * (cpos[2] - rz);
    const int cx = sparse_axis_cell(dx, p.inv_extent, p.kx, p.off[0]);
    const int cy = sparse_axis_cell(dy, p.inv_extent, p.ky, p.off[1]);
    const int cz = sparse_axis_cell(dz, p.inv_extent, p.kz, p.off[2]);
    return (cz * p.ky + cy) * p.kx + cx;
}

constexpr int kSpRows = 16;                // rows of a wave's tile
constexpr int kSpChunk = 240;              // floats of a row's image per chunk
constexpr int kSpStride = kSpChunk + 4;    // 244 = 52 (mod 64): the 16 rows x 4 lanes of an update hit 64 different banks
constexpr int kSpNT = 4;                   // 16-column output tiles per pass over the list

__global__ __launch_bounds__(256) void sparse_conv_kernel(const SparseParams p) {
    __shared__ float img_all[4][kSpRows * kSpStride];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* img = img_all[wave];
    const int64_t tile0 = ((int64_t)blockIdx.x * 4 + wave) * kSpRows;
    if (tile0 >= p.n_rows) return;  // whole wave leaves (no workgroup barrier below)
    // splat role: 4 lanes per row
    const int srow = lane >> 2, sub = lane & 3;
    const int64_t r = tile0 + srow;
    int64_t beg = 0, end = 0;
    float rx = 0.0f, ry = 0.0f, rz = 0.0f;
    if (r < p.n_rows) {
        beg = p.rs[r];
        end = p.rs[r + 1];
        if (beg < 0 || end > p.n_pairs || end < beg) end = beg;  // a row reaching past the list: empty
        rx = p.row_pos[3 * r];
        ry = p.row_pos[3 * r + 1];
        rz = p.row_pos[3 * r + 2];
    }
    // contraction role: lane (m, kq) holds A[m][kq] and B[kq][m]
    const int m16 = lane & 15, kq = lane >> 4;
    const int NT = (p.cout + 15) >> 4;
    const int64_t wcell = (int64_t)p.cw_in * p.cw_out;
    for (int n0 = 0; n0 < NT; n0 += kSpNT) {
        f32x4 acc[kSpNT];
#pragma unroll
        for (int n = 0; n < kSpNT; ++n) acc[n] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        for (int c0 = 0; c0 < p.K; c0 += p.cpc) {
            const int nc = min(p.cpc, p.K - c0);
            for (int cc = 0; cc < p.ncc; ++cc) {
                const int ch0 = cc * p.CW;
                const int cw = min(p.CW, ((p.cin + 3) & ~3) - ch0);  // multiple of 4
                const int used = nc * p.CW;
                // (the previous chunk's reads are done before the image is cleared: lanes talk through LDS)
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                for (int f = sub; f < used; f += 4) img[srow * kSpStride + f] = 0.0f;
                for (int64_t q = beg; q < end; ++q) {
                    const int32_t j = p.idx[q];
                    if (j < 0 || j >= p.n_cols) continue;
                    const int cell = sparse_cell(p, p.col_pos + 3 * (int64_t)j, rx, ry, rz) - c0;
                    if (cell < 0 || cell >= nc) continue;
                    const float s = p.csc ? p.csc[j] : 1.0f;
                    const float* __restrict__ xj = p.x + (int64_t)j * p.cin;
                    float* dst = img + srow * kSpStride + cell * p.CW;
                    for (int ch = sub; ch < cw; ch += 4) {
                        const int g = ch0 + ch;
                        if (g < p.cin) dst[ch] += s * xj[g];
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                for (int c = 0; c < nc; ++c) {
                    const float* arow = img + m16 * kSpStride + c * p.CW + kq;
                    for (int qd = 0; qd < (cw >> 2); ++qd) {
                        const float a = arow[4 * qd];
                        if (__ballot(a != 0.0f) == 0ull) continue;  // no row of the tile has a pair in this cell
                        const int ch = ch0 + 4 * qd + kq;
#pragma unroll
                        for (int n = 0; n < kSpNT; ++n) {
                            if (n0 + n >= NT) break;
                            const int co = 16 * (n0 + n) + m16;
                            float w = 0.0f;
                            if (ch < p.cin && co < p.cout) {
                                const int64_t e = p.transposed ? ((int64_t)co * p.cw_out + ch) : ((int64_t)ch * p.cw_out + co);
                                w = p.W[(int64_t)(c0 + c) * wcell + e];
                            }
                            acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, w, acc[n], 0, 0, 0);
                        }
                    }
                }
            }
        }
        // D layout: lane (rows 4 (lane >> 4) + i, column lane & 15)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t row = tile0 + 4 * kq + i;
            if (row >= p.n_rows) continue;
            const float rsv = p.rsc ? p.rsc[row] : 1.0f;
#pragma unroll
            for (int n = 0; n < kSpNT; ++n) {
                const int co = 16 * (n0 + n) + m16;
                if (n0 + n >= NT || co >= p.cout) continue;
                float v = acc[n][i] * rsv;
                if (p.bias) v += p.bias[co];
                float* dst = p.out + row * p.cout + co;
                if (p.accumulate) v += *dst;
                *dst = v;
            }
        }
    }
}

// ---- backward: the filter gradient ------------------------------------------------------------------------------------------------

// one thread per row: row, cell and scale of each of its pairs (pair_row stays -1, from the memset, for everything that is no pair)
__global__ __launch_bounds__(256) void sparse_pair_geometry(const SparseParams p, int32_t* __restrict__ pair_row,
                                                            int32_t* __restrict__ pair_cell, float* __restrict__ pair_scale) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= p.n_rows) return;
    const int64_t beg = p.rs[r], end = p.rs[r + 1];
    if (beg < 0 || end > p.n_pairs || end < beg) return;
    const float rx = p.row_pos[3 * r], ry = p.row_pos[3 * r + 1], rz = p.row_pos[3 * r + 2];
    const float rsv = p.rsc ? p.rsc[r] : 1.0f;
    for (int64_t q = beg; q < end; ++q) {
        const int32_t j = p.idx[q];
        if (j < 0 || j >= p.n_cols) continue;
        pair_row[q] = (int32_t)r;
        pair_cell[q] = sparse_cell(p, p.col_pos + 3 * (int64_t)j, rx, ry, rz);
        pair_scale[q] = rsv * (p.csc ? p.csc[j] : 1.0f);
    }
}

constexpr int kSpGradChunk = 8192;  // elements of dW a workgroup accumulates in LDS
constexpr int kSpStage = 4096;      // floats of staged operand rows per batch of pairs
constexpr int kSpBatchMax = 256;

// Workgroup (slab, chunk): the slab's pairs in order, batch by batch -- the batch's geometry and operand rows are staged in LDS
// by all threads, then every thread adds the batch's terms to ITS elements of the chunk, pair after pair.
// U: the operand with cw_in channels (x without W_TRANSPOSED, else grad_out), V: the one with cw_out channels.
__global__ __launch_bounds__(256) void sparse_filter_grad(const SparseParams p, const float* __restrict__ grad_out,
                                                          const int32_t* __restrict__ pair_row, const int32_t* __restrict__ pair_cell,
                                                          const float* __restrict__ pair_scale, int64_t slab_pairs, int batch,
                                                          int64_t T, float* __restrict__ partial) {
    __shared__ float part[kSpGradChunk];
    __shared__ float stage[kSpStage];
    __shared__ int32_t m_row[kSpBatchMax], m_col[kSpBatchMax], m_cell[kSpBatchMax];
    __shared__ float m_scale[kSpBatchMax];
    const int tid = threadIdx.x;
    const int64_t e0 = (int64_t)blockIdx.y * kSpGradChunk, e1 = min(T, e0 + kSpGradChunk);
    const int64_t q0 = (int64_t)blockIdx.x * slab_pairs, q1 = min(p.n_pairs, q0 + slab_pairs);
    const int64_t CC = (int64_t)p.cw_in * p.cw_out;
    const int cu = p.cw_in, cv = p.cw_out;
    float* U = stage;
    float* V = stage + (int64_t)batch * cu;
    for (int e = tid; e < kSpGradChunk; e += 256) part[e] = 0.0f;
    for (int64_t b0 = q0; b0 < q1; b0 += batch) {
        const int nb = (int)min((int64_t)batch, q1 - b0);
        __syncthreads();  // the previous batch is consumed (and, first, the chunk is cleared)
        for (int b = tid; b < nb; b += 256) {
            int32_t row = pair_row[b0 + b], cell = 0;
            if (row >= 0) {
                cell = pair_cell[b0 + b];
                if (cell * CC >= e1 || (cell + 1) * CC <= e0) row = -1;  // not in this chunk
            }
            m_row[b] = row;
            m_cell[b] = cell;
            m_col[b] = row >= 0 ? p.idx[b0 + b] : 0;
            m_scale[b] = row >= 0 ? pair_scale[b0 + b] : 0.0f;
        }
        __syncthreads();
        for (int t = tid; t < nb * (cu + cv); t += 256) {
            const int b = t / (cu + cv), ch = t - b * (cu + cv);
            if (m_row[b] < 0) continue;
            const bool isu = ch < cu;
            const int c = isu ? ch : ch - cu;
            // (isu == transposed: the operand comes from grad_out, rows indexed by the pair's row)
            const bool from_g = isu == (p.transposed != 0);
            const float v = from_g ? grad_out[(int64_t)m_row[b] * (isu ? cu : cv) + c] : p.x[(int64_t)m_col[b] * (isu ? cu : cv) + c];
            (isu ? U[b * cu + c] : V[b * cv + c]) = v;
        }
        __syncthreads();
        for (int b = 0; b < nb; ++b) {
            if (m_row[b] < 0) continue;  // (uniform)
            const int64_t cbase = (int64_t)m_cell[b] * CC;
            const int64_t lo = max(cbase, e0), hi = min(cbase + CC, e1);
            const float s = m_scale[b];
            for (int64_t e = lo + tid; e < hi; e += 256) {
                const int ab = (int)(e - cbase);
                const int a = ab / cv, bb = ab - a * cv;
                part[e - e0] += (s * U[b * cu + a]) * V[b * cv + bb];
            }
        }
    }
    __syncthreads();
    for (int64_t e = e0 + tid; e < e1; e += 256) partial[(int64_t)blockIdx.x * T + e] = part[e - e0];
}

__global__ __launch_bounds__(256) void sparse_filter_reduce(const float* __restrict__ partial, int nslabs, int64_t T,
                                                            float* __restrict__ grad_filters) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= T) return;
    float s = 0.0f;
    for (int k = 0; k < nslabs; ++k) s += partial[(int64_t)k * T + e];
    grad_filters[e] = s;
}

}  // namespace dmcf

using namespace dmcf;

static constexpr int kSparseFlags = DMCF_SPARSE_NEGATE | DMCF_SPARSE_W_TRANSPOSED | DMCF_SPARSE_ACCUMULATE;
static constexpr int64_t kSlabPairsMin = 512;
static constexpr int64_t kSlabsMax = 512;

// `out` is not needed for the backward
static int sparse_validate(const dmcf_sparse_conv_args* a, bool need_out) {
    if (!a || a->struct_size < sizeof(dmcf_sparse_conv_args)) return DMCF_EINVAL;
    if (a->flags & ~kSparseFlags) return DMCF_EINVAL;
    int64_t k = 1;
    for (int i = 0; i < 5; ++i) {
        if (a->filter_dims[i] <= 0) return DMCF_EINVAL;
        if (i < 3) k *= a->filter_dims[i];
    }
    if (a->n_rows < 0 || a->n_cols < 0 || a->n_pairs < 0 || !(a->extent > 0.0f)) return DMCF_EINVAL;
    for (int i = 0; i < 3; ++i)
        if (!(a->offset[i] == a->offset[i]) || a->offset[i] > 1e6f || a->offset[i] < -1e6f) return DMCF_EINVAL;
    if (!a->filters) return DMCF_EINVAL;
    if (a->n_rows > 0 && (!a->row_positions || !a->neighbors_row_splits || (need_out && !a->out))) return DMCF_EINVAL;
    if (a->n_pairs > 0 && (!a->neighbors_index || !a->col_positions || !a->col_features)) return DMCF_EINVAL;
    // cell * Cin * Cout is an int64 in the kernels; the counts themselves are ints
    if (k > (1 << 20) || a->n_cols > 0x7fffffff || a->n_rows > 0x7fffffff) return DMCF_EUNSUPPORTED;
    if ((a->n_rows + 63) / 64 > 0x7fffffff) return DMCF_EUNSUPPORTED;
    return DMCF_OK;
}

static SparseParams sparse_params(const dmcf_sparse_conv_args* a) {
    SparseParams p;
    p.W = a->filters;
    p.kz = a->filter_dims[0];
    p.ky = a->filter_dims[1];
    p.kx = a->filter_dims[2];
    p.K = p.kx * p.ky * p.kz;
    p.cw_in = a->filter_dims[3];
    p.cw_out = a->filter_dims[4];
    p.transposed = (a->flags & DMCF_SPARSE_W_TRANSPOSED) ? 1 : 0;
    p.cin = p.transposed ? p.cw_out : p.cw_in;
    p.cout = p.transposed ? p.cw_in : p.cw_out;
    p.row_pos = a->row_positions;
    p.col_pos = a->col_positions;
    p.x = a->col_features;
    p.rsc = a->row_scale;
    p.csc = a->col_scale;
    p.idx = a->neighbors_index;
    p.rs = a->neighbors_row_splits;
    p.n_rows = a->n_rows;
    p.n_cols = a->n_cols;
    p.n_pairs = a->n_pairs;
    p.inv_extent = 1.0f / a->extent;
    p.sign = (a->flags & DMCF_SPARSE_NEGATE) ? -1.0f : 1.0f;
    for (int i = 0; i < 3; ++i) p.off[i] = a->offset[i];
    p.bias = a->bias;
    p.out = a->out;
    p.accumulate = (a->flags & DMCF_SPARSE_ACCUMULATE) ? 1 : 0;
    return p;
}

static void sparse_set_chunks(SparseParams& p) {
    const int cin4 = (p.cin + 3) & ~3;
    p.CW = cin4 < kSpChunk ? cin4 : kSpChunk;
    p.ncc = (cin4 + p.CW - 1) / p.CW;
    p.cpc = kSpChunk / p.CW;
}

static int sparse_launch_forward(SparseParams p, hipStream_t stream) {
    if (p.n_rows == 0) return DMCF_OK;
    sparse_set_chunks(p);
    const unsigned g = (unsigned)((p.n_rows + 63) / 64);
    hipLaunchKernelGGL(sparse_conv_kernel, dim3(g), dim3(256), 0, stream, p);
    return check_launch();
}

struct SparseBwdLayout {
    int64_t T, slab_pairs;
    int nslabs;
    size_t off_row, off_cell, off_scale, off_partial, total;
};

static SparseBwdLayout sparse_bwd_layout(const dmcf_sparse_conv_args* a, bool want_filters) {
    SparseBwdLayout L;
    L.T = (int64_t)a->filter_dims[0] * a->filter_dims[1] * a->filter_dims[2] * a->filter_dims[3] * a->filter_dims[4];
    const int64_t P = a->n_pairs;
    L.slab_pairs = (P + kSlabsMax - 1) / kSlabsMax;
    if (L.slab_pairs < kSlabPairsMin) L.slab_pairs = kSlabPairsMin;
    L.nslabs = (int)((P + L.slab_pairs - 1) / L.slab_pairs);
    if (L.nslabs < 1) L.nslabs = 1;
    size_t off = 0;
    const size_t per = align_up((size_t)(P > 0 ? P : 1) * 4, 256);
    L.off_row = off;      off += want_filters ? per : 0;
    L.off_cell = off;     off += want_filters ? per : 0;
    L.off_scale = off;    off += want_filters ? per : 0;
    L.off_partial = off;  off += want_filters ? align_up((size_t)L.nslabs * (size_t)L.T * 4, 256) : 0;
    L.total = off;
    return L;
}

// limits of the filter gradient: int element indices inside a cell, staged operand rows
static bool sparse_filter_grad_supported(const dmcf_sparse_conv_args* a) {
    const int64_t cc = (int64_t)a->filter_dims[3] * a->filter_dims[4];
    const int64_t T = cc * a->filter_dims[0] * a->filter_dims[1] * a->filter_dims[2];
    return cc < ((int64_t)1 << 30) && T < ((int64_t)1 << 40) && a->filter_dims[3] + a->filter_dims[4] <= kSpStage &&
           (T + kSpGradChunk - 1) / kSpGradChunk <= 65535;
}

extern "C" {

int dmcf_sparse_conv_forward(const dmcf_sparse_conv_args* a, dmcf_stream_t stream_) {
    const int rc = sparse_validate(a, true);
    if (rc != DMCF_OK) return rc;
    return sparse_launch_forward(sparse_params(a), (hipStream_t)stream_);
}

size_t dmcf_sparse_conv_backward_workspace_bytes(const dmcf_sparse_conv_args* fwd, int want_grad_filters) {
    if (sparse_validate(fwd, false) != DMCF_OK) return 0;
    return sparse_bwd_layout(fwd, want_grad_filters != 0).total;
}

int dmcf_sparse_conv_backward(const dmcf_sparse_conv_args* fwd, const float* grad_out, const int32_t* inv_index,
                              const int64_t* inv_row_splits, int64_t inv_n_pairs, float* grad_filters, float* grad_col_features,
                              void* workspace, size_t workspace_bytes, dmcf_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const int rc = sparse_validate(fwd, false);
    if (rc != DMCF_OK) return rc;
    if (!grad_filters && !grad_col_features) return DMCF_EINVAL;
    if (fwd->n_rows > 0 && !grad_out) return DMCF_EINVAL;
    if (grad_col_features && (inv_n_pairs < 0 || (fwd->n_cols > 0 && !inv_row_splits) || (inv_n_pairs > 0 && !inv_index)))
        return DMCF_EINVAL;
    if (grad_filters && !sparse_filter_grad_supported(fwd)) return DMCF_EUNSUPPORTED;
    const SparseBwdLayout L = sparse_bwd_layout(fwd, grad_filters != nullptr);
    if (L.total > 0 && (!workspace || workspace_bytes < L.total)) return DMCF_EWORKSPACE;
    if (workspace && ((uintptr_t)workspace & 15) != 0) return DMCF_EINVAL;
    SparseParams p = sparse_params(fwd);
    p.bias = nullptr;
    p.accumulate = 0;
    if (grad_filters) {
        char* ws = (char*)workspace;
        if (p.n_pairs == 0 || p.n_rows == 0) {
            if (hipMemsetAsync(grad_filters, 0, (size_t)L.T * 4, stream) != hipSuccess) return DMCF_ELAUNCH;
        } else {
            int32_t* pair_row = (int32_t*)(ws + L.off_row);
            int32_t* pair_cell = (int32_t*)(ws + L.off_cell);
            float* pair_scale = (float*)(ws + L.off_scale);
            float* partial = (float*)(ws + L.off_partial);
            if (hipMemsetAsync(pair_row, 0xff, (size_t)p.n_pairs * 4, stream) != hipSuccess) return DMCF_ELAUNCH;
            hipLaunchKernelGGL(sparse_pair_geometry, dim3((unsigned)((p.n_rows + 255) / 256)), dim3(256), 0, stream, p, pair_row, pair_cell,
                               pair_scale);
            int batch = kSpStage / (p.cw_in + p.cw_out);
            if (batch > kSpBatchMax) batch = kSpBatchMax;
            const unsigned nchunks = (unsigned)((L.T + kSpGradChunk - 1) / kSpGradChunk);
            hipLaunchKernelGGL(sparse_filter_grad, dim3((unsigned)L.nslabs, nchunks), dim3(256), 0, stream, p, grad_out,
                               (const int32_t*)pair_row, (const int32_t*)pair_cell, (const float*)pair_scale, L.slab_pairs, batch, L.T,
                               partial);
            hipLaunchKernelGGL(sparse_filter_reduce, dim3((unsigned)((L.T + 255) / 256)), dim3(256), 0, stream, (const float*)partial,
                               L.nslabs, L.T, grad_filters);
        }
    }
    if (grad_col_features && (p.n_pairs == 0 || p.n_rows == 0 || inv_n_pairs == 0)) {
        // no pair: zeros, without a launch (col_positions, the rows of that launch, is only required with pairs)
        if (p.n_cols > 0 && hipMemsetAsync(grad_col_features, 0, (size_t)p.n_cols * p.cin * 4, stream) != hipSuccess) return DMCF_ELAUNCH;
    } else if (grad_col_features) {
        // the same operator over the inverted list: rows and columns swapped, the other sign, W the other way round
        SparseParams t = p;
        t.transposed = !p.transposed;
        t.cin = p.cout;
        t.cout = p.cin;
        t.row_pos = p.col_pos;
        t.col_pos = p.row_pos;
        t.x = grad_out;
        t.rsc = p.csc;
        t.csc = p.rsc;
        t.idx = inv_index;
        t.rs = inv_row_splits;
        t.n_rows = p.n_cols;
        t.n_cols = p.n_rows;
        t.n_pairs = inv_n_pairs;
        t.sign = -p.sign;
        t.out = grad_col_features;
        const int rc2 = sparse_launch_forward(t, stream);
        if (rc2 != DMCF_OK) return rc2;
    }
    return check_launch();
}

int dmcf_sparse_conv_kernel_names(const dmcf_sparse_conv_args* args, int backward, char* names, size_t name_bytes) {
    const int rc = sparse_validate(args, false);
    if (rc != DMCF_OK) return rc;
    if (!names || name_bytes == 0 || backward < 0 || backward > 3) return DMCF_EINVAL;
    const char* s = "sparse_conv_kernel";
    if (backward == 1) s = "sparse_pair_geometry;sparse_filter_grad;sparse_filter_reduce";
    if (backward == 2) s = "sparse_conv_kernel";
    if (backward == 3) s = "sparse_pair_geometry;sparse_filter_grad;sparse_filter_reduce;sparse_conv_kernel";
    if (strlen(s) + 1 > name_bytes) return DMCF_EINVAL;
    memcpy(names, s, strlen(s) + 1);
    return DMCF_OK;
}

}  // extern "C"
