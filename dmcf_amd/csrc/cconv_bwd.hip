// Backward pass of CConv / ASCC (dmcf_cconv_backward) and the neighbour-list inversion it walks (dmcf_invert_neighbors_list).
//
// Replaces the two gradients Open3D 0.15.2 registers for ml3d.ops.continuous_conv: continuous_conv_backprop_filter (filters)
// and invert_neighbors_list + continuous_conv_transpose (input features).  Positions, extents and importances get no gradient,
// as there.  With G = dL/d out [n_out, Cout], pair p = (output row i, input j), corner weights w_c(p), pair weight a_p (window,
// times s_j when there is a point importance) and row normaliser psi_i (1 without DMCF_FLAG_NORMALIZE, and where psi_i == 0):
//   dF[j,:] = sum_{p -> j} (a_p / psi_i) sum_c w_c(p) W_c G[i,:]                     (input features)
//   dW_c    = sum_i B_i[c]^T G[i],   B_i[c,:] = sum_{p in row i} (a_p / psi_i) w_c(p) f_j   (filters)
// ASCC (DMCF_FLAG_SYMMETRIC, pair features f_j + f_i on the mirrored full kernel g) adds the centre term
//   dF[i,:] += sum_{p in row i} (a_p / psi_i) sum_c w_c(p) g_c G[i,:]
// takes B on (f_j + f_i), and folds the full-kernel gradient onto the stored half: dHalf = dFull[upper] - flip_zyx(dFull[lower]).
//
// Every pair's geometry (x_j - x_i, window, mapping, interpolation weights) is formed with the operations, in the order, of
// the generic forward body (cconv_generic_body.inc); psi_i is summed in that kernel's order too.  Only the order of the sums
// of the gradients differs from a forward.  Nothing uses float atomics: every output element is written by one thread, and
// the filter gradient is reduced from per-workgroup slabs in a fixed order, so two identical calls give the same bits.
//
// Kernels (the names dmcf_cconv_backward_kernel_names reports):
//   cconv_bwd_norm          psi_i per output row (NORMALIZE only), one half-wave per row as in the forward
//   cconv_bwd_expand        ASCC: the mirrored full kernel [K, Cin, Cout] (the layout the input-feature gradient reads)
//   cconv_bwd_input         one wave per input row j: splat (a_p / psi_i) G[i] over the 8 corners into T_j [K, Cout] (LDS),
//                           walking the inverted list (and, for ASCC, row j of the forward list), then dF_j = sum_c W_c T_j[c]
//   cconv_bwd_filter_splat  one wave per output row i: B_i [K, Cin] in LDS, written to a chunk buffer [rows, K * Cin]
//   cconv_bwd_filter_gemm   per chunk: slab s = sum over its rows of B_r^T G_r, 64 x 64 tiles, one slab per z-block
//   cconv_bwd_filter_reduce per chunk: the slabs summed in slab order into the full-kernel gradient
//   cconv_bwd_filter_store  the full-kernel gradient (folded for ASCC) written, or added, to grad_filters
// Individual extents (dmcf_cconv_backward_extents): the kernels that form a pair's geometry -- cconv_bwd_norm, cconv_bwd_input,
// cconv_bwd_filter_splat -- have a second entry point each (suffix _ext) over the same body, in which 1 / e_i and 1 / (e_i / 2)^2
// of the pair's OUTPUT row i replace p.inv_extent / p.inv_r2 (the arithmetic of the forward's EXT body, cconv_generic_body.inc);
// a row whose extent is not positive and finite is an empty row.  The other kernels never see an extent.
// Inversion: a stable rocPRIM radix sort of (input index, pair index) pairs keyed by input index, then a binary search per
// input row for the row splits (invert_keys, invert_splits, invert_gather).
#include <rocprim/device/device_radix_sort.hpp>

#include <stdio.h>
#include <string.h>

#include "cconv_common.h"

namespace dmcf {

constexpr int kBwdWStride = 9;                 // staged floats per pair: 8 corner weights + 1 pad (bank spread)
constexpr int kBwdLdsFloats = 16384;           // K * max(Cin, Cout) limit: 64 KiB of LDS per wave
constexpr size_t kBwdChunkFloats = (size_t)1 << 28;  // B chunk: at most 1 GiB
constexpr int kBwdMaxSlabs = 256;
constexpr int kBwdSlabRows = 256;              // at least this many rows per slab

struct BwdGeo {
    int K, cin, cout;
    int off[8];       // corner offsets from the base cell, in cells
    uint32_t live;    // bit t: corner t exists (a "+1" corner along an axis of size 1 does not)
};

// The pair's geometry, as the generic forward body forms it: returns a_p (window, SKIP_SELF, importance), the base cell and
// the 8 corner weights in Open3D's product order.  inv_extent, inv_r2: of the pair's output row (bwd_row_extent).
__device__ __forceinline__ float bwd_pair(const CconvParams& p, int64_t i, int j, int64_t pp, float ox, float oy, float oz,
                                          float inv_extent, float inv_r2, int& base, float (&w)[8]) {
    const float gx = p.inp_pos[3 * (int64_t)j], gy = p.inp_pos[3 * (int64_t)j + 1], gz = p.inp_pos[3 * (int64_t)j + 2];
    float x = gx - ox;
    float y = gy - oy;
    float z = gz - oz;
    float a = window_value(p.window, p.nval ? p.nval[pp] : rel_dist2(x, y, z), inv_r2, p.window_fac);
    if ((p.flags & DMCF_FLAG_SKIP_SELF) && ((x == 0.0f && y == 0.0f && z == 0.0f) || j == (int)i)) a = 0.0f;
    if (p.inp_imp) a *= p.inp_imp[j];
    filter_coords<true>(x, y, z, p, inv_extent);
    int bx, by, bz;
    float wx0, wx1, wy0, wy1, wz0, wz1;
    axis_weights(x, p.sx, p.interp, bx, wx0, wx1);
    axis_weights(y, p.sy, p.interp, by, wy0, wy1);
    axis_weights(z, p.sz, p.interp, bz, wz0, wz1);
    base = (bz * p.sy + by) * p.sx + bx;
    const float w00 = wx0 * wy0, w10 = wx1 * wy0, w01 = wx0 * wy1, w11 = wx1 * wy1;
    w[0] = w00 * wz0; w[1] = w10 * wz0; w[2] = w01 * wz0; w[3] = w11 * wz0;
    w[4] = w00 * wz1; w[5] = w10 * wz1; w[6] = w01 * wz1; w[7] = w11 * wz1;
    return a;
}

// window value of a pair before the importance: what the forward sums into psi_i
__device__ __forceinline__ float bwd_norm_term(const CconvParams& p, int64_t i, int j, int64_t pp, float ox, float oy, float oz,
                                               float inv_r2) {
    const float x = p.inp_pos[3 * (int64_t)j] - ox, y = p.inp_pos[3 * (int64_t)j + 1] - oy, z = p.inp_pos[3 * (int64_t)j + 2] - oz;
    float a = window_value(p.window, p.nval ? p.nval[pp] : rel_dist2(x, y, z), inv_r2, p.window_fac);
    if ((p.flags & DMCF_FLAG_SKIP_SELF) && ((x == 0.0f && y == 0.0f && z == 0.0f) || j == (int)i)) a = 0.0f;
    return a;
}

__device__ __forceinline__ void bwd_row(const CconvParams& p, int64_t i, int64_t& rb, int64_t& re) {
    rb = p.rs[i];
    re = p.cnt ? rb + p.cnt[i] : p.rs[i + 1];
    if (re > p.pair_cap || rb < 0 || re < rb) re = rb;
}

__device__ __forceinline__ bool bwd_valid_j(const CconvParams& p, int j) { return j >= 0 && (int64_t)j < p.n_inp; }

// 1 / e_i and 1 / (e_i / 2)^2 of output row i.  EXT: from out_ext[i], with the operations of the forward's EXT body (which are
// the host's of dmcf_cconv_forward for a scalar); false: the extent is not positive and finite -- the row is empty, as there.
// !EXT: the call's two constants.
template <bool EXT>
__device__ __forceinline__ bool bwd_row_extent(const CconvParams& p, const float* __restrict__ out_ext, int64_t i, float& inv_extent,
                                               float& inv_r2) {
    if (!EXT) {
        inv_extent = p.inv_extent;
        inv_r2 = p.inv_r2;
        return true;
    }
    const float e = out_ext[i];
    inv_extent = __fdiv_rn(1.0f, e);
    const float radius = __fmul_rn(0.5f, e);
    inv_r2 = __fdiv_rn(1.0f, __fmul_rn(radius, radius));
    return e > 0.0f && isfinite(e);
}

// The three kernels below have two entry points over one body each (cconv_bwd_*_body.inc, included rather than called: through
// a shared __device__ function the scalar kernels compile to other code than they did on their own, see cconv_generic_body.inc).

// psi_i: the forward's half-wave sum (lane pl takes pairs rb + pl, rb + pl + 32, ..., then a butterfly)
__global__ __launch_bounds__(64) void cconv_bwd_norm(const CconvParams p, float* __restrict__ psi) {
    constexpr bool EXT = false;
    const float* const out_ext = nullptr;
#include "cconv_bwd_norm_body.inc"
}

__global__ __launch_bounds__(64) void cconv_bwd_norm_ext(const CconvParams p, const float* __restrict__ out_ext,
                                                         float* __restrict__ psi) {
    constexpr bool EXT = true;
#include "cconv_bwd_norm_body.inc"
}

__device__ __forceinline__ float bwd_scale(const float* psi, int64_t i) {
    if (!psi) return 1.0f;
    const float v = psi[i];
    return v != 0.0f ? v : 1.0f;
}

// full[K, Cin, Cout] from the stored half kernel (the mirror of pack_filter: g = concat([-flip_zyx(W), W], sym_axis))
__global__ void cconv_bwd_expand(const float* __restrict__ half, float* __restrict__ full, int d0, int d1, int d2, int cin,
                                 int cout, int sym_axis) {
    const int hd[3] = {sym_axis == 0 ? d0 / 2 : d0, sym_axis == 1 ? d1 / 2 : d1, sym_axis == 2 ? d2 / 2 : d2};
    const int64_t total = (int64_t)d0 * d1 * d2 * cin * cout;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t co = e % ((int64_t)cin * cout);
        const int cell = (int)(e / ((int64_t)cin * cout));
        int c3[3] = {cell / (d1 * d2), (cell / d2) % d1, cell % d2};
        float sign = 1.0f;
        const int hh = hd[sym_axis];
        if (c3[sym_axis] >= hh) {
            c3[sym_axis] -= hh;
        } else {
            sign = -1.0f;
            for (int a = 0; a < 3; ++a) c3[a] = hd[a] - 1 - c3[a];
        }
        full[e] = sign * half[((int64_t)(c3[0] * hd[1] + c3[1]) * hd[2] + c3[2]) * cin * cout + co];
    }
}

// Stages up to 64 pairs (one per lane): corner weights times coef, base cell, partner index.  Invalid lanes stage zeros.
__device__ __forceinline__ void bwd_stage(float* ws, int* bs, int* js, int lane, bool valid, float coef, int base,
                                          const float (&w)[8], int partner) {
#pragma unroll
    for (int t = 0; t < 8; ++t) ws[lane * kBwdWStride + t] = valid ? w[t] * coef : 0.0f;
    bs[lane] = valid ? base : 0;
    js[lane] = valid ? partner : 0;
}

// Input-feature gradient: one wave per input row j.  EXT: a pair takes the constants of ITS output row -- one more load per
// pair (out_ext[i], next to out_pos[3 * i]) and two divisions, in the lane that forms the pair's geometry.
__global__ __launch_bounds__(64) void cconv_bwd_input(const CconvParams p, const BwdGeo geo, const float* __restrict__ Wfull,
                                                      const float* __restrict__ G, const float* __restrict__ psi,
                                                      const int32_t* __restrict__ inv_index, const int32_t* __restrict__ inv_pair,
                                                      const int64_t* __restrict__ inv_rs, int64_t inv_n_pairs, int symmetric,
                                                      float* __restrict__ dF, int accumulate) {
    constexpr bool EXT = false;
    const float* const out_ext = nullptr;
#include "cconv_bwd_input_body.inc"
}

__global__ __launch_bounds__(64) void cconv_bwd_input_ext(const CconvParams p, const BwdGeo geo, const float* __restrict__ out_ext,
                                                          const float* __restrict__ Wfull, const float* __restrict__ G,
                                                          const float* __restrict__ psi, const int32_t* __restrict__ inv_index,
                                                          const int32_t* __restrict__ inv_pair, const int64_t* __restrict__ inv_rs,
                                                          int64_t inv_n_pairs, int symmetric, float* __restrict__ dF,
                                                          int accumulate) {
    constexpr bool EXT = true;
#include "cconv_bwd_input_body.inc"
}

// Filter gradient, step 1: B_i [K, Cin] of output rows row0 .. row0 + gridDim.x - 1 into Bc [rows][K * Cin].
__global__ __launch_bounds__(64) void cconv_bwd_filter_splat(const CconvParams p, const BwdGeo geo, const float* __restrict__ psi,
                                                             int symmetric, int64_t row0, float* __restrict__ Bc) {
    constexpr bool EXT = false;
    const float* const out_ext = nullptr;
#include "cconv_bwd_filter_splat_body.inc"
}

__global__ __launch_bounds__(64) void cconv_bwd_filter_splat_ext(const CconvParams p, const BwdGeo geo,
                                                                 const float* __restrict__ out_ext, const float* __restrict__ psi,
                                                                 int symmetric, int64_t row0, float* __restrict__ Bc) {
    constexpr bool EXT = true;
#include "cconv_bwd_filter_splat_body.inc"
}

// Filter gradient, step 2: slab[z] [M, cout] = sum over rows r of slab z of Bc[r, :]^T G[row0 + r, :]; 64 x 64 tiles of
// 4 x 4 per thread.
__global__ __launch_bounds__(256) void cconv_bwd_filter_gemm(const float* __restrict__ Bc, const float* __restrict__ G, int64_t rows,
                                                             int M, int cout, int64_t rows_per_slab, float* __restrict__ slabs) {
    __shared__ float As[16][64];
    __shared__ float Gs[16][64];
    const int tid = threadIdx.x, tm = tid >> 4, tn = tid & 15;
    const int m0 = blockIdx.x * 64, n0 = blockIdx.y * 64;
    const int64_t r0 = (int64_t)blockIdx.z * rows_per_slab;
    const int64_t r1 = min(rows, r0 + rows_per_slab);
    float acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = 0.0f;
    for (int64_t rr = r0; rr < r1; rr += 16) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int e = tid + 256 * k, r = e >> 6, c = e & 63;
            const bool rok = rr + r < r1;
            As[r][c] = (rok && m0 + c < M) ? Bc[(rr + r) * M + m0 + c] : 0.0f;
            Gs[r][c] = (rok && n0 + c < cout) ? G[(rr + r) * cout + n0 + c] : 0.0f;
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float av[4], gv[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) av[a] = As[r][tm * 4 + a];
#pragma unroll
            for (int b = 0; b < 4; ++b) gv[b] = Gs[r][tn * 4 + b];
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) acc[a][b] += av[a] * gv[b];
        }
        __syncthreads();
    }
    float* out = slabs + (size_t)blockIdx.z * M * cout;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int m = m0 + tm * 4 + a;
        if (m >= M) continue;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int n = n0 + tn * 4 + b;
            if (n < cout) out[(size_t)m * cout + n] = acc[a][b];
        }
    }
}

// Filter gradient, step 3: dfull (+)= sum of the slabs in slab order
__global__ void cconv_bwd_filter_reduce(const float* __restrict__ slabs, int nslabs, int64_t n, float* __restrict__ dfull, int first) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        float v = 0.0f;
        for (int s = 0; s < nslabs; ++s) v += slabs[(size_t)s * n + e];
        dfull[e] = first ? v : dfull[e] + v;
    }
}

// Filter gradient, step 4: grad_filters (+)= dfull, folded onto the stored half for ASCC
__global__ void cconv_bwd_filter_store(const float* __restrict__ dfull, float* __restrict__ dW, int d0, int d1, int d2, int cin,
                                       int cout, int symmetric, int sym_axis, int accumulate) {
    // d0..d2: full dims
    const int hd[3] = {symmetric && sym_axis == 0 ? d0 / 2 : d0, symmetric && sym_axis == 1 ? d1 / 2 : d1,
                       symmetric && sym_axis == 2 ? d2 / 2 : d2};
    const int64_t cc = (int64_t)cin * cout;
    const int64_t total = (int64_t)hd[0] * hd[1] * hd[2] * cc;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        float v;
        if (!symmetric) {
            v = dfull[e];
        } else {
            const int64_t co = e % cc;
            const int cell = (int)(e / cc);
            const int h3[3] = {cell / (hd[1] * hd[2]), (cell / hd[2]) % hd[1], cell % hd[2]};
            int up[3] = {h3[0], h3[1], h3[2]};
            up[sym_axis] += hd[sym_axis];
            const int lo[3] = {hd[0] - 1 - h3[0], hd[1] - 1 - h3[1], hd[2] - 1 - h3[2]};
            const float vu = dfull[((int64_t)(up[0] * d1 + up[1]) * d2 + up[2]) * cc + co];
            const float vl = dfull[((int64_t)(lo[0] * d1 + lo[1]) * d2 + lo[2]) * cc + co];
            v = vu - vl;
        }
        dW[e] = accumulate ? dW[e] + v : v;
    }
}

// ---- inversion ----
__global__ void invert_init(uint32_t* __restrict__ keys, int32_t* __restrict__ vals, int64_t n, uint32_t fill) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        keys[e] = fill;
        vals[e] = (int32_t)e;
    }
}

__global__ void invert_keys(const int32_t* __restrict__ idx, const int64_t* __restrict__ rs, const int32_t* __restrict__ cnt,
                            int64_t n_out, int64_t n_inp, int64_t n_pairs, uint32_t* __restrict__ keys, int32_t* __restrict__ row_of) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_out) return;
    const int64_t rb = rs[i];
    int64_t re = cnt ? rb + cnt[i] : rs[i + 1];
    if (re > n_pairs || rb < 0 || re < rb) re = rb;
    for (int64_t pp = rb; pp < re; ++pp) {
        const int j = idx[pp];
        keys[pp] = (j >= 0 && (int64_t)j < n_inp) ? (uint32_t)j : (uint32_t)n_inp;
        row_of[pp] = (int32_t)i;
    }
}

__global__ void invert_splits(const uint32_t* __restrict__ skeys, int64_t n_pairs, int64_t n_inp, int64_t* __restrict__ splits) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j > n_inp) return;
    int64_t lo = 0, hi = n_pairs;  // first position with key >= j
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)skeys[mid] < j) lo = mid + 1; else hi = mid;
    }
    splits[j] = lo;
}

__global__ void invert_gather(const uint32_t* __restrict__ skeys, const int32_t* __restrict__ perm, const int32_t* __restrict__ row_of,
                              const float* __restrict__ values, int64_t n_pairs, int64_t n_inp, int32_t* __restrict__ inv_index,
                              int32_t* __restrict__ inv_pair, float* __restrict__ inv_values) {
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n_pairs; q += (int64_t)gridDim.x * blockDim.x) {
        const bool valid = (int64_t)skeys[q] < n_inp;
        const int32_t pp = perm[q];
        inv_index[q] = valid ? row_of[pp] : -1;
        if (inv_pair) inv_pair[q] = valid ? pp : -1;
        if (inv_values) inv_values[q] = (valid && values) ? values[pp] : 0.0f;
    }
}

static unsigned grid_for(int64_t n, int threads, unsigned cap = 4096) {
    const int64_t g = (n + threads - 1) / threads;
    return (unsigned)(g < 1 ? 1 : (g > cap ? cap : g));
}

static size_t invert_sort_tmp(int64_t n_pairs) {
    size_t bytes = 0;
    (void)rocprim::radix_sort_pairs((void*)nullptr, bytes, (const uint32_t*)nullptr, (uint32_t*)nullptr, (const int32_t*)nullptr,
                              (int32_t*)nullptr, (size_t)n_pairs, 0u, 32u, (hipStream_t)0);
    return bytes;
}

// ---- backward: validation and layout ----
struct BwdPlan {
    int dz, dy, dx, K, cin, cout, M;
    bool sym, want_f, want_w;
    int64_t R, rows_per_slab;
    int S;
    size_t off_psi, off_wfull, off_b, off_slabs, off_dfull, total;
    size_t lds_input, lds_splat;
};

static int bwd_plan(const dmcf_cconv_args* a, const dmcf_cconv_backward_args* b, BwdPlan& pl) {
    if (!a || !b) return DMCF_EINVAL;
    if (b->struct_size < sizeof(dmcf_cconv_backward_args)) return DMCF_EINVAL;
    for (int d = 0; d < 5; ++d)
        if (a->filter_dims[d] < 1) return DMCF_EINVAL;
    if (a->n_out < 0 || a->n_inp < 0 || a->n_pairs < 0) return DMCF_EINVAL;
    if (!(a->extent > 0.0f)) return DMCF_EINVAL;
    if (a->window < DMCF_WINDOW_NONE || a->window > DMCF_WINDOW_CUBIC_GRAD) return DMCF_EINVAL;
    if (a->coordinate_mapping < 0 || a->coordinate_mapping > 2) return DMCF_EINVAL;
    if (a->interpolation < 0 || a->interpolation > 2) return DMCF_EINVAL;
    if (b->flags & ~DMCF_BWD_ACCUMULATE) return DMCF_EINVAL;
    pl.sym = (a->flags & DMCF_FLAG_SYMMETRIC) != 0;
    if (pl.sym) {
        if (a->sym_axis < 0 || a->sym_axis > 2) return DMCF_EINVAL;
        if (a->n_inp < a->n_out) return DMCF_EINVAL;
    }
    pl.want_f = b->grad_inp_features != nullptr;
    pl.want_w = b->grad_filters != nullptr;
    if (a->n_out > 0) {
        if (!a->out_positions || !a->neighbors_row_splits || !b->grad_out) return DMCF_EINVAL;
        if (a->window == DMCF_WINDOW_EXPLICIT && !a->neighbors_value) return DMCF_EINVAL;
        if (a->n_pairs > 0 && !a->neighbors_index) return DMCF_EINVAL;
    }
    if (a->n_inp > 0 && !a->inp_positions) return DMCF_EINVAL;
    if (pl.want_w && a->n_inp > 0 && !a->inp_features) return DMCF_EINVAL;
    if (pl.want_f) {
        if (!a->filters) return DMCF_EINVAL;
        if (!b->inv_row_splits || b->inv_n_rows != a->n_inp || b->inv_n_pairs < 0) return DMCF_EINVAL;
        if (b->inv_n_pairs > 0 && (!b->inv_index || !b->inv_pair)) return DMCF_EINVAL;
    }
    if (pl.sym && a->n_inp != a->n_out) return DMCF_EUNSUPPORTED;  // the sharded layout (ghosts after the owned points)
    pl.dz = a->filter_dims[0]; pl.dy = a->filter_dims[1]; pl.dx = a->filter_dims[2];
    if (pl.sym) {
        if (a->sym_axis == 0) pl.dz *= 2;
        if (a->sym_axis == 1) pl.dy *= 2;
        if (a->sym_axis == 2) pl.dx *= 2;
    }
    pl.cin = a->filter_dims[3];
    pl.cout = a->filter_dims[4];
    const int64_t K = (int64_t)pl.dz * pl.dy * pl.dx;
    if (K * pl.cin > kBwdLdsFloats || K * pl.cout > kBwdLdsFloats) return DMCF_EUNSUPPORTED;
    if (a->n_pairs > 0x7fffffffLL || a->n_out > 0x7fffffffLL || a->n_inp >= 0x7fffffffLL) return DMCF_EUNSUPPORTED;
    pl.K = (int)K;
    pl.M = pl.K * pl.cin;
    const size_t full = (size_t)pl.M * pl.cout;
    pl.R = a->n_out < 1 ? 1 : a->n_out;
    const int64_t rmax = (int64_t)(kBwdChunkFloats / (size_t)pl.M);
    if (pl.R > rmax) pl.R = rmax;
    int64_t S = (pl.R + kBwdSlabRows - 1) / kBwdSlabRows;
    if (S > kBwdMaxSlabs) S = kBwdMaxSlabs;
    pl.S = (int)S;
    pl.rows_per_slab = (pl.R + S - 1) / S;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += align_up(bytes, 256); return o; };
    pl.off_psi = take(sizeof(float) * (size_t)(a->n_out > 0 ? a->n_out : 1));
    pl.off_wfull = take(pl.sym && pl.want_f ? sizeof(float) * full : 0);
    pl.off_b = take(pl.want_w ? sizeof(float) * (size_t)pl.R * pl.M : 0);
    pl.off_slabs = take(pl.want_w ? sizeof(float) * (size_t)pl.S * full : 0);
    pl.off_dfull = take(pl.want_w ? sizeof(float) * full : 0);
    pl.total = off + 256;
    pl.lds_input = sizeof(float) * ((size_t)pl.K * pl.cout + 64 * kBwdWStride + 64) + 2 * 64 * sizeof(int);
    pl.lds_splat = sizeof(float) * ((size_t)pl.K * pl.cin + 64 * kBwdWStride) + 2 * 64 * sizeof(int);
    return DMCF_OK;
}

static void bwd_params(const dmcf_cconv_args* a, const BwdPlan& pl, CconvParams& p, BwdGeo& geo) {
    memset(&p, 0, sizeof(p));
    p.sx = pl.dx; p.sy = pl.dy; p.sz = pl.dz;
    p.K = pl.K; p.cin = pl.cin; p.cout = pl.cout;
    p.out_pos = a->out_positions;
    p.inp_pos = a->inp_positions;
    p.inp_feat = a->inp_features;
    p.inp_imp = a->inp_importance;
    p.idx = a->neighbors_index;
    p.rs = a->neighbors_row_splits;
    p.cnt = a->neighbors_row_count;
    p.nval = a->neighbors_value;
    p.n_out = a->n_out;
    p.n_inp = a->n_inp;
    p.pair_cap = a->n_pairs;
    // the host arithmetic of dmcf_cconv_forward
    p.inv_extent = 1.0f / a->extent;
    const float radius = 0.5f * a->extent;
    p.inv_r2 = 1.0f / (radius * radius);
    p.window_fac = a->window_fac;
    p.window = a->window;
    p.mapping = a->coordinate_mapping;
    p.interp = a->interpolation;
    p.flags = a->flags;
    geo.K = pl.K; geo.cin = pl.cin; geo.cout = pl.cout;
    geo.live = 0;
    for (int t = 0; t < 8; ++t) {
        const int tx = t & 1, ty = (t >> 1) & 1, tz = (t >> 2) & 1;
        const bool live = !((tx && pl.dx < 2) || (ty && pl.dy < 2) || (tz && pl.dz < 2));
        geo.off[t] = live ? (tz * pl.dy + ty) * pl.dx + tx : 0;
        if (live) geo.live |= 1u << t;
    }
}

// dmcf_cconv_backward (out_ext == NULL) and dmcf_cconv_backward_extents: one sequence of launches, the three kernels that form
// pair geometry in their _ext form when there is an extent per output row.
static int bwd_run(const dmcf_cconv_args* a, const dmcf_cconv_backward_args* b, const BwdPlan& pl, const float* out_ext,
                   void* workspace, size_t workspace_bytes, hipStream_t stream) {
    int rc = DMCF_OK;
    if (!pl.want_f && !pl.want_w) return DMCF_OK;
    if (!workspace || ((uintptr_t)workspace & 255)) return DMCF_EINVAL;
    if (workspace_bytes < pl.total) return DMCF_EWORKSPACE;
    const int accumulate = (b->flags & DMCF_BWD_ACCUMULATE) ? 1 : 0;
    char* w = (char*)workspace;
    const int64_t n_full = (int64_t)pl.M * pl.cout;
    const int64_t n_stored = (int64_t)a->filter_dims[0] * a->filter_dims[1] * a->filter_dims[2] * pl.cin * pl.cout;
    // empty point sets: the gradients are zero
    if (a->n_out == 0 || a->n_inp == 0) {
        hipError_t e = hipSuccess;
        if (pl.want_w && !accumulate) e = hipMemsetAsync(b->grad_filters, 0, sizeof(float) * (size_t)n_stored, stream);
        if (e == hipSuccess && pl.want_f && !accumulate && a->n_inp > 0)
            e = hipMemsetAsync(b->grad_inp_features, 0, sizeof(float) * (size_t)a->n_inp * pl.cin, stream);
        if (e != hipSuccess) { g_last_hip_error = (int)e; return DMCF_ELAUNCH; }
        return DMCF_OK;
    }
    CconvParams p;
    BwdGeo geo;
    bwd_params(a, pl, p, geo);
    float* psi = nullptr;
    if (a->flags & DMCF_FLAG_NORMALIZE) {
        psi = (float*)(w + pl.off_psi);
        const dim3 grid((unsigned)((a->n_out + 1) / 2));
        if (out_ext)
            hipLaunchKernelGGL(cconv_bwd_norm_ext, grid, dim3(64), 0, stream, p, out_ext, psi);
        else
            hipLaunchKernelGGL(cconv_bwd_norm, grid, dim3(64), 0, stream, p, psi);
    }
    if (pl.want_f) {
        const float* Wfull = a->filters;
        if (pl.sym) {
            float* wf = (float*)(w + pl.off_wfull);
            hipLaunchKernelGGL(cconv_bwd_expand, dim3(grid_for(n_full, 256)), dim3(256), 0, stream, a->filters, wf, pl.dz, pl.dy,
                               pl.dx, pl.cin, pl.cout, a->sym_axis);
            Wfull = wf;
        }
        hipError_t e = hipFuncSetAttribute(out_ext ? (const void*)cconv_bwd_input_ext : (const void*)cconv_bwd_input,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds_input);
        if (e != hipSuccess) { g_last_hip_error = (int)e; return DMCF_ELAUNCH; }
        if (out_ext)
            hipLaunchKernelGGL(cconv_bwd_input_ext, dim3((unsigned)a->n_inp), dim3(64), pl.lds_input, stream, p, geo, out_ext, Wfull,
                               b->grad_out, (const float*)psi, b->inv_index, b->inv_pair, b->inv_row_splits, b->inv_n_pairs,
                               pl.sym ? 1 : 0, b->grad_inp_features, accumulate);
        else
            hipLaunchKernelGGL(cconv_bwd_input, dim3((unsigned)a->n_inp), dim3(64), pl.lds_input, stream, p, geo, Wfull, b->grad_out,
                               (const float*)psi, b->inv_index, b->inv_pair, b->inv_row_splits, b->inv_n_pairs, pl.sym ? 1 : 0,
                               b->grad_inp_features, accumulate);
        rc = check_launch();
        if (rc != DMCF_OK) return rc;
    }
    if (pl.want_w) {
        hipError_t e = hipFuncSetAttribute(out_ext ? (const void*)cconv_bwd_filter_splat_ext : (const void*)cconv_bwd_filter_splat,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds_splat);
        if (e != hipSuccess) { g_last_hip_error = (int)e; return DMCF_ELAUNCH; }
        float* Bc = (float*)(w + pl.off_b);
        float* slabs = (float*)(w + pl.off_slabs);
        float* dfull = (float*)(w + pl.off_dfull);
        int first = 1;
        for (int64_t row0 = 0; row0 < a->n_out; row0 += pl.R) {
            const int64_t rows = min(pl.R, a->n_out - row0);
            const int64_t rps = (rows + pl.S - 1) / pl.S;
            const int S = (int)((rows + rps - 1) / rps);
            if (out_ext)
                hipLaunchKernelGGL(cconv_bwd_filter_splat_ext, dim3((unsigned)rows), dim3(64), pl.lds_splat, stream, p, geo, out_ext,
                                   (const float*)psi, pl.sym ? 1 : 0, row0, Bc);
            else
                hipLaunchKernelGGL(cconv_bwd_filter_splat, dim3((unsigned)rows), dim3(64), pl.lds_splat, stream, p, geo,
                                   (const float*)psi, pl.sym ? 1 : 0, row0, Bc);
            hipLaunchKernelGGL(cconv_bwd_filter_gemm, dim3((unsigned)((pl.M + 63) / 64), (unsigned)((pl.cout + 63) / 64), (unsigned)S),
                               dim3(256), 0, stream, (const float*)Bc, b->grad_out + row0 * pl.cout, rows, pl.M, pl.cout, rps, slabs);
            hipLaunchKernelGGL(cconv_bwd_filter_reduce, dim3(grid_for(n_full, 256)), dim3(256), 0, stream, (const float*)slabs, S, n_full,
                               dfull, first);
            first = 0;
            rc = check_launch();
            if (rc != DMCF_OK) return rc;
        }
        hipLaunchKernelGGL(cconv_bwd_filter_store, dim3(grid_for(n_stored, 256)), dim3(256), 0, stream, (const float*)dfull,
                           b->grad_filters, pl.dz, pl.dy, pl.dx, pl.cin, pl.cout, pl.sym ? 1 : 0, a->sym_axis, accumulate);
    }
    return check_launch();
}

// the kernels bwd_run launches, in launch order, separated by ';' (ext: the names of the individual-extent call)
static int bwd_names(const dmcf_cconv_args* a, const BwdPlan& pl, bool ext, char* names, size_t name_bytes) {
    if (!names || name_bytes < 2) return DMCF_EINVAL;
    char buf[256];
    buf[0] = 0;
    auto add = [&](const char* s) {
        if (buf[0]) strncat(buf, ";", sizeof(buf) - strlen(buf) - 1);
        strncat(buf, s, sizeof(buf) - strlen(buf) - 1);
    };
    if (a->flags & DMCF_FLAG_NORMALIZE) add(ext ? "cconv_bwd_norm_ext" : "cconv_bwd_norm");
    if (pl.want_f) {
        if (pl.sym) add("cconv_bwd_expand");
        add(ext ? "cconv_bwd_input_ext" : "cconv_bwd_input");
    }
    if (pl.want_w) {
        add(ext ? "cconv_bwd_filter_splat_ext" : "cconv_bwd_filter_splat");
        add("cconv_bwd_filter_gemm");
        add("cconv_bwd_filter_reduce");
        add("cconv_bwd_filter_store");
    }
    if (strlen(buf) + 1 > name_bytes) return DMCF_EINVAL;
    memcpy(names, buf, strlen(buf) + 1);
    return DMCF_OK;
}

// bwd_plan of the individual-extent call: args->extent is ignored (planned with 1), and SKIP_SELF is refused as in
// dmcf_cconv_forward_extents
static int bwd_plan_extents(const dmcf_cconv_args* a, const dmcf_cconv_backward_args* b, BwdPlan& pl) {
    if (!a) return DMCF_EINVAL;
    dmcf_cconv_args a1 = *a;
    a1.extent = 1.0f;
    const int rc = bwd_plan(&a1, b, pl);
    if (rc != DMCF_OK) return rc;
    if (a->flags & DMCF_FLAG_SKIP_SELF) return DMCF_EUNSUPPORTED;
    return DMCF_OK;
}

}  // namespace dmcf

using namespace dmcf;

extern "C" {

size_t dmcf_invert_neighbors_list_workspace_bytes(int64_t n_pairs) {
    if (n_pairs < 0) return 256;
    const size_t n = (size_t)(n_pairs > 0 ? n_pairs : 1);
    return 4 * align_up(n * 4, 256) + align_up(invert_sort_tmp(n_pairs > 0 ? n_pairs : 1), 256) + 256;
}

int dmcf_invert_neighbors_list(int64_t n_inp, const int32_t* neighbors_index, const int64_t* neighbors_row_splits,
                               const int32_t* neighbors_row_count, int64_t n_out, int64_t n_pairs, const float* values,
                               int32_t* inv_index, int64_t* inv_row_splits, int32_t* inv_pair, float* inv_values,
                               void* workspace, size_t workspace_bytes, dmcf_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n_inp < 0 || n_out < 0 || n_pairs < 0 || !inv_row_splits) return DMCF_EINVAL;
    if (n_out > 0 && !neighbors_row_splits) return DMCF_EINVAL;
    if (n_pairs > 0 && (!neighbors_index || !inv_index)) return DMCF_EINVAL;
    if (inv_values && n_pairs > 0 && !values) return DMCF_EINVAL;
    if (n_pairs > 0x7fffffffLL || n_inp >= 0x7fffffffLL || n_out > 0x7fffffffLL) return DMCF_EUNSUPPORTED;
    if (workspace_bytes < dmcf_invert_neighbors_list_workspace_bytes(n_pairs)) return DMCF_EWORKSPACE;
    if (!workspace || ((uintptr_t)workspace & 255)) return DMCF_EINVAL;
    if (n_pairs == 0) {
        const hipError_t e = hipMemsetAsync(inv_row_splits, 0, sizeof(int64_t) * (size_t)(n_inp + 1), stream);
        if (e != hipSuccess) { g_last_hip_error = (int)e; return DMCF_ELAUNCH; }
        return DMCF_OK;
    }
    const size_t seg = align_up((size_t)n_pairs * 4, 256);
    char* w = (char*)workspace;
    uint32_t* keys = (uint32_t*)w;
    uint32_t* skeys = (uint32_t*)(w + seg);
    int32_t* vals = (int32_t*)(w + 2 * seg);
    int32_t* row_of = (int32_t*)(w + 3 * seg);
    void* tmp = w + 4 * seg;
    size_t tmp_bytes = workspace_bytes - 4 * seg - 256;
    int32_t* perm = inv_pair;
    if (!perm) return DMCF_EINVAL;  // (the permutation is written there)
    hipLaunchKernelGGL(invert_init, dim3(grid_for(n_pairs, 256)), dim3(256), 0, stream, keys, vals, n_pairs, (uint32_t)n_inp);
    if (n_out > 0)
        hipLaunchKernelGGL(invert_keys, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, stream, neighbors_index,
                           neighbors_row_splits, neighbors_row_count, n_out, n_inp, n_pairs, keys, row_of);
    int rc = check_launch();
    if (rc != DMCF_OK) return rc;
    unsigned end_bit = 1;
    while (end_bit < 32 && ((uint64_t)1 << end_bit) <= (uint64_t)n_inp) ++end_bit;
    hipError_t e = rocprim::radix_sort_pairs(tmp, tmp_bytes, (const uint32_t*)keys, skeys, (const int32_t*)vals, perm,
                                             (size_t)n_pairs, 0u, end_bit, stream);
    if (e != hipSuccess) { g_last_hip_error = (int)e; return DMCF_ELAUNCH; }
    hipLaunchKernelGGL(invert_splits, dim3((unsigned)((n_inp + 1 + 255) / 256)), dim3(256), 0, stream, (const uint32_t*)skeys,
                       n_pairs, n_inp, inv_row_splits);
    hipLaunchKernelGGL(invert_gather, dim3(grid_for(n_pairs, 256)), dim3(256), 0, stream, (const uint32_t*)skeys, (const int32_t*)perm,
                       (const int32_t*)row_of, values, n_pairs, n_inp, inv_index, inv_pair, inv_values);
    return check_launch();
}

size_t dmcf_cconv_backward_workspace_bytes(const dmcf_cconv_args* fwd, const dmcf_cconv_backward_args* bwd) {
    BwdPlan pl;
    if (bwd_plan(fwd, bwd, pl) != DMCF_OK) return 256;
    return pl.total;
}

int dmcf_cconv_backward(const dmcf_cconv_args* a, const dmcf_cconv_backward_args* b, void* workspace, size_t workspace_bytes,
                        dmcf_stream_t stream) {
    BwdPlan pl;
    const int rc = bwd_plan(a, b, pl);
    if (rc != DMCF_OK) return rc;
    return bwd_run(a, b, pl, nullptr, workspace, workspace_bytes, (hipStream_t)stream);
}

int dmcf_cconv_backward_extents(const dmcf_cconv_args* a, const dmcf_cconv_backward_args* b, const float* out_extents,
                                void* workspace, size_t workspace_bytes, dmcf_stream_t stream) {
    BwdPlan pl;
    const int rc = bwd_plan_extents(a, b, pl);
    if (rc != DMCF_OK) return rc;
    if (a->n_out > 0 && !out_extents) return DMCF_EINVAL;
    return bwd_run(a, b, pl, out_extents, workspace, workspace_bytes, (hipStream_t)stream);
}

int dmcf_cconv_backward_kernel_names(const dmcf_cconv_args* a, const dmcf_cconv_backward_args* b, char* names, size_t name_bytes) {
    if (!names || name_bytes < 2) return DMCF_EINVAL;
    BwdPlan pl;
    const int rc = bwd_plan(a, b, pl);
    if (rc != DMCF_OK) return rc;
    return bwd_names(a, pl, false, names, name_bytes);
}

int dmcf_cconv_backward_extents_kernel_names(const dmcf_cconv_args* a, const dmcf_cconv_backward_args* b, char* names,
                                             size_t name_bytes) {
    if (!names || name_bytes < 2) return DMCF_EINVAL;
    BwdPlan pl;
    const int rc = bwd_plan_extents(a, b, pl);
    if (rc != DMCF_OK) return rc;
    return bwd_names(a, pl, true, names, name_bytes);
}

}  // extern "C"
