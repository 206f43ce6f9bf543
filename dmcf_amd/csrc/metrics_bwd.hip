// Gradients of the point-cloud ops (ABI 2.13): nn_distance (utils/tools/nn_distance.cu:158-183, NmDistanceGradKernel),
// match_cost (tf_approxmatch.cu:346-430, matchcostgrad1 / matchcostgrad2), the match-free gradient of the fused EMD
// (match_cost(approx_match(...)) with the match held constant: NoGradient('ApproxMatch')) and gather_point
// (sampling.cu, GatherPointGrad).
//
// No float atomics (the reference scatters with atomicAdd).  Scattered terms are gathered instead: the index list is
// inverted by a stable radix sort of (batch * targets + target) keys over the sources in ascending order, so each target
// sums its sources in ascending source order (a target with more than kInvShort of them: one workgroup in a fixed order).
// The all-pairs gradients have the shape of metrics.hip: 256 rows per
// workgroup, one per lane, the other set streamed through LDS in tiles, column splits writing per-split partials that a
// second launch sums in split order, and a plan that depends on the sizes only.  Two identical calls give identical bits.
//
// EMD: the match of the forward is w_kl = sum over the ten levels j of (e^(level_j d2_kl) ratioR_j[l]) ratioL_j[k], with
// ratioL_j / ratioR_j recorded by dmcf_emd_with_levels.  Each term is formed with the float32 expression and operand order of
// the forward's pass C (am_pass_kernel<kMtFused>), and the terms are summed in level order from 0, as the dense match
// accumulates them, so w_kl has the bits of match[l, k] of dmcf_approx_match.  Then
//   grad_xyz1[k] = g sum_l w_kl (x1_k - x2_l) rsqrt(max(d2, 1e-20)),   grad_xyz2[l] = g sum_k w_kl (x2_l - x1_k) rsqrt(...).
// Both sweeps form d2 from (row - column) differences; negation is exact, so d2 has the forward's bits in either sweep.
#include <math.h>

#include <vector>

#include <rocprim/device/device_radix_sort.hpp>

#include "common.h"
#include "metrics_plan.h"

namespace dmcf {

// ------------------------------------------------------------------------------------------------------------------
// inversion of an index list: sources s in [0, S), S / per_seg segments (batch items) of per_seg sources each; source s of
// segment b points at target idx[s] in [0, T).  Sorted by key b * T + idx[s] (stable: ascending s within a key); indices
// outside [0, T) get the key b_total * T and are never gathered.  splits[t] = first sorted entry of global target t.
// ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void inv_keys_kernel(const int32_t* __restrict__ idx, int64_t S, int64_t per_seg, int64_t T,
                                                       uint32_t* __restrict__ keys, int32_t* __restrict__ vals) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= S) return;
    const int64_t b = s / per_seg;
    const int32_t t = idx[s];
    keys[s] = (t >= 0 && t < T) ? (uint32_t)(b * T + t) : (uint32_t)(S / per_seg * T);
    vals[s] = (int32_t)s;
}

__global__ __launch_bounds__(256) void inv_splits_kernel(const uint32_t* __restrict__ skeys, int64_t S, int64_t NT,
                                                         int32_t* __restrict__ splits) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t > NT) return;
    int64_t lo = 0, hi = S;  // first entry with key >= t
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)skeys[mid] < t) lo = mid + 1;
        else hi = mid;
    }
    splits[t] = (int32_t)lo;
}

struct InvWork {
    uint32_t *keys, *skeys;
    int32_t *vals, *svals, *splits;
    void* tmp;
    size_t tmp_bytes;
};

inline size_t inv_sort_tmp(int64_t S) {
    size_t bytes = 0;
    (void)rocprim::radix_sort_pairs((void*)nullptr, bytes, (const uint32_t*)nullptr, (uint32_t*)nullptr, (const int32_t*)nullptr,
                                    (int32_t*)nullptr, (size_t)S, 0u, 32u, (hipStream_t)0);
    return bytes;
}

// workspace of one inversion of S sources onto NT targets, carved from base (NULL: size only)
inline size_t inv_carve(int64_t S, int64_t NT, char* base, InvWork* w) {
    const size_t a = align_up((size_t)(S > 0 ? S : 1) * 4, 256), sp = align_up((size_t)(NT + 1) * 4, 256);
    const size_t tb = align_up(inv_sort_tmp(S > 0 ? S : 1), 256);
    if (base != nullptr) {
        w->keys = (uint32_t*)base;
        w->vals = (int32_t*)(base + a);
        w->skeys = (uint32_t*)(base + 2 * a);
        w->svals = (int32_t*)(base + 3 * a);
        w->splits = (int32_t*)(base + 4 * a);
        w->tmp = base + 4 * a + sp;
        w->tmp_bytes = tb;
    }
    return 4 * a + sp + tb;
}

int invert_index(const int32_t* idx, int64_t S, int64_t per_seg, int64_t T, const InvWork& w, hipStream_t st) {
    const int64_t NT = S / per_seg * T;
    inv_keys_kernel<<<(unsigned)((S + 255) / 256), 256, 0, st>>>(idx, S, per_seg, T, w.keys, w.vals);
    int rc = check_launch();
    if (rc != DMCF_OK) return rc;
    unsigned end_bit = 1;
    while (end_bit < 32 && ((uint64_t)1 << end_bit) <= (uint64_t)NT) ++end_bit;
    size_t tb = w.tmp_bytes;
    const hipError_t e = rocprim::radix_sort_pairs(w.tmp, tb, (const uint32_t*)w.keys, w.skeys, (const int32_t*)w.vals, w.svals,
                                                   (size_t)S, 0u, end_bit, st);
    if (e != hipSuccess) {
        g_last_hip_error = (int)e;
        return DMCF_ELAUNCH;
    }
    inv_splits_kernel<<<(unsigned)((NT + 1 + 255) / 256), 256, 0, st>>>(w.skeys, S, NT, w.splits);
    return check_launch();
}

// ------------------------------------------------------------------------------------------------------------------
// Gathering the inverted sources.  A target with at most kInvShort sources sums them in one thread, in ascending source
// order.  A longer one (all points of a collapsed or distant cloud share one nearest point) is summed by one 256-thread
// workgroup: lane j takes the entries j, j + 256, ... in order, then a fixed LDS tree adds the lanes.  The workgroup that owns
// a long target is the one whose chunk of kInvShort sorted entries starts first inside the target's entries, so each long
// target has exactly one owner and the grid depends on the number of sources only.  Either way the order of the sums
// depends on the segment's length alone: two identical calls give identical bits.
// ------------------------------------------------------------------------------------------------------------------
constexpr int kInvShort = 256;

// the target whose long segment workgroup blockIdx.x owns (-1: none), and that segment
__device__ __forceinline__ int64_t inv_long_owner(const uint32_t* __restrict__ skeys, const int32_t* __restrict__ splits, int64_t S,
                                                  int64_t NT, int32_t* lo, int32_t* hi) {
    const int64_t p = (int64_t)blockIdx.x * kInvShort;
    if (p >= S) return -1;
    const int64_t t = skeys[p];
    if (t >= NT) return -1;  // (the entries of out-of-range indices sort last)
    *lo = splits[t];
    *hi = splits[t + 1];
    // p lies in [lo, hi); the owner is the first chunk start at or after lo
    return (*hi - *lo > kInvShort && p - kInvShort < (int64_t)*lo) ? t : -1;
}

// deterministic workgroup sum of one value per lane (256 lanes, fixed tree); the result is valid in lane 0
__device__ __forceinline__ float block_sum256(float v, float* red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    const float r = red[0];
    __syncthreads();
    return r;
}

// ------------------------------------------------------------------------------------------------------------------
// nn_distance: per point i of the query set q (batch b): the direct term of its own distance, g = 2 gq[i],
// g (q_i - o_{idxq[i]}), then minus g' (o_s - q_i), g' = 2 go[s], for every point s of the other set o whose nearest point is
// i (the inversion of idxo): in ascending source order here when there are at most kInvShort of them, else added by
// nn_grad_long_kernel.  gq / go NULL: that term is absent.
// ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void nn_grad_kernel(const float* __restrict__ q, int64_t nq, const float* __restrict__ o,
                                                      int64_t no, int64_t total, const float* __restrict__ gq,
                                                      const int32_t* __restrict__ idxq, const float* __restrict__ go,
                                                      const int32_t* __restrict__ splits, const int32_t* __restrict__ svals,
                                                      float* __restrict__ grad) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int64_t b = i / nq;
    const float x = q[3 * i], y = q[3 * i + 1], z = q[3 * i + 2];
    float ax = 0.0f, ay = 0.0f, az = 0.0f;
    if (gq != nullptr) {
        const int32_t p = idxq[i];
        if (p >= 0 && p < no) {
            const float g = gq[i] * 2.0f;
            const float* op = o + (b * no + p) * 3;
            ax = g * (x - op[0]);
            ay = g * (y - op[1]);
            az = g * (z - op[2]);
        }
    }
    if (go != nullptr && splits[i + 1] - splits[i] <= kInvShort) {
        for (int32_t e = splits[i], e1 = splits[i + 1]; e < e1; ++e) {
            const int64_t s = svals[e];
            const float g = go[s] * 2.0f;
            ax -= g * (o[3 * s] - x);
            ay -= g * (o[3 * s + 1] - y);
            az -= g * (o[3 * s + 2] - z);
        }
    }
    grad[3 * i] = ax;
    grad[3 * i + 1] = ay;
    grad[3 * i + 2] = az;
}

// the scattered terms of the points with more than kInvShort sources, after nn_grad_kernel (one workgroup per chunk of
// kInvShort sorted entries; grid ceil(S / kInvShort))
__global__ __launch_bounds__(256) void nn_grad_long_kernel(const float* __restrict__ q, const float* __restrict__ o, int64_t S,
                                                           int64_t NT, const float* __restrict__ go, const uint32_t* __restrict__ skeys,
                                                           const int32_t* __restrict__ splits, const int32_t* __restrict__ svals,
                                                           float* __restrict__ grad) {
    __shared__ float red[256];
    int32_t lo = 0, hi = 0;
    const int64_t i = inv_long_owner(skeys, splits, S, NT, &lo, &hi);
    if (i < 0) return;  // (uniform across the workgroup)
    const float x = q[3 * i], y = q[3 * i + 1], z = q[3 * i + 2];
    float ax = 0.0f, ay = 0.0f, az = 0.0f;
    for (int64_t e = lo + (int64_t)threadIdx.x; e < hi; e += 256) {
        const int64_t s = svals[e];
        const float g = go[s] * 2.0f;
        ax += g * (o[3 * s] - x);
        ay += g * (o[3 * s + 1] - y);
        az += g * (o[3 * s + 2] - z);
    }
    ax = block_sum256(ax, red);
    ay = block_sum256(ay, red);
    az = block_sum256(az, red);
    if (threadIdx.x == 0) {
        grad[3 * i] -= ax;
        grad[3 * i + 1] -= ay;
        grad[3 * i + 2] -= az;
    }
}

// gather_point: grad_inp[t, c] = sum over the sources s with index[s] == t, in ascending s, of grad_out[s, c]; targets with
// more than kInvShort sources are left to gather_grad_long_kernel
__global__ __launch_bounds__(256) void gather_grad_kernel(const float* __restrict__ grad_out, int64_t n_inp, int channels,
                                                          const int32_t* __restrict__ splits, const int32_t* __restrict__ svals,
                                                          float* __restrict__ grad_inp) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= n_inp * channels) return;
    const int64_t t = q / channels, c = q - t * channels;
    float s = 0.0f;
    if (splits[t + 1] - splits[t] <= kInvShort)
        for (int32_t e = splits[t], e1 = splits[t + 1]; e < e1; ++e) s += grad_out[(int64_t)svals[e] * channels + c];
    grad_inp[q] = s;
}

__global__ __launch_bounds__(256) void gather_grad_long_kernel(const float* __restrict__ grad_out, int64_t S, int64_t n_inp, int channels,
                                                               const uint32_t* __restrict__ skeys, const int32_t* __restrict__ splits,
                                                               const int32_t* __restrict__ svals, float* __restrict__ grad_inp) {
    __shared__ float red[256];
    int32_t lo = 0, hi = 0;
    const int64_t t = inv_long_owner(skeys, splits, S, n_inp, &lo, &hi);
    if (t < 0) return;
    for (int c = 0; c < channels; ++c) {
        float s = 0.0f;
        for (int64_t e = lo + (int64_t)threadIdx.x; e < hi; e += 256) s += grad_out[(int64_t)svals[e] * channels + c];
        s = block_sum256(s, red);
        if (threadIdx.x == 0) grad_inp[t * channels + c] = s;
    }
}

// ------------------------------------------------------------------------------------------------------------------
// match_cost, dense match [b, m, n]: rows of xyz1 read match[l, row] (consecutive across lanes); rows of xyz2 read
// match[row, k], strided across lanes, so a 256-row x 32-column block is staged transposed through LDS first.
// Partials part[((s * nb + b) * 3 + c) * nrow + row]; the combine launch multiplies the split sum by grad_cost[b].
// ------------------------------------------------------------------------------------------------------------------
constexpr int kMcSub = 32;  // columns per transposed match block (rows of xyz2)

template <bool ROWS1>
__global__ __launch_bounds__(kMtThreads) void mc_grad_kernel(const float* __restrict__ rp, int64_t nrow, const float* __restrict__ cp,
                                                             int64_t ncol, int64_t chunk, const float* __restrict__ match,
                                                             float* __restrict__ part) {
    constexpr int kSub = ROWS1 ? kMtTile : kMcSub;
    __shared__ float4 tile[kSub];
    __shared__ float mt[ROWS1 ? 1 : kMcSub][kMtThreads + 1];
    const int64_t b = blockIdx.z, s = blockIdx.y, nb = gridDim.z;
    const int64_t row0 = (int64_t)blockIdx.x * kMtThreads, row = row0 + threadIdx.x;
    const bool live = row < nrow;
    rp += b * nrow * 3;
    cp += b * ncol * 3;
    match += b * nrow * ncol;  // [m, n] of this item
    float x = 0.0f, y = 0.0f, z = 0.0f;
    if (live) {
        x = rp[3 * row];
        y = rp[3 * row + 1];
        z = rp[3 * row + 2];
    }
    const int64_t c0 = s * chunk, c1 = c0 + chunk < ncol ? c0 + chunk : ncol;
    float ax = 0.0f, ay = 0.0f, az = 0.0f;
    for (int64_t t0 = c0; t0 < c1; t0 += kSub) {
        const int cnt = (int)(c1 - t0 < kSub ? c1 - t0 : kSub);
        __syncthreads();
        if ((int)threadIdx.x < cnt) {
            const int64_t c = t0 + threadIdx.x;
            tile[threadIdx.x] = make_float4(cp[3 * c], cp[3 * c + 1], cp[3 * c + 2], 0.0f);
        }
        if (!ROWS1) {  // match[row0 + r, t0 + j] -> mt[j][r]: each wave reads two 128-byte row pieces per step
#pragma unroll 4
            for (int e = threadIdx.x; e < kMcSub * kMtThreads; e += kMtThreads) {
                const int r = e / kMcSub, j = e % kMcSub;
                mt[j][r] = (row0 + r < nrow && j < cnt) ? match[(row0 + r) * ncol + t0 + j] : 0.0f;
            }
        }
        __syncthreads();
#pragma unroll 4
        for (int j = 0; j < cnt; ++j) {
            const float4 p = tile[j];
            const float dx = x - p.x, dy = y - p.y, dz = z - p.z;
            const float d2 = fmaf(dx, dx, fmaf(dy, dy, dz * dz));
            float mv;
            if (ROWS1) mv = live ? match[(t0 + j) * nrow + row] : 0.0f;
            else mv = mt[j][threadIdx.x];
            const float cf = mv * rsqrtf(fmaxf(d2, 1e-20f));
            ax = fmaf(cf, dx, ax);
            ay = fmaf(cf, dy, ay);
            az = fmaf(cf, dz, az);
        }
    }
    if (live) {
        float* pp = part + (s * nb + b) * 3 * nrow + row;
        pp[0] = ax;
        pp[nrow] = ay;
        pp[2 * nrow] = az;
    }
}

// ------------------------------------------------------------------------------------------------------------------
// EMD, match-free: one batch item, rows of one set against the other; the ten ratios of every column sit in LDS next to its
// coordinates, the row's ten in registers.  ROWS1: rows are xyz1 (their ratios ratioL), columns xyz2 (ratioR).
// ------------------------------------------------------------------------------------------------------------------
struct AmLevels {
    float v[kAmLevels];
};

struct alignas(16) EmdCol {
    float x, y, z, pad;
    float r[kAmLevels];
    float pad2[2];
};

// the tile walk of both EMD gradient kernels: the columns [c0, c1) of cp in ascending order, in LDS tiles of kMtTile, against
// the row at rp[3 * row] (live: the lane has one) -> the three sums of the chunk.  rrat / crat: the ten ratios of row r at
// rrat[L * lvl_ld + r], of column c at crat[L * lvl_ld + c].  Every lane of the workgroup calls it (it synchronises).
template <bool ROWS1>
__device__ __forceinline__ void emd_grad_walk(EmdCol* __restrict__ tile, const float* __restrict__ rp, int64_t row, bool live,
                                              const float* __restrict__ cp, int64_t c0, int64_t c1, const AmLevels& lv,
                                              const float* __restrict__ rrat, const float* __restrict__ crat, int64_t lvl_ld,
                                              float& ax, float& ay, float& az) {
    float x = 0.0f, y = 0.0f, z = 0.0f, rr[kAmLevels];
#pragma unroll
    for (int L = 0; L < kAmLevels; ++L) rr[L] = 0.0f;
    if (live) {
        x = rp[3 * row];
        y = rp[3 * row + 1];
        z = rp[3 * row + 2];
#pragma unroll
        for (int L = 0; L < kAmLevels; ++L) rr[L] = rrat[L * lvl_ld + row];
    }
    ax = ay = az = 0.0f;
    for (int64_t t0 = c0; t0 < c1; t0 += kMtTile) {
        const int cnt = (int)(c1 - t0 < kMtTile ? c1 - t0 : kMtTile);
        __syncthreads();
        if ((int)threadIdx.x < cnt) {
            const int64_t c = t0 + threadIdx.x;
            EmdCol& e = tile[threadIdx.x];
            e.x = cp[3 * c];
            e.y = cp[3 * c + 1];
            e.z = cp[3 * c + 2];
#pragma unroll
            for (int L = 0; L < kAmLevels; ++L) e.r[L] = crat[L * lvl_ld + c];
        }
        __syncthreads();
#pragma unroll 2
        for (int j = 0; j < cnt; ++j) {
            const EmdCol& p = tile[j];
            const float dx = x - p.x, dy = y - p.y, dz = z - p.z;
            const float d2 = fmaf(dx, dx, fmaf(dy, dy, dz * dz));
            float w = 0.0f;
#pragma unroll
            for (int L = 0; L < kAmLevels; ++L) {
                // pass C: e = __expf(level d2) ratioR[l]; w = e ratioL[k]
                const float e = __expf(lv.v[L] * d2) * (ROWS1 ? p.r[L] : rr[L]);
                w += e * (ROWS1 ? rr[L] : p.r[L]);
            }
            const float cf = w * rsqrtf(fmaxf(d2, 1e-20f));
            ax = fmaf(cf, dx, ax);
            ay = fmaf(cf, dy, ay);
            az = fmaf(cf, dz, az);
        }
    }
}

template <bool ROWS1>
__global__ __launch_bounds__(kMtThreads) void emd_grad_kernel(const float* __restrict__ rp, int64_t nrow, const float* __restrict__ cp,
                                                              int64_t ncol, int64_t chunk, AmLevels lv, const float* __restrict__ rrat,
                                                              const float* __restrict__ crat, int64_t lvl_ld,
                                                              float* __restrict__ part) {
    __shared__ EmdCol tile[kMtTile];
    const int64_t s = blockIdx.y;
    const int64_t row = (int64_t)blockIdx.x * kMtThreads + threadIdx.x;
    const bool live = row < nrow;
    const int64_t c0 = s * chunk, c1 = c0 + chunk < ncol ? c0 + chunk : ncol;
    float ax, ay, az;
    emd_grad_walk<ROWS1>(tile, rp, row, live, cp, c0, c1, lv, rrat, crat, lvl_ld, ax, ay, az);
    if (live) {
        float* pp = part + s * 3 * nrow + row;
        pp[0] = ax;
        pp[nrow] = ay;
        pp[2 * nrow] = az;
    }
}

// the sum of a row's partials of one coordinate, p[j * step] for j < nsplit in split order (both combine kernels)
__device__ __forceinline__ float grad_split_sum(const float* __restrict__ p, int64_t step, int64_t nsplit) {
    float s = 0.0f;
    for (int64_t j = 0; j < nsplit; ++j) s += p[j * step];
    return s;
}

// grad[(b * nout + row) * 3 + c] = grad_cost[b] * sum_s part[((s * nb + b) * 3 + c) * nrow + row] for row < nrow, 0 up to nout
__global__ __launch_bounds__(kMtThreads) void grad_combine_kernel(const float* __restrict__ part, int64_t nrow, int64_t nout,
                                                                  int64_t nb, int64_t nsplit, const float* __restrict__ grad_cost,
                                                                  float* __restrict__ grad) {
    const int64_t i = (int64_t)blockIdx.x * kMtThreads + threadIdx.x;
    if (i >= nb * nout) return;
    const int64_t b = i / nout, row = i - b * nout;
    float a[3] = {0.0f, 0.0f, 0.0f};
    if (row < nrow) {
        const float g = grad_cost[b];
        for (int c = 0; c < 3; ++c) a[c] = g * grad_split_sum(part + (b * 3 + c) * nrow + row, nb * 3 * nrow, nsplit);
    }
    grad[3 * i] = a[0];
    grad[3 * i + 1] = a[1];
    grad[3 * i + 2] = a[2];
}

// ------------------------------------------------------------------------------------------------------------------
// EMD over a ragged batch (ABI 2.25): the gradient launch and the combine launch of dmcf_emd_backward, each ONE launch over the
// tiles / row blocks of ALL items.  An item keeps the column chunks of its own mt_plan(rows, cols), the walk is emd_grad_walk
// and the combine sums in split order before g * s, so an item's rows have dmcf_emd_backward's bits for the item alone.  The
// host writes the tables from the row splits it has validated: no kernel reads row splits and every index lies inside its array
// by construction.  Points and levels run over the concatenated rows (levels [kAmLevels, n_total + m_total], ratioR from
// column n_total on); an item's partials are [nsplit, 3, rows of the item] at its own base.
// ------------------------------------------------------------------------------------------------------------------
struct EgTile {          // one workgroup of the gradient launch
    int32_t row0, rows;  // rows [row0, row0 + rows) of the concatenated row set, 1 <= rows <= kMtThreads
    int32_t c0, c1;      // the chunk [c0, c1) of the concatenated column set, c0 < c1
    int64_t pbase;       // part[pbase + c * stride + lane]: coordinate c of (this chunk, row0 + lane)
    int32_t stride, pad; // the item's rows
};
static_assert(sizeof(EgTile) == 32, "EgTile is packed");

struct EgRows {             // one workgroup of the combine launch
    int32_t row0, rows;     // as above
    int32_t item, nsplit;   // grad_cost[item]; nsplit == 0: an item without pairs, its rows get zeros
    int64_t pbase;          // part[pbase + (j * 3 + c) * stride + lane], j < nsplit in split order
    int32_t stride, pad;
};
static_assert(sizeof(EgRows) == 32, "EgRows is packed");

template <bool ROWS1>
__global__ __launch_bounds__(kMtThreads) void emd_ragged_grad_kernel(const float* __restrict__ rp, const float* __restrict__ cp,
                                                                     const EgTile* __restrict__ tiles, AmLevels lv,
                                                                     const float* __restrict__ rrat, const float* __restrict__ crat,
                                                                     int64_t lvl_ld, float* __restrict__ part) {
    __shared__ EmdCol tile[kMtTile];
    const EgTile t = tiles[blockIdx.x];
    const int lane = (int)threadIdx.x;
    const bool live = lane < t.rows;
    float ax, ay, az;
    emd_grad_walk<ROWS1>(tile, rp, (int64_t)t.row0 + lane, live, cp, t.c0, t.c1, lv, rrat, crat, lvl_ld, ax, ay, az);
    if (live) {
        float* pp = part + t.pbase + lane;
        pp[0] = ax;
        pp[t.stride] = ay;
        pp[2 * (int64_t)t.stride] = az;
    }
}

__global__ __launch_bounds__(kMtThreads) void emd_ragged_combine_kernel(const EgRows* __restrict__ recs, const float* __restrict__ part,
                                                                        const float* __restrict__ grad_cost, float* __restrict__ grad) {
    const EgRows r = recs[blockIdx.x];
    if ((int)threadIdx.x >= r.rows) return;
    const int64_t row = (int64_t)r.row0 + threadIdx.x;
    float a[3] = {0.0f, 0.0f, 0.0f};
    if (r.nsplit > 0) {
        const float g = grad_cost[r.item];
        for (int c = 0; c < 3; ++c)
            a[c] = g * grad_split_sum(part + r.pbase + (int64_t)c * r.stride + threadIdx.x, 3 * (int64_t)r.stride, r.nsplit);
    }
    grad[3 * row] = a[0];
    grad[3 * row + 1] = a[1];
    grad[3 * row + 2] = a[2];
}

// what the validated splits ask of dmcf_emd_ragged_backward, per side (0: rows of xyz1, 1: rows of xyz2)
struct EgSizes {
    int64_t tiles[2] = {0, 0};  // gradient tiles: sum of row_blocks * nsplit over the items with pairs
    int64_t recs[2] = {0, 0};   // combine records: the row blocks of every item, with pairs or not
    int64_t part[2] = {0, 0};   // floats of partials: sum of nsplit * 3 * rows over the items with pairs
};

inline EgSizes eg_sizes(const int64_t* rs1, const int64_t* rs2, int64_t batch) {
    EgSizes z;
    for (int64_t b = 0; b < batch; ++b) {
        const int64_t n = rs1[b + 1] - rs1[b], m = rs2[b + 1] - rs2[b];
        for (int side = 0; side < 2; ++side) {
            const int64_t rows = side == 0 ? n : m, cols = side == 0 ? m : n;
            const int64_t blocks = (rows + kMtThreads - 1) / kMtThreads;
            z.recs[side] += blocks;
            if (rows == 0 || cols == 0) continue;
            const MtPlan p = mt_plan(rows, cols);
            z.tiles[side] += blocks * p.nsplit;
            z.part[side] += p.nsplit * 3 * rows;
        }
    }
    return z;
}

// the workspace: the four tables (tiles of side 0, of side 1, records of side 0, of side 1; one copy from the host's block of the
// same layout), then the partials, which the two sides use one after the other
struct EgTables {
    EgTile* t[2];
    EgRows* r[2];
};

inline size_t eg_tables(const EgSizes& z, char* base, EgTables* t) {
    const size_t at_t1 = (size_t)z.tiles[0] * sizeof(EgTile), at_r0 = at_t1 + (size_t)z.tiles[1] * sizeof(EgTile);
    const size_t at_r1 = at_r0 + (size_t)z.recs[0] * sizeof(EgRows);
    if (base != nullptr) *t = EgTables{{(EgTile*)base, (EgTile*)(base + at_t1)}, {(EgRows*)(base + at_r0), (EgRows*)(base + at_r1)}};
    return at_r1 + (size_t)z.recs[1] * sizeof(EgRows);
}

inline size_t eg_workspace(const EgSizes& z, size_t table_bytes) {
    const int64_t part = z.part[0] > z.part[1] ? z.part[0] : z.part[1];
    return align_up(table_bytes, 256) + align_up((size_t)(part > 0 ? part : 1) * sizeof(float), 256);
}

inline unsigned grid256(int64_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace dmcf

using namespace dmcf;

extern "C" {

size_t dmcf_nn_distance_backward_workspace_bytes(int64_t b, int64_t n, int64_t m) {
    if (b <= 0 || n <= 0 || m <= 0) return 0;
    InvWork w;
    const size_t a = inv_carve(b * m, b * n, nullptr, &w), c = inv_carve(b * n, b * m, nullptr, &w);
    return a > c ? a : c;
}

int dmcf_nn_distance_backward(const float* xyz1, const float* xyz2, int64_t b, int64_t n, int64_t m, const int32_t* idx1,
                              const int32_t* idx2, const float* grad_dist1, const float* grad_dist2, float* grad_xyz1,
                              float* grad_xyz2, void* workspace, size_t workspace_bytes, dmcf_stream_t stream) {
    if (b < 0 || n < 0 || m < 0 || n >= INT32_MAX || m >= INT32_MAX) return DMCF_EINVAL;
    if (b * n >= INT32_MAX || b * m >= INT32_MAX) return DMCF_EINVAL;  // (sorted keys and source indices are 32-bit)
    if (grad_xyz1 == nullptr && grad_xyz2 == nullptr) return DMCF_EINVAL;
    if ((grad_dist1 != nullptr && idx1 == nullptr) || (grad_dist2 != nullptr && idx2 == nullptr)) return DMCF_EINVAL;
    if (b == 0) return DMCF_OK;
    if (n == 0 || m == 0) return DMCF_EINVAL;  // as dmcf_nn_distance
    if (xyz1 == nullptr || xyz2 == nullptr || workspace == nullptr) return DMCF_EINVAL;
    if (workspace_bytes < dmcf_nn_distance_backward_workspace_bytes(b, n, m)) return DMCF_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    for (int dir = 0; dir < 2; ++dir) {
        float* grad = dir == 0 ? grad_xyz1 : grad_xyz2;
        if (grad == nullptr) continue;
        const float* q = dir == 0 ? xyz1 : xyz2;
        const float* o = dir == 0 ? xyz2 : xyz1;
        const int64_t nq = dir == 0 ? n : m, no = dir == 0 ? m : n;
        const float* gq = dir == 0 ? grad_dist1 : grad_dist2;
        const float* go = dir == 0 ? grad_dist2 : grad_dist1;
        const int32_t* idxq = dir == 0 ? idx1 : idx2;
        const int32_t* idxo = dir == 0 ? idx2 : idx1;
        InvWork w{};
        if (go != nullptr) {
            inv_carve(b * no, b * nq, (char*)workspace, &w);
            const int rc = invert_index(idxo, b * no, no, nq, w, st);
            if (rc != DMCF_OK) return rc;
        }
        nn_grad_kernel<<<grid256(b * nq), 256, 0, st>>>(q, nq, o, no, b * nq, gq, idxq, go, w.splits, w.svals, grad);
        if (go != nullptr)
            nn_grad_long_kernel<<<(unsigned)((b * no + kInvShort - 1) / kInvShort), 256, 0, st>>>(q, o, b * no, b * nq, go, w.skeys,
                                                                                               w.splits, w.svals, grad);
        const int rc = check_launch();
        if (rc != DMCF_OK) return rc;
    }
    return DMCF_OK;
}

size_t dmcf_match_cost_backward_workspace_bytes(int64_t b, int64_t n, int64_t m) {
    if (b <= 0 || n <= 0 || m <= 0) return 0;
    const MtPlan p1 = mt_plan(n, m, b), p2 = mt_plan(m, n, b);
    const int64_t e = p1.nsplit * n > p2.nsplit * m ? p1.nsplit * n : p2.nsplit * m;
    return align_up((size_t)(e * b * 3) * sizeof(float), 256);
}

int dmcf_match_cost_backward(const float* xyz1, const float* xyz2, int64_t b, int64_t n, int64_t m, const float* match,
                             const float* grad_cost, float* grad_xyz1, float* grad_xyz2, void* workspace, size_t workspace_bytes,
                             dmcf_stream_t stream) {
    if (b < 0 || n < 0 || m < 0 || b > kMtMaxGridYZ || n >= INT32_MAX || m >= INT32_MAX) return DMCF_EINVAL;
    if (grad_xyz1 == nullptr && grad_xyz2 == nullptr) return DMCF_EINVAL;
    if (b == 0) return DMCF_OK;
    hipStream_t st = (hipStream_t)stream;
    if (n == 0 || m == 0) {  // no pairs: zero gradients
        if (grad_xyz1 != nullptr && n > 0 && hipMemsetAsync(grad_xyz1, 0, (size_t)b * n * 3 * sizeof(float), st) != hipSuccess)
            return check_launch();
        if (grad_xyz2 != nullptr && m > 0 && hipMemsetAsync(grad_xyz2, 0, (size_t)b * m * 3 * sizeof(float), st) != hipSuccess)
            return check_launch();
        return DMCF_OK;
    }
    if (xyz1 == nullptr || xyz2 == nullptr || match == nullptr || grad_cost == nullptr || workspace == nullptr) return DMCF_EINVAL;
    if (workspace_bytes < dmcf_match_cost_backward_workspace_bytes(b, n, m)) return DMCF_EWORKSPACE;
    float* part = (float*)workspace;
    if (grad_xyz1 != nullptr) {  // rows xyz1 (k), columns xyz2 (l): match[l, k] with k across lanes
        const MtPlan p = mt_plan(n, m, b);
        mc_grad_kernel<true><<<dim3((unsigned)p.row_blocks, (unsigned)p.nsplit, (unsigned)b), kMtThreads, 0, st>>>(
            xyz1, n, xyz2, m, p.chunk, match, part);
        grad_combine_kernel<<<grid256(b * n), kMtThreads, 0, st>>>(part, n, n, b, p.nsplit, grad_cost, grad_xyz1);
    }
    if (grad_xyz2 != nullptr) {  // rows xyz2 (l), columns xyz1 (k): match[l, k] staged transposed
        const MtPlan p = mt_plan(m, n, b);
        mc_grad_kernel<false><<<dim3((unsigned)p.row_blocks, (unsigned)p.nsplit, (unsigned)b), kMtThreads, 0, st>>>(
            xyz2, m, xyz1, n, p.chunk, match, part);
        grad_combine_kernel<<<grid256(b * m), kMtThreads, 0, st>>>(part, m, m, b, p.nsplit, grad_cost, grad_xyz2);
    }
    return check_launch();
}

size_t dmcf_emd_backward_workspace_bytes(int64_t b, int64_t n, int64_t m) {
    if (b <= 0 || n <= 0 || m <= 0) return 0;
    const int64_t p1 = mt_partial_bound(n, m), p2 = mt_partial_bound(m, n);
    return align_up((size_t)((p1 > p2 ? p1 : p2) * 3) * sizeof(float), 256);
}

int dmcf_emd_backward(const float* xyz1, const float* xyz2, int64_t b, int64_t n, int64_t m, const int32_t* count1,
                      const int32_t* count2, const float* levels, const float* grad_cost, float* grad_xyz1, float* grad_xyz2,
                      void* workspace, size_t workspace_bytes, dmcf_stream_t stream) {
    if (b < 0 || n < 0 || m < 0 || n >= INT32_MAX || m >= INT32_MAX) return DMCF_EINVAL;
    if (!valid_counts(count1, b, n) || !valid_counts(count2, b, m)) return DMCF_EINVAL;
    if (grad_xyz1 == nullptr && grad_xyz2 == nullptr) return DMCF_EINVAL;
    if (b == 0) return DMCF_OK;
    if (xyz1 == nullptr || xyz2 == nullptr || levels == nullptr || grad_cost == nullptr) return DMCF_EINVAL;
    if (n > 0 && m > 0 && workspace == nullptr) return DMCF_EINVAL;
    if (workspace_bytes < dmcf_emd_backward_workspace_bytes(b, n, m)) return DMCF_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    AmLevels lv;
    for (int L = 0; L < kAmLevels; ++L) lv.v[L] = am_level(L);
    const int64_t lvl_ld = n + m;
    float* part = (float*)workspace;
    for (int64_t i = 0; i < b; ++i) {  // one item after another (as the forward), each with the plan of its own counts
        const int64_t ni = count1 != nullptr ? count1[i] : n, mi = count2 != nullptr ? count2[i] : m;
        const float* x1 = xyz1 + i * n * 3;
        const float* x2 = xyz2 + i * m * 3;
        const float* lvi = levels + i * kAmLevels * lvl_ld;
        for (int side = 0; side < 2; ++side) {
            float* grad = side == 0 ? grad_xyz1 : grad_xyz2;
            if (grad == nullptr) continue;
            const int64_t nout = side == 0 ? n : m;
            grad += i * nout * 3;
            const int64_t nrow = ni == 0 || mi == 0 ? 0 : (side == 0 ? ni : mi), ncol = side == 0 ? mi : ni;
            if (nrow == 0) {
                if (nout > 0 && hipMemsetAsync(grad, 0, (size_t)nout * 3 * sizeof(float), st) != hipSuccess) return check_launch();
                continue;
            }
            const MtPlan p = mt_plan(nrow, ncol);
            const dim3 g((unsigned)p.row_blocks, (unsigned)p.nsplit, 1);
            if (side == 0)
                emd_grad_kernel<true><<<g, kMtThreads, 0, st>>>(x1, ni, x2, mi, p.chunk, lv, lvi, lvi + n, lvl_ld, part);
            else
                emd_grad_kernel<false><<<g, kMtThreads, 0, st>>>(x2, mi, x1, ni, p.chunk, lv, lvi + n, lvi, lvl_ld, part);
            grad_combine_kernel<<<grid256(nout), kMtThreads, 0, st>>>(part, nrow, nout, 1, p.nsplit, grad_cost + i, grad);
            const int rc = check_launch();
            if (rc != DMCF_OK) return rc;
        }
    }
    return DMCF_OK;
}

size_t dmcf_emd_ragged_backward_workspace_bytes(int64_t n_total, const int64_t* row_splits1, int64_t m_total,
                                                const int64_t* row_splits2, int64_t batch) {
    if (!er_valid(n_total, row_splits1, m_total, row_splits2, batch)) return 0;
    const EgSizes z = eg_sizes(row_splits1, row_splits2, batch);
    if (z.tiles[0] > INT32_MAX || z.tiles[1] > INT32_MAX) return 0;
    return eg_workspace(z, eg_tables(z, nullptr, nullptr));
}

int dmcf_emd_ragged_backward(const float* xyz1, int64_t n_total, const int64_t* row_splits1, const float* xyz2, int64_t m_total,
                             const int64_t* row_splits2, int64_t batch, const float* levels, const float* grad_cost,
                             float* grad_xyz1, float* grad_xyz2, void* workspace, size_t workspace_bytes, dmcf_stream_t stream) {
    if (grad_xyz1 == nullptr && grad_xyz2 == nullptr) return DMCF_EINVAL;
    if (batch == 0) return n_total == 0 && m_total == 0 ? DMCF_OK : DMCF_EINVAL;
    if (!er_valid(n_total, row_splits1, m_total, row_splits2, batch)) return DMCF_EINVAL;
    const EgSizes z = eg_sizes(row_splits1, row_splits2, batch);
    if (z.tiles[0] > INT32_MAX || z.tiles[1] > INT32_MAX) return DMCF_EINVAL;  // (one workgroup per tile)
    hipStream_t st = (hipStream_t)stream;
    if (z.tiles[0] == 0) {  // no item has a pair (then neither side has a tile): zero gradients
        if (grad_xyz1 != nullptr && n_total > 0 && hipMemsetAsync(grad_xyz1, 0, (size_t)n_total * 3 * sizeof(float), st) != hipSuccess)
            return check_launch();
        if (grad_xyz2 != nullptr && m_total > 0 && hipMemsetAsync(grad_xyz2, 0, (size_t)m_total * 3 * sizeof(float), st) != hipSuccess)
            return check_launch();
        return DMCF_OK;
    }
    if (xyz1 == nullptr || xyz2 == nullptr || levels == nullptr || grad_cost == nullptr || workspace == nullptr) return DMCF_EINVAL;
    EgTables d, h;  // the tables in the workspace and on the host
    const size_t table_bytes = eg_tables(z, (char*)workspace, &d);
    if (workspace_bytes < eg_workspace(z, table_bytes)) return DMCF_EWORKSPACE;
    float* part = (float*)((char*)workspace + align_up(table_bytes, 256));
    std::vector<char> table(table_bytes);
    eg_tables(z, table.data(), &h);
    for (int side = 0; side < 2; ++side) {  // 0: rows of xyz1 over the item's xyz2; 1: the reverse
        if ((side == 0 ? grad_xyz1 : grad_xyz2) == nullptr) continue;  // (its tables stay zero and are not read)
        const int64_t* rrs = side == 0 ? row_splits1 : row_splits2;
        const int64_t* crs = side == 0 ? row_splits2 : row_splits1;
        int64_t nt = 0, nr = 0, off = 0;
        for (int64_t b = 0; b < batch; ++b) {
            const int64_t rows = rrs[b + 1] - rrs[b], cols = crs[b + 1] - crs[b], r0 = rrs[b], c0 = crs[b];
            const MtPlan p = rows == 0 || cols == 0 ? MtPlan{0, 0, 0} : mt_plan(rows, cols);  // (no pairs: zeros, no tile)
            const int64_t nsplit = p.nsplit;
            for (int64_t first = 0; first < rows; first += kMtThreads) {
                const int64_t cnt = rows - first < kMtThreads ? rows - first : kMtThreads;
                h.r[side][nr++] = EgRows{(int32_t)(r0 + first), (int32_t)cnt, (int32_t)b, (int32_t)nsplit, off + first, (int32_t)rows, 0};
                for (int64_t s = 0; s < nsplit; ++s) {
                    const int64_t a = s * p.chunk, e = a + p.chunk < cols ? a + p.chunk : cols;
                    h.t[side][nt++] = EgTile{(int32_t)(r0 + first), (int32_t)cnt, (int32_t)(c0 + a), (int32_t)(c0 + e),
                                             off + s * 3 * rows + first, (int32_t)rows, 0};
                }
            }
            off += nsplit * 3 * rows;
        }
    }
    // (pageable host memory: the call returns once the tables have left `table`)
    if (hipMemcpyAsync(workspace, table.data(), table.size(), hipMemcpyHostToDevice, st) != hipSuccess) return check_launch();
    AmLevels lv;
    for (int L = 0; L < kAmLevels; ++L) lv.v[L] = am_level(L);
    const int64_t lvl_ld = n_total + m_total;
    // at most 4 launches whatever the batch: the gradient and the combine of every wanted side
    if (grad_xyz1 != nullptr) {
        emd_ragged_grad_kernel<true><<<(unsigned)z.tiles[0], kMtThreads, 0, st>>>(xyz1, xyz2, d.t[0], lv, levels, levels + n_total,
                                                                                  lvl_ld, part);
        emd_ragged_combine_kernel<<<(unsigned)z.recs[0], kMtThreads, 0, st>>>(d.r[0], part, grad_cost, grad_xyz1);
    }
    if (grad_xyz2 != nullptr) {
        emd_ragged_grad_kernel<false><<<(unsigned)z.tiles[1], kMtThreads, 0, st>>>(xyz2, xyz1, d.t[1], lv, levels + n_total, levels,
                                                                                   lvl_ld, part);
        emd_ragged_combine_kernel<<<(unsigned)z.recs[1], kMtThreads, 0, st>>>(d.r[1], part, grad_cost, grad_xyz2);
    }
    return check_launch();
}

size_t dmcf_gather_point_backward_workspace_bytes(int64_t n_index, int64_t n_inp) {
    if (n_index < 0 || n_inp < 0) return 0;
    InvWork w;
    return inv_carve(n_index, n_inp, nullptr, &w);
}

int dmcf_gather_point_backward(const float* grad_out, const int32_t* index, int64_t n_index, int channels, int64_t n_inp,
                               float* grad_inp, void* workspace, size_t workspace_bytes, dmcf_stream_t stream) {
    if (n_index < 0 || n_inp < 0 || channels <= 0 || n_index >= INT32_MAX || n_inp >= INT32_MAX) return DMCF_EINVAL;
    if (n_inp == 0) return DMCF_OK;
    if (grad_inp == nullptr) return DMCF_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (n_index == 0) {
        if (hipMemsetAsync(grad_inp, 0, (size_t)n_inp * channels * sizeof(float), st) != hipSuccess) return check_launch();
        return DMCF_OK;
    }
    if (grad_out == nullptr || index == nullptr || workspace == nullptr) return DMCF_EINVAL;
    if (workspace_bytes < dmcf_gather_point_backward_workspace_bytes(n_index, n_inp)) return DMCF_EWORKSPACE;
    InvWork w;
    inv_carve(n_index, n_inp, (char*)workspace, &w);
    const int rc = invert_index(index, n_index, n_index, n_inp, w, st);
    if (rc != DMCF_OK) return rc;
    gather_grad_kernel<<<grid256(n_inp * channels), 256, 0, st>>>(grad_out, n_inp, channels, w.splits, w.svals, grad_inp);
    gather_grad_long_kernel<<<(unsigned)((n_index + kInvShort - 1) / kInvShort), 256, 0, st>>>(grad_out, n_index, n_inp, channels,
                                                                                            w.skeys, w.splits, w.svals, grad_inp);
    return check_launch();
}

}  // extern "C"
