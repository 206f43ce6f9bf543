// Validation metrics (pipelines/simulator.py:167-285 of the reference): the nearest-neighbour distances of the Chamfer
// metric (utils/tools/nn_distance.*, utils/evaluation_helper.py:25-28) and the approximate-match EMD
// (utils/tools/tf_approxmatch.*, utils/tools/losses.py:401-409).
//
// Both are all-pairs work.  Every pass here is one row-parallel reduction over the whole other set, spread over the
// device as a grid of (row blocks) x (column splits): a workgroup holds 256 rows, one per lane, and walks one contiguous
// chunk of the other set through LDS in tiles of 256 points.  Each (split, row) writes its partial into the workspace;
// a second launch combines the partials of a row in split order.  Nothing is accumulated with atomics, and the split
// plan depends on the sizes alone (not on the device), so two identical calls give identical bits.
//
// Approximate match (behaviour of tf_approxmatch, restated): per batch item with counts n_i (xyz1) and m_i (xyz2),
//   remainL[k] = multiL, remainR[l] = multiR  (n_i >= m_i: 1 and n_i / m_i; else m_i / n_i and 1, integer division)
//   for level in -4^7, -4^6, ..., -4^-1, 0:
//     A  ratioL[k] = remainL[k] / (1e-9 + sum_l e_kl remainR[l])                          e_kl = __expf(level d2_kl)
//     B  s_l = remainR[l] sum_k e_kl ratioL[k];  ratioR[l] = min(remainR[l] / (s_l + 1e-9), 1) remainR[l];
//        remainR[l] = max(0, remainR[l] - s_l)
//     C  w_kl = e_kl ratioL[k] ratioR[l];  match[l, k] += w_kl;  remainL[k] = max(0, remainL[k] - sum_l w_kl)
// and cost = sum_{l,k} match[l, k] sqrt(d2_kl).  The fused entry point (dmcf_emd) adds w_kl sqrt(d2_kl) into a per-row
// partial in pass C instead of forming match.  Batch items run one after another (each with a grid sized to its counts),
// reusing the same workspace.
#include <math.h>

#include <vector>

#include "common.h"
#include "metrics_plan.h"

namespace dmcf {

// ------------------------------------------------------------------------------------------------------------------
// nearest neighbour: per (batch, row) the smallest squared distance into the chunk and its lowest index
// ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kMtThreads) void nn_partial_kernel(const float* __restrict__ q, int64_t nq,
                                                                const float* __restrict__ r, int64_t nr, int64_t chunk,
                                                                float* __restrict__ pd, int32_t* __restrict__ pi) {
    __shared__ float4 tile[kMtTile];
    const int64_t b = blockIdx.z, s = blockIdx.y, nb = gridDim.z;
    const int64_t row = (int64_t)blockIdx.x * kMtThreads + threadIdx.x;
    q += b * nq * 3;
    r += b * nr * 3;
    float qx = 0.0f, qy = 0.0f, qz = 0.0f;
    if (row < nq) {
        qx = q[3 * row];
        qy = q[3 * row + 1];
        qz = q[3 * row + 2];
    }
    const int64_t c0 = s * chunk, c1 = c0 + chunk < nr ? c0 + chunk : nr;
    float best = INFINITY;
    int32_t bi = (int32_t)c0;
    for (int64_t t0 = c0; t0 < c1; t0 += kMtTile) {
        const int cnt = (int)(c1 - t0 < kMtTile ? c1 - t0 : kMtTile);
        __syncthreads();
        if ((int)threadIdx.x < cnt) {
            const int64_t c = t0 + threadIdx.x;
            tile[threadIdx.x] = make_float4(r[3 * c], r[3 * c + 1], r[3 * c + 2], 0.0f);
        }
        __syncthreads();
#pragma unroll 8
        for (int j = 0; j < cnt; ++j) {
            const float4 p = tile[j];
            const float d = dist2_unfused(qx, qy, qz, p.x, p.y, p.z);
            if (d < best) {  // strict: the lowest index of equal distances stays
                best = d;
                bi = (int32_t)(t0 + j);
            }
        }
    }
    if (row < nq) {
        pd[(s * nb + b) * nq + row] = best;
        pi[(s * nb + b) * nq + row] = bi;
    }
}

__global__ __launch_bounds__(kMtThreads) void nn_combine_kernel(const float* __restrict__ pd, const int32_t* __restrict__ pi,
                                                                int64_t total, int64_t nsplit, float* __restrict__ dist,
                                                                int32_t* __restrict__ idx) {
    const int64_t i = (int64_t)blockIdx.x * kMtThreads + threadIdx.x;
    if (i >= total) return;
    float best = pd[i];
    int32_t bi = pi[i];
    for (int64_t s = 1; s < nsplit; ++s) {  // splits in column order: strict < keeps the lowest index
        const float d = pd[s * total + i];
        if (d < best) {
            best = d;
            bi = pi[s * total + i];
        }
    }
    dist[i] = best;
    if (idx != nullptr) idx[i] = bi;
}

// ------------------------------------------------------------------------------------------------------------------
// nearest neighbour over a ragged batch (ABI 2.23): many items of tens to a few thousand rows.  Every item's rows are cut into
// tiles of one wavefront; a workgroup IS one wavefront, takes one tile and walks its own item's other set through LDS from the
// first column to the last with the dense kernel's distance and strict <, so a row's result has the dense call's bits without a
// combine pass.  The tile table is written by the host from the row splits it has validated: the kernel reads no row splits,
// and every index it forms lies inside the arrays by construction.
// ------------------------------------------------------------------------------------------------------------------
constexpr int kNrRows = 64;   // rows per tile = lanes of a wavefront
constexpr int kNrTile = 256;  // points of the other set per LDS tile
constexpr int64_t kNrMaxBatch = (int64_t)1 << 26;  // (the limit of the batched searches)

struct NrTile {
    int32_t row0, rows;  // the tile's rows [row0, row0 + rows) of the concatenated set, 1 <= rows <= kNrRows
    int32_t c0, c1;      // its item's other set [c0, c1) of the concatenated other set, c0 < c1
};
static_assert(sizeof(NrTile) == 16, "NrTile is read as one 16-byte load");

__global__ __launch_bounds__(kNrRows) void nn_ragged_kernel(const float* __restrict__ q, const float* __restrict__ r,
                                                            const NrTile* __restrict__ tiles, float* __restrict__ dist,
                                                            int32_t* __restrict__ idx) {
    __shared__ float4 tile[kNrTile];
    const NrTile t = tiles[blockIdx.x];
    const int lane = (int)threadIdx.x;
    const bool live = lane < t.rows;
    const int64_t row = (int64_t)t.row0 + lane;
    float qx = 0.0f, qy = 0.0f, qz = 0.0f;
    if (live) {
        qx = q[3 * row];
        qy = q[3 * row + 1];
        qz = q[3 * row + 2];
    }
    float best = INFINITY;
    int32_t bi = t.c0;
    for (int32_t t0 = t.c0; t0 < t.c1; t0 += kNrTile) {  // (c1 < 2^31 - 1 - kNrTile is checked by the host)
        const int cnt = t.c1 - t0 < kNrTile ? t.c1 - t0 : kNrTile;
        __syncthreads();
        for (int k = lane; k < cnt; k += kNrRows) {
            const int64_t c = (int64_t)t0 + k;
            tile[k] = make_float4(r[3 * c], r[3 * c + 1], r[3 * c + 2], 0.0f);
        }
        __syncthreads();
#pragma unroll 8
        for (int j = 0; j < cnt; ++j) {
            const float4 p = tile[j];
            const float d = dist2_unfused(qx, qy, qz, p.x, p.y, p.z);
            if (d < best) {  // strict, columns ascending: the lowest index of equal distances stays
                best = d;
                bi = t0 + j;
            }
        }
    }
    if (live) {
        dist[row] = best;
        idx[row] = bi;
    }
}

inline int64_t nr_tile_bound(int64_t rows, int64_t batch) { return rows / kNrRows + batch; }  // every item adds <= 1 partial tile

// host row splits of `batch` items over `total` rows: start at 0, do not decrease, end at total
bool valid_row_splits(const int64_t* rs, int64_t batch, int64_t total) {
    if (rs[0] != 0 || rs[batch] != total) return false;
    for (int64_t b = 0; b < batch; ++b)
        if (rs[b + 1] < rs[b]) return false;
    return true;
}

// ------------------------------------------------------------------------------------------------------------------
// approximate match: one kernel for the three all-pairs passes and the cost of a given match
// ------------------------------------------------------------------------------------------------------------------
enum MtMode {
    kMtSumWeighted = 0,  // part[row] = sum_c e_rc cw[c]                          (passes A and B)
    kMtMatch = 1,        // w = e_rc cw[c] rw[row]; match[c, row] += w; part = sum w   (pass C, dense)
    kMtFused = 2,        // w as above; part = sum w; part2 = sum w sqrt(d2)           (pass C, fused EMD)
    kMtCost = 3,         // part = sum_c match[c, row] sqrt(d2_rc)                     (dmcf_match_cost)
};

template <int MODE>
__global__ __launch_bounds__(kMtThreads) void am_pass_kernel(const float* __restrict__ rp, int64_t nrow, int64_t rp_bs,
                                                             const float* __restrict__ cp, int64_t ncol, int64_t cp_bs,
                                                             int64_t chunk, float level, const float* __restrict__ cw,
                                                             const float* __restrict__ rw, float* __restrict__ match,
                                                             int64_t ld, int64_t match_bs, float* __restrict__ part,
                                                             float* __restrict__ part2) {
    __shared__ float4 tile[kMtTile];
    const int64_t b = blockIdx.z, s = blockIdx.y, nb = gridDim.z;
    const int64_t row = (int64_t)blockIdx.x * kMtThreads + threadIdx.x;
    const bool live = row < nrow;
    rp += b * rp_bs;
    cp += b * cp_bs;
    float x = 0.0f, y = 0.0f, z = 0.0f, rs = 0.0f;
    if (live) {
        x = rp[3 * row];
        y = rp[3 * row + 1];
        z = rp[3 * row + 2];
        if (MODE == kMtMatch || MODE == kMtFused) rs = rw[row];
    }
    float* mrow = nullptr;
    if (MODE == kMtMatch || MODE == kMtCost) mrow = match + b * match_bs + row;
    const int64_t c0 = s * chunk, c1 = c0 + chunk < ncol ? c0 + chunk : ncol;
    float sum = 0.0f, sum2 = 0.0f;
    for (int64_t t0 = c0; t0 < c1; t0 += kMtTile) {
        const int cnt = (int)(c1 - t0 < kMtTile ? c1 - t0 : kMtTile);
        __syncthreads();
        if ((int)threadIdx.x < cnt) {
            const int64_t c = t0 + threadIdx.x;
            tile[threadIdx.x] = make_float4(cp[3 * c], cp[3 * c + 1], cp[3 * c + 2], MODE == kMtCost ? 0.0f : cw[c]);
        }
        __syncthreads();
#pragma unroll 4
        for (int j = 0; j < cnt; ++j) {
            const float4 p = tile[j];
            const float dx = x - p.x, dy = y - p.y, dz = z - p.z;
            const float d2 = fmaf(dx, dx, fmaf(dy, dy, dz * dz));
            if (MODE == kMtCost) {
                const float mv = live ? mrow[(t0 + j) * ld] : 0.0f;
                sum = fmaf(mv, __builtin_amdgcn_sqrtf(d2), sum);
            } else {
                const float e = __expf(level * d2) * p.w;
                if (MODE == kMtSumWeighted) {
                    sum += e;
                } else {
                    const float w = e * rs;
                    sum += w;
                    if (MODE == kMtMatch) {
                        if (live) mrow[(t0 + j) * ld] += w;
                    } else {
                        sum2 = fmaf(w, __builtin_amdgcn_sqrtf(d2), sum2);
                    }
                }
            }
        }
    }
    if (live) {
        part[(s * nb + b) * nrow + row] = sum;
        if (MODE == kMtFused) part2[(s * nb + b) * nrow + row] = sum2;
    }
}

__global__ __launch_bounds__(kMtThreads) void am_init_kernel(float* __restrict__ remainL, float* __restrict__ costL, int64_t n,
                                                             float multiL, float* __restrict__ remainR, int64_t m, float multiR) {
    const int64_t i = (int64_t)blockIdx.x * kMtThreads + threadIdx.x;
    if (i < n) {
        remainL[i] = multiL;
        costL[i] = 0.0f;
    }
    if (i < m) remainR[i] = multiR;
}

// pass A: ratioL[k] = remainL[k] / (1e-9 + sum)
__global__ __launch_bounds__(kMtThreads) void am_finish_a_kernel(const float* __restrict__ part, int64_t n, int64_t nsplit,
                                                                 const float* __restrict__ remainL, float* __restrict__ ratioL) {
    const int64_t k = (int64_t)blockIdx.x * kMtThreads + threadIdx.x;
    if (k >= n) return;
    float s = 1e-9f;
    for (int64_t j = 0; j < nsplit; ++j) s += part[j * n + k];
    ratioL[k] = remainL[k] / s;
}

// pass B: s_l = remainR[l] sum; ratioR[l] = min(remainR[l] / (s_l + 1e-9), 1) remainR[l]; remainR[l] = max(0, remainR[l] - s_l)
__global__ __launch_bounds__(kMtThreads) void am_finish_b_kernel(const float* __restrict__ part, int64_t m, int64_t nsplit,
                                                                 float* __restrict__ remainR, float* __restrict__ ratioR) {
    const int64_t l = (int64_t)blockIdx.x * kMtThreads + threadIdx.x;
    if (l >= m) return;
    float s = 0.0f;
    for (int64_t j = 0; j < nsplit; ++j) s += part[j * m + l];
    const float rr = remainR[l];
    s *= rr;
    ratioR[l] = fminf(rr / (s + 1e-9f), 1.0f) * rr;
    remainR[l] = fmaxf(0.0f, rr - s);
}

// pass C: remainL[k] = max(0, remainL[k] - sum w); fused: costL[k] += sum w sqrt(d2)
__global__ __launch_bounds__(kMtThreads) void am_finish_c_kernel(const float* __restrict__ part, const float* __restrict__ part2,
                                                                 int64_t n, int64_t nsplit, float* __restrict__ remainL,
                                                                 float* __restrict__ costL) {
    const int64_t k = (int64_t)blockIdx.x * kMtThreads + threadIdx.x;
    if (k >= n) return;
    float s = 0.0f, c = 0.0f;
    for (int64_t j = 0; j < nsplit; ++j) s += part[j * n + k];
    remainL[k] = fmaxf(0.0f, remainL[k] - s);
    if (part2 != nullptr) {
        for (int64_t j = 0; j < nsplit; ++j) c += part2[j * n + k];
        costL[k] += c;
    }
}

// out[b] = sum_{s, k} part[(s * nb + b) * n + k], one workgroup per batch item, fixed order (strided per lane, then a tree)
__global__ __launch_bounds__(kMtThreads) void am_total_kernel(const float* __restrict__ part, int64_t n, int64_t nsplit,
                                                              float* __restrict__ out) {
    __shared__ float red[kMtThreads];
    const int64_t b = blockIdx.x, nb = gridDim.x;
    float s = 0.0f;
    for (int64_t j = 0; j < nsplit; ++j)
        for (int64_t k = threadIdx.x; k < n; k += kMtThreads) s += part[(j * nb + b) * n + k];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = kMtThreads / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[b] = red[0];
}

inline unsigned grid1(int64_t n) { return (unsigned)((n + kMtThreads - 1) / kMtThreads); }

// workspace of dmcf_approx_match / dmcf_emd, carved from the caller's block
struct AmWork {
    float *remainL, *ratioL, *costL, *remainR, *ratioR, *part, *part2;
};

inline size_t am_carve(int64_t n, int64_t m, char* base, AmWork* w) {
    const int64_t pn = mt_partial_bound(n, m), pm = mt_partial_bound(m, n);
    const int64_t sizes[7] = {n, n, n, m, m, pn > pm ? pn : pm, pn};
    float** dst[7] = {&w->remainL, &w->ratioL, &w->costL, &w->remainR, &w->ratioR, &w->part, &w->part2};
    size_t off = 0;
    for (int i = 0; i < 7; ++i) {
        if (base != nullptr) *dst[i] = (float*)(base + off);
        off += align_up((size_t)(sizes[i] > 0 ? sizes[i] : 1) * sizeof(float), 256);
    }
    return off;
}

bool valid_counts(const int32_t* counts, int64_t b, int64_t limit) {
    if (counts == nullptr) return true;
    for (int64_t i = 0; i < b; ++i)
        if (counts[i] < 0 || counts[i] > limit) return false;
    return true;
}

// one batch item of the approximate match: match (dense, already zeroed) or costL (fused) and the final total into *cost;
// levels (NULL: not wanted): per level L the copies of ratioL (after pass A) at levels[L * lvl_ld] and of ratioR (after pass B)
// at levels[L * lvl_ld + lvl_r] (dmcf_emd_with_levels, the saved state of dmcf_emd_backward)
int approx_match_item(const float* xyz1, const float* xyz2, int64_t ni, int64_t mi, float* match, int64_t ld, float* cost,
                      const AmWork& w, hipStream_t st, float* levels = nullptr, int64_t lvl_ld = 0, int64_t lvl_r = 0) {
    const float multiL = ni >= mi ? 1.0f : (float)(mi / ni);
    const float multiR = ni >= mi ? (float)(ni / mi) : 1.0f;
    const int64_t nm = ni > mi ? ni : mi;
    am_init_kernel<<<grid1(nm), kMtThreads, 0, st>>>(w.remainL, w.costL, ni, multiL, w.remainR, mi, multiR);
    const MtPlan pa = mt_plan(ni, mi), pb = mt_plan(mi, ni);
    const dim3 ga((unsigned)pa.row_blocks, (unsigned)pa.nsplit, 1), gb((unsigned)pb.row_blocks, (unsigned)pb.nsplit, 1);
    for (int L = 0; L < kAmLevels; ++L) {  // (the schedule of metrics_plan.h, shared with dmcf_emd_backward)
        const float level = am_level(L);
        am_pass_kernel<kMtSumWeighted><<<ga, kMtThreads, 0, st>>>(xyz1, ni, 0, xyz2, mi, 0, pa.chunk, level, w.remainR, nullptr,
                                                                  nullptr, 0, 0, w.part, nullptr);
        am_finish_a_kernel<<<grid1(ni), kMtThreads, 0, st>>>(w.part, ni, pa.nsplit, w.remainL, w.ratioL);
        float* lv = levels != nullptr ? levels + L * lvl_ld : nullptr;
        if (lv != nullptr && hipMemcpyAsync(lv, w.ratioL, (size_t)ni * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess)
            return check_launch();
        am_pass_kernel<kMtSumWeighted><<<gb, kMtThreads, 0, st>>>(xyz2, mi, 0, xyz1, ni, 0, pb.chunk, level, w.ratioL, nullptr,
                                                                  nullptr, 0, 0, w.part, nullptr);
        am_finish_b_kernel<<<grid1(mi), kMtThreads, 0, st>>>(w.part, mi, pb.nsplit, w.remainR, w.ratioR);
        if (lv != nullptr &&
            hipMemcpyAsync(lv + lvl_r, w.ratioR, (size_t)mi * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess)
            return check_launch();
        if (match != nullptr)
            am_pass_kernel<kMtMatch><<<ga, kMtThreads, 0, st>>>(xyz1, ni, 0, xyz2, mi, 0, pa.chunk, level, w.ratioR, w.ratioL,
                                                                match, ld, 0, w.part, nullptr);
        else
            am_pass_kernel<kMtFused><<<ga, kMtThreads, 0, st>>>(xyz1, ni, 0, xyz2, mi, 0, pa.chunk, level, w.ratioR, w.ratioL,
                                                                nullptr, 0, 0, w.part, w.part2);
        am_finish_c_kernel<<<grid1(ni), kMtThreads, 0, st>>>(w.part, match != nullptr ? nullptr : w.part2, ni, pa.nsplit,
                                                             w.remainL, w.costL);
    }
    if (cost != nullptr) am_total_kernel<<<1, kMtThreads, 0, st>>>(w.costL, ni, 1, cost);
    return check_launch();
}

int approx_match_common(const float* xyz1, const float* xyz2, int64_t b, int64_t n, int64_t m, const int32_t* count1,
                        const int32_t* count2, float* match, float* cost, void* workspace, size_t workspace_bytes,
                        dmcf_stream_t stream, float* levels = nullptr) {
    if (b < 0 || n < 0 || m < 0 || n >= INT32_MAX || m >= INT32_MAX) return DMCF_EINVAL;
    if (!valid_counts(count1, b, n) || !valid_counts(count2, b, m)) return DMCF_EINVAL;
    if (b == 0) return DMCF_OK;
    if (xyz1 == nullptr || xyz2 == nullptr || (match == nullptr && cost == nullptr) || workspace == nullptr) return DMCF_EINVAL;
    AmWork w;
    if (workspace_bytes < am_carve(n, m, nullptr, &w)) return DMCF_EWORKSPACE;
    am_carve(n, m, (char*)workspace, &w);
    hipStream_t st = (hipStream_t)stream;
    if (match != nullptr && n > 0 && m > 0) {
        if (hipMemsetAsync(match, 0, (size_t)b * n * m * sizeof(float), st) != hipSuccess) return check_launch();
    }
    const int64_t lvl_ld = n + m;  // levels [b, kAmLevels, n + m]: ratioL in [0, n_i), ratioR in [n, n + m_i), zeros elsewhere
    if (levels != nullptr && hipMemsetAsync(levels, 0, (size_t)b * kAmLevels * lvl_ld * sizeof(float), st) != hipSuccess)
        return check_launch();
    for (int64_t i = 0; i < b; ++i) {
        const int64_t ni = count1 != nullptr ? count1[i] : n, mi = count2 != nullptr ? count2[i] : m;
        if (ni == 0 || mi == 0) {  // nothing to match: zero match rows (already), zero cost
            if (cost != nullptr && hipMemsetAsync(cost + i, 0, sizeof(float), st) != hipSuccess) return check_launch();
            continue;
        }
        const int rc = approx_match_item(xyz1 + i * n * 3, xyz2 + i * m * 3, ni, mi, match != nullptr ? match + i * n * m : nullptr,
                                         n, match != nullptr ? nullptr : cost + i, w, st,
                                         levels != nullptr ? levels + i * kAmLevels * lvl_ld : nullptr, lvl_ld, n);
        if (rc != DMCF_OK) return rc;
    }
    return check_launch();
}

// ------------------------------------------------------------------------------------------------------------------
// the fused EMD over a ragged batch (ABI 2.24): the passes, finish steps and totals of approx_match_item, each ONE launch over
// the tiles of ALL items, so the number of launches (the 62 of one approx_match_item) does not depend on the batch.  An item keeps the column
// chunks of its own mt_plan and every sum keeps approx_match_item's order, so cost[b] has dmcf_emd's bits for item b alone.
// The host writes the tables from the row splits it has validated: a pass tile per (item, row block, column chunk), a row
// record per (item, row block) for the finish steps, one record per item for the totals.  No kernel reads row splits, and
// every index lies inside the arrays by construction of the tables.  The state arrays run over the concatenated rows; an
// item's partials are [nsplit, rows of the item] at its own base.
// ------------------------------------------------------------------------------------------------------------------
struct ErTile {          // one workgroup of a pass
    int32_t row0, rows;  // rows [row0, row0 + rows) of the concatenated row set, 1 <= rows <= kMtThreads
    int32_t c0, c1;      // the chunk [c0, c1) of the concatenated column set, c0 < c1
    int64_t pbase;       // part[pbase + lane]: the partial of (this chunk, row0 + lane)
};
static_assert(sizeof(ErTile) == 24, "ErTile is packed");

struct ErRows {             // one workgroup of a finish step or of the init
    int32_t row0, rows;     // as above
    int32_t stride, nsplit; // the row's partials: part[pbase + j * stride + lane], j < nsplit in split order
    int64_t pbase;
    float mult;             // the initial remain of the item's rows on this side (multiL / multiR)
    int32_t left;           // 1: rows of xyz1 (remainL, costL), 0: rows of xyz2 (remainR)
};
static_assert(sizeof(ErRows) == 32, "ErRows is packed");

struct ErItem {
    int32_t row0, rows;  // the item's rows of xyz1; rows == 0 when either of its sets is empty (cost 0)
};

template <int MODE>  // kMtSumWeighted (passes A and B) or kMtFused (pass C): the column walk of am_pass_kernel
__global__ __launch_bounds__(kMtThreads) void er_pass_kernel(const float* __restrict__ rp, const float* __restrict__ cp,
                                                             const ErTile* __restrict__ tiles, float level,
                                                             const float* __restrict__ cw, const float* __restrict__ rw,
                                                             float* __restrict__ part, float* __restrict__ part2) {
    static_assert(MODE == kMtSumWeighted || MODE == kMtFused, "the ragged form has the fused passes only");
    __shared__ float4 tile[kMtTile];
    const ErTile t = tiles[blockIdx.x];
    const int lane = (int)threadIdx.x;
    const bool live = lane < t.rows;
    const int64_t row = (int64_t)t.row0 + lane;
    float x = 0.0f, y = 0.0f, z = 0.0f, rs = 0.0f;
    if (live) {
        x = rp[3 * row];
        y = rp[3 * row + 1];
        z = rp[3 * row + 2];
        if (MODE == kMtFused) rs = rw[row];
    }
    float sum = 0.0f, sum2 = 0.0f;
    for (int32_t t0 = t.c0; t0 < t.c1; t0 += kMtTile) {  // (c1 < 2^31 - 1 - kMtTile is checked by the host)
        const int cnt = t.c1 - t0 < kMtTile ? t.c1 - t0 : kMtTile;
        __syncthreads();
        if (lane < cnt) {
            const int64_t c = (int64_t)t0 + lane;
            tile[lane] = make_float4(cp[3 * c], cp[3 * c + 1], cp[3 * c + 2], cw[c]);
        }
        __syncthreads();
#pragma unroll 4
        for (int j = 0; j < cnt; ++j) {
            const float4 p = tile[j];
            const float dx = x - p.x, dy = y - p.y, dz = z - p.z;
            const float d2 = fmaf(dx, dx, fmaf(dy, dy, dz * dz));
            const float e = __expf(level * d2) * p.w;
            if (MODE == kMtSumWeighted) {
                sum += e;
            } else {
                const float w = e * rs;
                sum += w;
                sum2 = fmaf(w, __builtin_amdgcn_sqrtf(d2), sum2);
            }
        }
    }
    if (live) {
        part[t.pbase + lane] = sum;
        if (MODE == kMtFused) part2[t.pbase + lane] = sum2;
    }
}

__global__ __launch_bounds__(kMtThreads) void er_init_kernel(const ErRows* __restrict__ recs, float* __restrict__ remainL,
                                                             float* __restrict__ costL, float* __restrict__ remainR) {
    const ErRows r = recs[blockIdx.x];
    if ((int)threadIdx.x >= r.rows) return;
    const int64_t k = (int64_t)r.row0 + threadIdx.x;
    if (r.left != 0) {
        remainL[k] = r.mult;
        costL[k] = 0.0f;
    } else {
        remainR[k] = r.mult;
    }
}

// the three finish steps, with the sums and expressions of am_finish_a / b / c_kernel
// lv (NULL: not wanted): the level's row of dmcf_emd_ragged_with_levels, which takes a copy of the ratio
__global__ __launch_bounds__(kMtThreads) void er_finish_a_kernel(const ErRows* __restrict__ recs, const float* __restrict__ part,
                                                                 const float* __restrict__ remainL, float* __restrict__ ratioL,
                                                                 float* __restrict__ lv) {
    const ErRows r = recs[blockIdx.x];
    if ((int)threadIdx.x >= r.rows) return;
    const int64_t k = (int64_t)r.row0 + threadIdx.x;
    const float* p = part + r.pbase + threadIdx.x;
    float s = 1e-9f;
    for (int32_t j = 0; j < r.nsplit; ++j) s += p[(int64_t)j * r.stride];
    const float v = remainL[k] / s;
    ratioL[k] = v;
    if (lv != nullptr) lv[k] = v;
}

__global__ __launch_bounds__(kMtThreads) void er_finish_b_kernel(const ErRows* __restrict__ recs, const float* __restrict__ part,
                                                                 float* __restrict__ remainR, float* __restrict__ ratioR,
                                                                 float* __restrict__ lv) {
    const ErRows r = recs[blockIdx.x];
    if ((int)threadIdx.x >= r.rows) return;
    const int64_t l = (int64_t)r.row0 + threadIdx.x;
    const float* p = part + r.pbase + threadIdx.x;
    float s = 0.0f;
    for (int32_t j = 0; j < r.nsplit; ++j) s += p[(int64_t)j * r.stride];
    const float rr = remainR[l];
    s *= rr;
    const float v = fminf(rr / (s + 1e-9f), 1.0f) * rr;
    ratioR[l] = v;
    if (lv != nullptr) lv[l] = v;
    remainR[l] = fmaxf(0.0f, rr - s);
}

__global__ __launch_bounds__(kMtThreads) void er_finish_c_kernel(const ErRows* __restrict__ recs, const float* __restrict__ part,
                                                                 const float* __restrict__ part2, float* __restrict__ remainL,
                                                                 float* __restrict__ costL) {
    const ErRows r = recs[blockIdx.x];
    if ((int)threadIdx.x >= r.rows) return;
    const int64_t k = (int64_t)r.row0 + threadIdx.x;
    const float* p = part + r.pbase + threadIdx.x;
    const float* p2 = part2 + r.pbase + threadIdx.x;
    float s = 0.0f, c = 0.0f;
    for (int32_t j = 0; j < r.nsplit; ++j) s += p[(int64_t)j * r.stride];
    remainL[k] = fmaxf(0.0f, remainL[k] - s);
    for (int32_t j = 0; j < r.nsplit; ++j) c += p2[(int64_t)j * r.stride];
    costL[k] += c;
}

// cost[b] = the sum of the item's costL in am_total_kernel's order (strided per lane, then a tree); one workgroup per item
__global__ __launch_bounds__(kMtThreads) void er_total_kernel(const ErItem* __restrict__ items, const float* __restrict__ costL,
                                                              float* __restrict__ cost) {
    __shared__ float red[kMtThreads];
    const ErItem it = items[blockIdx.x];
    const float* c = costL + it.row0;
    float s = 0.0f;
    for (int32_t k = (int32_t)threadIdx.x; k < it.rows; k += kMtThreads) s += c[k];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = kMtThreads / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) cost[blockIdx.x] = red[0];
}

// what the validated splits ask of the workspace: the tables' record counts and the partials of every item's plan
struct ErSizes {
    int64_t tiles_a = 0, tiles_b = 0;  // pass tiles with rows of xyz1 (passes A and C) / of xyz2 (pass B)
    int64_t rows_a = 0, rows_b = 0;    // row records of xyz1 / xyz2
    int64_t part_a = 0, part_b = 0;    // floats of partials: sum of nsplit * rows over the items
};

inline ErSizes er_sizes(const int64_t* rs1, const int64_t* rs2, int64_t batch) {
    ErSizes z;
    for (int64_t b = 0; b < batch; ++b) {
        const int64_t n = rs1[b + 1] - rs1[b], m = rs2[b + 1] - rs2[b];
        if (n == 0 || m == 0) continue;
        const MtPlan pa = mt_plan(n, m), pb = mt_plan(m, n);
        z.tiles_a += pa.row_blocks * pa.nsplit;
        z.tiles_b += pb.row_blocks * pb.nsplit;
        z.rows_a += pa.row_blocks;
        z.rows_b += pb.row_blocks;
        z.part_a += pa.nsplit * n;
        z.part_b += pb.nsplit * m;
    }
    return z;
}

// the tables of dmcf_emd_ragged, one block at the start of its workspace (one copy from the host's block of the same layout)
struct ErTables {
    ErTile *ta, *tb;
    ErRows *ra, *rb;  // (adjacent: the init walks them as one array)
    ErItem* items;
};

inline size_t er_tables(const ErSizes& z, int64_t batch, char* base, ErTables* t) {
    const size_t at_tb = (size_t)z.tiles_a * sizeof(ErTile), at_ra = at_tb + (size_t)z.tiles_b * sizeof(ErTile);
    const size_t at_rb = at_ra + (size_t)z.rows_a * sizeof(ErRows), at_items = at_rb + (size_t)z.rows_b * sizeof(ErRows);
    if (base != nullptr) *t = ErTables{(ErTile*)base, (ErTile*)(base + at_tb), (ErRows*)(base + at_ra), (ErRows*)(base + at_rb),
                                       (ErItem*)(base + at_items)};
    return at_items + (size_t)batch * sizeof(ErItem);
}

// the rest of the workspace, from `off` on: the state arrays over the concatenated rows and the partials
inline size_t er_carve(const ErSizes& z, int64_t n_total, int64_t m_total, size_t off, char* base, AmWork* w) {
    const int64_t sizes[7] = {n_total, n_total, n_total, m_total, m_total, z.part_a > z.part_b ? z.part_a : z.part_b, z.part_a};
    float** dst[7] = {&w->remainL, &w->ratioL, &w->costL, &w->remainR, &w->ratioR, &w->part, &w->part2};
    off = align_up(off, 256);
    for (int i = 0; i < 7; ++i) {
        if (base != nullptr) *dst[i] = (float*)(base + off);
        off += align_up((size_t)(sizes[i] > 0 ? sizes[i] : 1) * sizeof(float), 256);
    }
    return off;
}

// the argument checks the ragged EMD entry points and their workspace queries share (no pointer but the splits is looked at)
bool er_valid(int64_t n_total, const int64_t* rs1, int64_t m_total, const int64_t* rs2, int64_t batch) {
    if (batch < 1 || batch > kNrMaxBatch || n_total < 0 || m_total < 0) return false;
    if (n_total >= INT32_MAX - kMtTile || m_total >= INT32_MAX - kMtTile) return false;  // (int32 indices)
    if (rs1 == nullptr || rs2 == nullptr) return false;
    return valid_row_splits(rs1, batch, n_total) && valid_row_splits(rs2, batch, m_total);
}

// dmcf_emd_ragged, and with `record` dmcf_emd_ragged_with_levels: levels [kAmLevels, n_total + m_total] is zeroed, then every
// level's finish steps A and B write their ratios into its row as well (rows of items without pairs stay zero)
int emd_ragged_common(const float* xyz1, int64_t n_total, const int64_t* row_splits1, const float* xyz2, int64_t m_total,
                      const int64_t* row_splits2, int64_t batch, float* cost, bool record, float* levels, void* workspace,
                      size_t workspace_bytes, dmcf_stream_t stream) {
    if (batch == 0) return n_total == 0 && m_total == 0 ? DMCF_OK : DMCF_EINVAL;
    if (!er_valid(n_total, row_splits1, m_total, row_splits2, batch)) return DMCF_EINVAL;
    if (n_total == 0 && m_total == 0) return DMCF_OK;  // (every item empty on both sides: nothing enqueued)
    if (record && levels == nullptr) return DMCF_EINVAL;
    if (cost == nullptr || workspace == nullptr || (xyz1 == nullptr && n_total > 0) || (xyz2 == nullptr && m_total > 0))
        return DMCF_EINVAL;
    const ErSizes z = er_sizes(row_splits1, row_splits2, batch);
    if (z.tiles_a > INT32_MAX || z.tiles_b > INT32_MAX) return DMCF_EINVAL;  // (one workgroup per tile)
    ErTables d, h;  // the tables in the workspace and on the host
    AmWork w;
    const size_t table_bytes = er_tables(z, batch, (char*)workspace, &d);
    if (workspace_bytes < er_carve(z, n_total, m_total, table_bytes, (char*)workspace, &w)) return DMCF_EWORKSPACE;
    std::vector<char> table(table_bytes);
    er_tables(z, batch, table.data(), &h);
    int64_t na = 0, nb = 0, ra = 0, rb = 0, off_a = 0, off_b = 0;
    for (int64_t b = 0; b < batch; ++b) {
        const int64_t n = row_splits1[b + 1] - row_splits1[b], m = row_splits2[b + 1] - row_splits2[b];
        if (n == 0 || m == 0) {  // nothing to match: cost 0
            h.items[b] = ErItem{0, 0};
            continue;
        }
        h.items[b] = ErItem{(int32_t)row_splits1[b], (int32_t)n};
        for (int side = 0; side < 2; ++side) {  // 0: rows of xyz1 over the item's xyz2 (passes A and C); 1: the reverse (pass B)
            const int64_t rows = side == 0 ? n : m, cols = side == 0 ? m : n;
            const int64_t r0 = side == 0 ? row_splits1[b] : row_splits2[b], c0 = side == 0 ? row_splits2[b] : row_splits1[b];
            const MtPlan p = mt_plan(rows, cols);
            // the multipliers of approx_match_item: 1 on the larger side, the integer quotient on the smaller
            const float mult = side == 0 ? (n >= m ? 1.0f : (float)(m / n)) : (n >= m ? (float)(n / m) : 1.0f);
            int64_t& off = side == 0 ? off_a : off_b;
            for (int64_t k = 0; k < p.row_blocks; ++k) {
                const int64_t first = k * kMtThreads, cnt = rows - first < kMtThreads ? rows - first : kMtThreads;
                (side == 0 ? h.ra[ra++] : h.rb[rb++]) =
                    ErRows{(int32_t)(r0 + first), (int32_t)cnt, (int32_t)rows, (int32_t)p.nsplit, off + first, mult, side == 0};
                for (int64_t s = 0; s < p.nsplit; ++s) {
                    const int64_t a = s * p.chunk, e = a + p.chunk < cols ? a + p.chunk : cols;
                    (side == 0 ? h.ta[na++] : h.tb[nb++]) =
                        ErTile{(int32_t)(r0 + first), (int32_t)cnt, (int32_t)(c0 + a), (int32_t)(c0 + e), off + s * rows + first};
                }
            }
            off += p.nsplit * rows;
        }
    }
    hipStream_t st = (hipStream_t)stream;
    // (pageable host memory: the call returns once the tables have left `table`)
    if (hipMemcpyAsync(workspace, table.data(), table.size(), hipMemcpyHostToDevice, st) != hipSuccess) return check_launch();
    const int64_t lvl_ld = n_total + m_total;
    if (record && hipMemsetAsync(levels, 0, (size_t)kAmLevels * lvl_ld * sizeof(float), st) != hipSuccess) return check_launch();
    // 2 + 6 kAmLevels launches whatever the batch: each one covers the tiles or rows of every item
    if (z.tiles_a > 0) {
        const unsigned ga = (unsigned)z.tiles_a, gb = (unsigned)z.tiles_b, fa = (unsigned)z.rows_a, fb = (unsigned)z.rows_b;
        er_init_kernel<<<fa + fb, kMtThreads, 0, st>>>(d.ra, w.remainL, w.costL, w.remainR);
        for (int L = 0; L < kAmLevels; ++L) {
            const float level = am_level(L);
            er_pass_kernel<kMtSumWeighted><<<ga, kMtThreads, 0, st>>>(xyz1, xyz2, d.ta, level, w.remainR, nullptr, w.part, nullptr);
            float* lv = record ? levels + L * lvl_ld : nullptr;
            er_finish_a_kernel<<<fa, kMtThreads, 0, st>>>(d.ra, w.part, w.remainL, w.ratioL, lv);
            er_pass_kernel<kMtSumWeighted><<<gb, kMtThreads, 0, st>>>(xyz2, xyz1, d.tb, level, w.ratioL, nullptr, w.part, nullptr);
            er_finish_b_kernel<<<fb, kMtThreads, 0, st>>>(d.rb, w.part, w.remainR, w.ratioR, lv != nullptr ? lv + n_total : nullptr);
            er_pass_kernel<kMtFused><<<ga, kMtThreads, 0, st>>>(xyz1, xyz2, d.ta, level, w.ratioR, w.ratioL, w.part, w.part2);
            er_finish_c_kernel<<<fa, kMtThreads, 0, st>>>(d.ra, w.part, w.part2, w.remainL, w.costL);
        }
    }
    er_total_kernel<<<(unsigned)batch, kMtThreads, 0, st>>>(d.items, w.costL, cost);
    return check_launch();
}

}  // namespace dmcf

using namespace dmcf;

extern "C" {

size_t dmcf_nn_distance_workspace_bytes(int64_t b, int64_t n, int64_t m) {
    if (b <= 0 || n <= 0 || m <= 0) return 0;
    const MtPlan p1 = mt_plan(n, m, b), p2 = mt_plan(m, n, b);
    return align_up((size_t)(p1.nsplit * b * n) * 8, 256) + align_up((size_t)(p2.nsplit * b * m) * 8, 256);
}

int dmcf_nn_distance(const float* xyz1, const float* xyz2, int64_t b, int64_t n, int64_t m, float* dist1, int32_t* idx1,
                     float* dist2, int32_t* idx2, void* workspace, size_t workspace_bytes, dmcf_stream_t stream) {
    if (b < 0 || n < 0 || m < 0 || b > kMtMaxGridYZ || n >= INT32_MAX || m >= INT32_MAX) return DMCF_EINVAL;
    if ((dist1 == nullptr) != (idx1 == nullptr) || (dist2 == nullptr) != (idx2 == nullptr)) return DMCF_EINVAL;
    if (dist1 == nullptr && dist2 == nullptr) return DMCF_EINVAL;
    if (b == 0) return DMCF_OK;
    if (n == 0 || m == 0) return DMCF_EINVAL;  // a point without a set to search has no nearest neighbour
    if (xyz1 == nullptr || xyz2 == nullptr || workspace == nullptr) return DMCF_EINVAL;
    if (workspace_bytes < dmcf_nn_distance_workspace_bytes(b, n, m)) return DMCF_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    for (int dir = 0; dir < 2; ++dir) {
        const float* q = dir == 0 ? xyz1 : xyz2;
        const float* r = dir == 0 ? xyz2 : xyz1;
        const int64_t nq = dir == 0 ? n : m, nr = dir == 0 ? m : n;
        float* dist = dir == 0 ? dist1 : dist2;
        int32_t* idx = dir == 0 ? idx1 : idx2;
        const MtPlan p = mt_plan(nq, nr, b);
        const size_t bytes = align_up((size_t)(p.nsplit * b * nq) * 8, 256);
        if (dist != nullptr) {
            float* pd = (float*)ws;
            int32_t* pi = (int32_t*)(pd + p.nsplit * b * nq);
            nn_partial_kernel<<<dim3((unsigned)p.row_blocks, (unsigned)p.nsplit, (unsigned)b), kMtThreads, 0, st>>>(q, nq, r, nr,
                                                                                                                   p.chunk, pd, pi);
            nn_combine_kernel<<<grid1(b * nq), kMtThreads, 0, st>>>(pd, pi, b * nq, p.nsplit, dist, idx);
        }
        ws += bytes;
    }
    return check_launch();
}

size_t dmcf_nn_distance_ragged_workspace_bytes(int64_t n_total, int64_t m_total, int64_t batch) {
    if (n_total < 0 || m_total < 0 || batch < 1 || batch > kNrMaxBatch) return 0;
    return align_up((size_t)(nr_tile_bound(n_total, batch) + nr_tile_bound(m_total, batch)) * sizeof(NrTile), 256);
}

int dmcf_nn_distance_ragged(const float* xyz1, int64_t n_total, const int64_t* row_splits1, const float* xyz2, int64_t m_total,
                            const int64_t* row_splits2, int64_t batch, float* dist1, int32_t* idx1, float* dist2, int32_t* idx2,
                            void* workspace, size_t workspace_bytes, dmcf_stream_t stream) {
    if (batch < 0 || batch > kNrMaxBatch || n_total < 0 || m_total < 0) return DMCF_EINVAL;
    if (n_total >= INT32_MAX - kNrTile || m_total >= INT32_MAX - kNrTile) return DMCF_EINVAL;  // (int32 indices)
    if ((dist1 == nullptr) != (idx1 == nullptr) || (dist2 == nullptr) != (idx2 == nullptr)) return DMCF_EINVAL;
    if (dist1 == nullptr && dist2 == nullptr) return DMCF_EINVAL;
    if (batch == 0) return n_total == 0 && m_total == 0 ? DMCF_OK : DMCF_EINVAL;
    if (row_splits1 == nullptr || row_splits2 == nullptr) return DMCF_EINVAL;
    if (!valid_row_splits(row_splits1, batch, n_total) || !valid_row_splits(row_splits2, batch, m_total)) return DMCF_EINVAL;
    for (int64_t b = 0; b < batch; ++b)  // a point without a set to search has no nearest neighbour
        if ((row_splits1[b + 1] == row_splits1[b]) != (row_splits2[b + 1] == row_splits2[b])) return DMCF_EINVAL;
    if (n_total == 0) return DMCF_OK;  // (every item empty on both sides)
    if (xyz1 == nullptr || xyz2 == nullptr || workspace == nullptr) return DMCF_EINVAL;
    if (workspace_bytes < dmcf_nn_distance_ragged_workspace_bytes(n_total, m_total, batch)) return DMCF_EWORKSPACE;
    // the tile tables of the wanted directions, one after the other, in one copy
    std::vector<NrTile> tiles;
    tiles.reserve((size_t)((dist1 != nullptr ? nr_tile_bound(n_total, batch) : 0) + (dist2 != nullptr ? nr_tile_bound(m_total, batch) : 0)));
    size_t count[2] = {0, 0};
    for (int dir = 0; dir < 2; ++dir) {
        if ((dir == 0 ? dist1 : dist2) == nullptr) continue;
        const int64_t* qs = dir == 0 ? row_splits1 : row_splits2;
        const int64_t* cs = dir == 0 ? row_splits2 : row_splits1;
        for (int64_t b = 0; b < batch; ++b)
            for (int64_t row0 = qs[b]; row0 < qs[b + 1]; row0 += kNrRows) {
                const int64_t rows = qs[b + 1] - row0 < kNrRows ? qs[b + 1] - row0 : kNrRows;
                tiles.push_back(NrTile{(int32_t)row0, (int32_t)rows, (int32_t)cs[b], (int32_t)cs[b + 1]});
            }
        count[dir] = tiles.size() - count[0] * (size_t)dir;
    }
    hipStream_t st = (hipStream_t)stream;
    // (pageable host memory: the call returns once the table has left `tiles`)
    if (hipMemcpyAsync(workspace, tiles.data(), tiles.size() * sizeof(NrTile), hipMemcpyHostToDevice, st) != hipSuccess)
        return check_launch();
    const NrTile* table = (const NrTile*)workspace;
    if (dist1 != nullptr)
        nn_ragged_kernel<<<(unsigned)count[0], kNrRows, 0, st>>>(xyz1, xyz2, table, dist1, idx1);
    if (dist2 != nullptr)
        nn_ragged_kernel<<<(unsigned)count[1], kNrRows, 0, st>>>(xyz2, xyz1, table + count[0], dist2, idx2);
    return check_launch();
}

size_t dmcf_approx_match_workspace_bytes(int64_t b, int64_t n, int64_t m) {
    if (b < 0 || n < 0 || m < 0) return 0;
    AmWork w;
    return am_carve(n, m, nullptr, &w);
}

int dmcf_approx_match(const float* xyz1, const float* xyz2, int64_t b, int64_t n, int64_t m, const int32_t* count1,
                      const int32_t* count2, float* match, void* workspace, size_t workspace_bytes, dmcf_stream_t stream) {
    if (match == nullptr) return DMCF_EINVAL;
    return approx_match_common(xyz1, xyz2, b, n, m, count1, count2, match, nullptr, workspace, workspace_bytes, stream);
}

size_t dmcf_emd_workspace_bytes(int64_t b, int64_t n, int64_t m) { return dmcf_approx_match_workspace_bytes(b, n, m); }

int dmcf_emd(const float* xyz1, const float* xyz2, int64_t b, int64_t n, int64_t m, const int32_t* count1, const int32_t* count2,
             float* cost, void* workspace, size_t workspace_bytes, dmcf_stream_t stream) {
    if (cost == nullptr) return DMCF_EINVAL;
    return approx_match_common(xyz1, xyz2, b, n, m, count1, count2, nullptr, cost, workspace, workspace_bytes, stream);
}

size_t dmcf_emd_ragged_workspace_bytes(int64_t n_total, const int64_t* row_splits1, int64_t m_total, const int64_t* row_splits2,
                                       int64_t batch) {
    if (!er_valid(n_total, row_splits1, m_total, row_splits2, batch)) return 0;
    const ErSizes z = er_sizes(row_splits1, row_splits2, batch);
    if (z.tiles_a > INT32_MAX || z.tiles_b > INT32_MAX) return 0;
    AmWork w;
    return er_carve(z, n_total, m_total, er_tables(z, batch, nullptr, nullptr), nullptr, &w);
}

int dmcf_emd_ragged(const float* xyz1, int64_t n_total, const int64_t* row_splits1, const float* xyz2, int64_t m_total,
                    const int64_t* row_splits2, int64_t batch, float* cost, void* workspace, size_t workspace_bytes,
                    dmcf_stream_t stream) {
    return emd_ragged_common(xyz1, n_total, row_splits1, xyz2, m_total, row_splits2, batch, cost, false, nullptr, workspace,
                             workspace_bytes, stream);
}

int dmcf_emd_ragged_with_levels(const float* xyz1, int64_t n_total, const int64_t* row_splits1, const float* xyz2, int64_t m_total,
                                const int64_t* row_splits2, int64_t batch, float* cost, float* levels, void* workspace,
                                size_t workspace_bytes, dmcf_stream_t stream) {
    return emd_ragged_common(xyz1, n_total, row_splits1, xyz2, m_total, row_splits2, batch, cost, true, levels, workspace,
                             workspace_bytes, stream);
}

int dmcf_emd_with_levels(const float* xyz1, const float* xyz2, int64_t b, int64_t n, int64_t m, const int32_t* count1,
                         const int32_t* count2, float* cost, float* levels, void* workspace, size_t workspace_bytes,
                         dmcf_stream_t stream) {
    if (cost == nullptr || (levels == nullptr && b > 0)) return DMCF_EINVAL;
    return approx_match_common(xyz1, xyz2, b, n, m, count1, count2, nullptr, cost, workspace, workspace_bytes, stream, levels);
}

size_t dmcf_match_cost_workspace_bytes(int64_t b, int64_t n, int64_t m) {
    if (b <= 0 || n <= 0 || m <= 0) return 0;
    const MtPlan p = mt_plan(n, m, b);
    return align_up((size_t)(p.nsplit * b * n) * sizeof(float), 256);
}

int dmcf_match_cost(const float* xyz1, const float* xyz2, int64_t b, int64_t n, int64_t m, const float* match, float* cost,
                    void* workspace, size_t workspace_bytes, dmcf_stream_t stream) {
    if (b < 0 || n < 0 || m < 0 || b > kMtMaxGridYZ || n >= INT32_MAX || m >= INT32_MAX) return DMCF_EINVAL;
    if (b == 0) return DMCF_OK;
    if (cost == nullptr) return DMCF_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (n == 0 || m == 0) {
        if (hipMemsetAsync(cost, 0, (size_t)b * sizeof(float), st) != hipSuccess) return check_launch();
        return DMCF_OK;
    }
    if (xyz1 == nullptr || xyz2 == nullptr || match == nullptr || workspace == nullptr) return DMCF_EINVAL;
    if (workspace_bytes < dmcf_match_cost_workspace_bytes(b, n, m)) return DMCF_EWORKSPACE;
    const MtPlan p = mt_plan(n, m, b);
    float* part = (float*)workspace;
    am_pass_kernel<kMtCost><<<dim3((unsigned)p.row_blocks, (unsigned)p.nsplit, (unsigned)b), kMtThreads, 0, st>>>(
        xyz1, n, n * 3, xyz2, m, m * 3, p.chunk, 0.0f, nullptr, nullptr, const_cast<float*>(match), n, n * m, part, nullptr);
    am_total_kernel<<<(unsigned)b, kMtThreads, 0, st>>>(part, n, p.nsplit, cost);
    return check_launch();
}

}  // extern "C"
