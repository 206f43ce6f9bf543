// The velocity histograms of evaluation_helper.compare_dist for a ragged batch of scenes (ABI 2.26): per item the 5th and 95th
// percentiles of x[:, a] u y[:, a] on every axis, and the two clipped integer histograms on the grid those percentiles span.
//
// Both parts are order-independent in integers, so the results are the bits of the host function:
//   selection  an MSD radix select on order-preserving uint32 keys, 8-bit digits, four passes.  A pass is ONE launch over the
//              tiles of all items: a workgroup counts the digits of its tile in LDS ([3 axes][4 targets][256] uint32), every
//              target counting only the keys that carry its own prefix, and adds the non-zero counters to the item's global
//              [3][4][256] block with integer atomics.  A pick launch (one workgroup per item) then finds, per axis and target,
//              the digit at which the running count passes the target's remaining rank, extends the prefix, lowers the rank by
//              the keys below that digit and zeroes the block for the next pass.  Targets whose prefixes agree share the
//              counters of the first of them (rank k and k + 1 nearly always do), so ties cost nothing and are exact: both
//              ranks walk the same counts.
//   percentile numpy's _lerp in float32 (d = b - a; r = a + d g; g >= 0.5: r = b - d (1 - g)), without contraction
//              (-ffp-contract=off in the Makefile), in the last pick launch, which also zeroes the item's counts.
//   count      ONE launch over the same tiles: idx_a = clamp(trunc((v_a - min_a) / bin_w_a), 0, per) with the correctly rounded
//              division, flat = (idx_0 (per + 1) + idx_1)(per + 1) + idx_2, one global integer atomic per row.
// 4 + 4 + 1 = 9 launches, one memset (the selection state) and one table copy, whatever the batch; no host read in between.
// Inputs must be finite: NaN is not looked for (the host function returns NaN percentiles for it).
//
// LDS and occupancy: 12 KiB of counters per workgroup of 256 lanes (4 waves).  8 such workgroups fill a CU's 32 wave slots
// and take 96 of its 160 KiB, so LDS never limits occupancy; the kernels need well under 64 VGPRs.
#include <vector>

#include "common.h"
#include "metrics_plan.h"

namespace dmcf {

constexpr int kHsThreads = 256;
constexpr int kHsTileRows = DMCF_HIST_TILE_ROWS;  // rows of x (and of y) per tile
constexpr int kHsTargets = 4;                     // ranks k5, k5 + 1, k95, k95 + 1
constexpr int kHsCounters = 3 * kHsTargets * 256;  // per item and per workgroup
constexpr int kHsMaxPer = 1023;                    // (per + 1)^3 <= 2^30: flat bins fit int32
constexpr int64_t kHsMaxBatch = (int64_t)1 << 26;  // (the limit of the other ragged entry points)

struct HsTile {
    int32_t item, row0, rows, pad;  // rows [row0, row0 + rows) of the concatenated sets, 1 <= rows <= kHsTileRows
};
static_assert(sizeof(HsTile) == 16, "HsTile is read as one 16-byte load");

struct HsItem {
    int64_t off;  // the item's x counts start at counts[off], its y counts at counts[off + bins]
    int32_t bins, per;
    uint32_t rank[kHsTargets];  // 0-based ranks among the item's 2 cnt values, each < 2 cnt
    float gamma[2];
};
static_assert(sizeof(HsItem) == 40, "HsItem");

// per item: the prefix found so far and the rank among the keys that carry it, per axis and target
struct HsState {
    uint32_t prefix[3][kHsTargets];
    uint32_t rank[3][kHsTargets];
};

// order-preserving key of a finite float; -0.0 keys as +0.0 (what adding +0.0f does, whatever the denormal mode)
__device__ __forceinline__ uint32_t hs_key(float v) {
    uint32_t u = __float_as_uint(v);
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float hs_value(uint32_t key) {
    return __uint_as_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key);
}

// the first target of axis `a` that carries target t's prefix: the one that counts for t
__device__ __forceinline__ int hs_owner(const uint32_t (*prefix)[kHsTargets], int a, int t) {
    int o = t;
    for (int u = t - 1; u >= 0; --u)
        if (prefix[a][u] == prefix[a][t]) o = u;
    return o;
}

// one digit pass: shift = 24, 16, 8, 0.  `hist` [batch][3][4][256] is zero on entry (memset, then every pick launch).
__global__ __launch_bounds__(kHsThreads) void hist_digit_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                               const HsTile* __restrict__ tiles, const HsState* __restrict__ state,
                                                               int shift, uint32_t* __restrict__ hist) {
    __shared__ uint32_t cnt[kHsCounters];
    __shared__ uint32_t prefix[3][kHsTargets];
    __shared__ int counts_for[3][kHsTargets];  // 1: the target counts (no earlier target carries its prefix)
    const HsTile t = tiles[blockIdx.x];
    const int tid = (int)threadIdx.x;
    for (int i = tid; i < kHsCounters; i += kHsThreads) cnt[i] = 0;
    if (tid < 3 * kHsTargets) prefix[tid / kHsTargets][tid % kHsTargets] = shift == 24 ? 0u : state[t.item].prefix[tid / kHsTargets][tid % kHsTargets];
    __syncthreads();
    if (tid < 3 * kHsTargets) counts_for[tid / kHsTargets][tid % kHsTargets] = hs_owner(prefix, tid / kHsTargets, tid % kHsTargets) == tid % kHsTargets;
    __syncthreads();
    // the bits above the digit decide whether a key belongs to a target (none in the first pass)
    const uint32_t high = shift == 24 ? 0u : ~((1u << (shift + 8)) - 1u);
    const int64_t base = (int64_t)t.row0 * 3;
    const int n = t.rows * 3;  // the tile starts at a row, so element i lies on axis i % 3
    for (int i = tid; i < n; i += kHsThreads) {
        const int a = i % 3;
        const uint32_t kx = hs_key(x[base + i]), ky = hs_key(y[base + i]);
#pragma unroll
        for (int g = 0; g < kHsTargets; ++g) {
            if (!counts_for[a][g]) continue;
            uint32_t* c = cnt + (a * kHsTargets + g) * 256;
            if ((kx & high) == prefix[a][g]) atomicAdd(c + ((kx >> shift) & 255u), 1u);
            if ((ky & high) == prefix[a][g]) atomicAdd(c + ((ky >> shift) & 255u), 1u);
        }
    }
    __syncthreads();
    uint32_t* out = hist + (int64_t)t.item * kHsCounters;
    for (int i = tid; i < kHsCounters; i += kHsThreads) {
        const uint32_t c = cnt[i];
        if (c != 0) atomicAdd(out + i, c);
    }
}

// numpy's _lerp in float32 (the Makefile compiles without contraction)
__device__ __forceinline__ float hs_lerp(float a, float b, float g) {
    const float d = __fsub_rn(b, a);
    float r = __fadd_rn(a, __fmul_rn(d, g));
    if (g >= 0.5f) r = __fsub_rn(b, __fmul_rn(d, __fsub_rn(1.0f, g)));
    return r;
}

// one workgroup per item: wave w takes the (axis, target) pairs w, w + 4, w + 8.  kLast: the fourth pick -- the prefixes are
// the selected keys; the percentiles are written and the item's counts zeroed.
template <bool kFirst, bool kLast>
__global__ __launch_bounds__(kHsThreads) void hist_pick_kernel(const HsItem* __restrict__ items, HsState* __restrict__ state, int shift,
                                                              uint32_t* __restrict__ hist, float* __restrict__ percentiles,
                                                              int32_t* __restrict__ counts) {
    __shared__ uint32_t prefix[3][kHsTargets], rank[3][kHsTargets], next_prefix[3][kHsTargets];
    const int item = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const HsItem it = items[item];
    if (tid < 3 * kHsTargets) {
        const int a = tid / kHsTargets, g = tid % kHsTargets;
        prefix[a][g] = kFirst ? 0u : state[item].prefix[a][g];
        rank[a][g] = kFirst ? items[item].rank[g] : state[item].rank[a][g];
    }
    __syncthreads();
    uint32_t* h = hist + (int64_t)item * kHsCounters;
    for (int p = wave; p < 3 * kHsTargets; p += kHsThreads / 64) {
        const int a = p / kHsTargets, g = p % kHsTargets;
        const uint32_t* c = h + (a * kHsTargets + hs_owner(prefix, a, g)) * 256 + 4 * lane;
        const uint32_t c0 = c[0], c1 = c[1], c2 = c[2], c3 = c[3];
        const uint32_t mine = c0 + c1 + c2 + c3;
        uint32_t incl = mine;  // inclusive scan over the wave's 64 lanes
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        const uint32_t below = incl - mine, r = rank[a][g];
        if (below <= r && r < incl) {  // exactly one lane: the counts of the prefix sum to more than the rank
            uint32_t left = r - below;
            int digit = 4 * lane;
            if (left >= c0) {
                left -= c0, ++digit;
                if (left >= c1) {
                    left -= c1, ++digit;
                    if (left >= c2) left -= c2, ++digit;
                }
            }
            const uint32_t np = prefix[a][g] | ((uint32_t)digit << shift);
            next_prefix[a][g] = np;
            state[item].prefix[a][g] = np;
            state[item].rank[a][g] = left;
        }
    }
    __syncthreads();  // every counter has been read
    if (!kLast) {
        for (int i = tid; i < kHsCounters; i += kHsThreads) h[i] = 0;
        return;
    }
    if (tid < 3) {
        const float lo = hs_lerp(hs_value(next_prefix[tid][0]), hs_value(next_prefix[tid][1]), it.gamma[0]);
        const float hi = hs_lerp(hs_value(next_prefix[tid][2]), hs_value(next_prefix[tid][3]), it.gamma[1]);
        percentiles[(int64_t)item * 6 + tid] = lo;
        percentiles[(int64_t)item * 6 + 3 + tid] = hi;
    }
    for (int64_t i = tid; i < 2 * (int64_t)it.bins; i += kHsThreads) counts[it.off + i] = 0;
}

// clip(astype(int32)((v - min) / bin_w), 0, per): truncation, saturating (per <= 1023 is exact in float)
__device__ __forceinline__ int hs_bin(float v, float lo, float bin_w, int per) {
    const float q = __fdiv_rn(__fsub_rn(v, lo), bin_w);
    return q >= (float)per ? per : (q > 0.0f ? (int)q : 0);
}

__global__ __launch_bounds__(kHsThreads) void hist_count_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                               const HsTile* __restrict__ tiles, const HsItem* __restrict__ items,
                                                               const float* __restrict__ percentiles, int32_t* __restrict__ counts) {
    const HsTile t = tiles[blockIdx.x];
    const HsItem it = items[t.item];
    const int per = it.per, side = per + 1;
    float lo[3], bw[3];
    for (int a = 0; a < 3; ++a) {
        lo[a] = percentiles[(int64_t)t.item * 6 + a];
        // (max_v - min_v + 1e-6) / per in float32; per == 0 (cnt < bin_size): one bin, what the host's division by zero yields
        bw[a] = __fdiv_rn(__fadd_rn(__fsub_rn(percentiles[(int64_t)t.item * 6 + 3 + a], lo[a]), 1e-6f), (float)per);
    }
    int32_t* cx = counts + it.off;
    int32_t* cy = cx + it.bins;
    for (int r = (int)threadIdx.x; r < t.rows; r += kHsThreads) {
        const int64_t e = ((int64_t)t.row0 + r) * 3;
        int fx = 0, fy = 0;
        if (per > 0) {
            fx = (hs_bin(x[e], lo[0], bw[0], per) * side + hs_bin(x[e + 1], lo[1], bw[1], per)) * side + hs_bin(x[e + 2], lo[2], bw[2], per);
            fy = (hs_bin(y[e], lo[0], bw[0], per) * side + hs_bin(y[e + 1], lo[1], bw[1], per)) * side + hs_bin(y[e + 2], lo[2], bw[2], per);
        }
        atomicAdd(cx + fx, 1);
        atomicAdd(cy + fy, 1);
    }
}

inline int64_t hs_tile_bound(int64_t rows, int64_t batch) { return rows / kHsTileRows + batch; }  // every item adds <= 1 partial tile

// the workspace: [state | digit counters] (one memset), then [items | tiles] (one copy)
struct HsWork {
    HsState* state;
    uint32_t* hist;
    size_t zero_bytes;
    char* table;
    size_t items_bytes, table_bytes;
};
inline size_t hs_carve(int64_t n_total, int64_t batch, char* base, HsWork* w) {
    size_t off = 0;
    w->state = (HsState*)(base + off);
    off += align_up((size_t)batch * sizeof(HsState), 256);
    w->hist = (uint32_t*)(base + off);
    off += align_up((size_t)batch * kHsCounters * sizeof(uint32_t), 256);
    w->zero_bytes = off;
    w->table = base + off;
    w->items_bytes = align_up((size_t)batch * sizeof(HsItem), 256);
    w->table_bytes = w->items_bytes + align_up((size_t)hs_tile_bound(n_total, batch) * sizeof(HsTile), 256);
    return off + w->table_bytes;
}

inline bool hs_sizes_valid(int64_t n_total, int64_t batch, int64_t bins_total) {
    if (batch < 1 || batch > kHsMaxBatch || n_total < batch || n_total >= INT32_MAX - 256) return false;
    return bins_total >= batch && bins_total <= (INT32_MAX >> 1);  // (every item has at least one bin; 2 bins_total fits int32)
}

}  // namespace dmcf

using namespace dmcf;

extern "C" {

size_t dmcf_hist_pair_ragged_workspace_bytes(int64_t n_total, int64_t batch, int64_t bins_total) {
    if (!hs_sizes_valid(n_total, batch, bins_total)) return 0;
    HsWork w;
    return hs_carve(n_total, batch, nullptr, &w);
}

int dmcf_hist_pair_ragged(const float* x, const float* y, int64_t n_total, const int64_t* row_splits, int64_t batch,
                          const dmcf_hist_plan* plan, int64_t bins_total, float* percentiles, int32_t* counts, void* workspace,
                          size_t workspace_bytes, dmcf_stream_t stream) {
    if (!hs_sizes_valid(n_total, batch, bins_total)) return DMCF_EINVAL;
    if (row_splits == nullptr || plan == nullptr || !valid_row_splits(row_splits, batch, n_total)) return DMCF_EINVAL;
    int64_t bins = 0;
    for (int64_t b = 0; b < batch; ++b) {
        const int64_t cnt = row_splits[b + 1] - row_splits[b];
        const dmcf_hist_plan& p = plan[b];
        if (cnt < 1 || p.per < 0 || p.per > kHsMaxPer) return DMCF_EINVAL;
        for (int g = 0; g < kHsTargets; ++g)
            if (p.rank[g] < 0 || p.rank[g] >= 2 * cnt) return DMCF_EINVAL;
        if (!(p.gamma[0] >= 0.0f && p.gamma[0] <= 1.0f && p.gamma[1] >= 0.0f && p.gamma[1] <= 1.0f)) return DMCF_EINVAL;
        bins += (int64_t)(p.per + 1) * (p.per + 1) * (p.per + 1);
        if (bins > bins_total) return DMCF_EINVAL;
    }
    if (bins != bins_total) return DMCF_EINVAL;
    if (x == nullptr || y == nullptr || percentiles == nullptr || counts == nullptr || workspace == nullptr) return DMCF_EINVAL;
    HsWork w;
    if (workspace_bytes < hs_carve(n_total, batch, (char*)workspace, &w)) return DMCF_EWORKSPACE;
    std::vector<char> table(w.table_bytes);
    HsItem* items = (HsItem*)table.data();
    HsTile* tiles = (HsTile*)(table.data() + w.items_bytes);
    int64_t ntiles = 0, off = 0;
    for (int64_t b = 0; b < batch; ++b) {
        const dmcf_hist_plan& p = plan[b];
        const int64_t nb = (int64_t)(p.per + 1) * (p.per + 1) * (p.per + 1);
        HsItem& it = items[b];
        it.off = off;
        it.bins = (int32_t)nb;
        it.per = p.per;
        for (int g = 0; g < kHsTargets; ++g) it.rank[g] = (uint32_t)p.rank[g];
        it.gamma[0] = p.gamma[0];
        it.gamma[1] = p.gamma[1];
        off += 2 * nb;
        for (int64_t row0 = row_splits[b]; row0 < row_splits[b + 1]; row0 += kHsTileRows) {
            const int64_t rows = row_splits[b + 1] - row0 < kHsTileRows ? row_splits[b + 1] - row0 : kHsTileRows;
            tiles[ntiles++] = HsTile{(int32_t)b, (int32_t)row0, (int32_t)rows, 0};
        }
    }
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(workspace, 0, w.zero_bytes, st) != hipSuccess) return check_launch();
    // (pageable host memory: the call returns once the table has left `table`)
    if (hipMemcpyAsync(w.table, table.data(), w.items_bytes + (size_t)ntiles * sizeof(HsTile), hipMemcpyHostToDevice, st) != hipSuccess)
        return check_launch();
    const HsItem* d_items = (const HsItem*)w.table;
    const HsTile* d_tiles = (const HsTile*)(w.table + w.items_bytes);
    const unsigned gt = (unsigned)ntiles, gb = (unsigned)batch;
    // every pick follows its digit pass on the stream: no launch reads what an unfinished one writes
    hist_digit_kernel<<<gt, kHsThreads, 0, st>>>(x, y, d_tiles, w.state, 24, w.hist);
    hist_pick_kernel<true, false><<<gb, kHsThreads, 0, st>>>(d_items, w.state, 24, w.hist, percentiles, counts);
    for (int shift = 16; shift >= 8; shift -= 8) {
        hist_digit_kernel<<<gt, kHsThreads, 0, st>>>(x, y, d_tiles, w.state, shift, w.hist);
        hist_pick_kernel<false, false><<<gb, kHsThreads, 0, st>>>(d_items, w.state, shift, w.hist, percentiles, counts);
    }
    hist_digit_kernel<<<gt, kHsThreads, 0, st>>>(x, y, d_tiles, w.state, 0, w.hist);
    hist_pick_kernel<false, true><<<gb, kHsThreads, 0, st>>>(d_items, w.state, 0, w.hist, percentiles, counts);
    hist_count_kernel<<<gt, kHsThreads, 0, st>>>(x, y, d_tiles, d_items, percentiles, counts);
    return check_launch();
}

}  // extern "C"
