// grid_pos (utils/tools/losses.py:136-181): the lattice points of every voxel corner touched by a particle, in the
// order tf.unique gives them (first appearance in the candidate list).  The reference builds the 16 N candidate cell
// indices, runs tf.unique on them and decodes; the torch form of that (sort + unique + scatter-min + argsort) costs
// ~5 ms per call at 1M particles.  Here:
//
//   bounds : centre (optional mean of the positions, deterministic two-stage double sum), extrema of floor(pos/vs -+ h)
//            -> header {minp, dims, cells} on the device; the host reads it once to size the dense cell table
//   count  : atomicMin(first[cell], k) over all candidates k = row * n_off + off (row < N: floor(s - h), row >= N:
//            floor(s + h); off in meshgrid 'ij' order); then per row the number of candidates that own their cell
//            (first[cell] == k) and an exclusive scan of those counts
//   write  : the owners, in candidate order, decoded to positions exactly as :172-179
//
// A row of the second half whose cell equals the first half's can never own a cell (same cells, larger k) and is
// skipped.  All integer work: the result is bit-identical to the sort-based formulation.
#include "common.h"

namespace dmcf {

struct GridHeader {  // 64 bytes, written by the device
    int32_t minp[3];
    int32_t dims[3];
    int64_t cells;   // dims product (0 when n == 0)
    int64_t total;   // number of lattice points (valid after count)
    float center[3];
    int32_t pad_[3];
};
static_assert(sizeof(GridHeader) == 64, "the batched entry points keep one 64-byte header per item");

struct GridParams {
    const float* pos;
    int64_t n;
    float vs[3];     // clamped voxel size
    float h[3];      // hysteresis per axis (0 on collapsed axes)
    int lo[3], len[3];  // offset range per axis: lo .. lo + len - 1
    int centralize;
    float voxel[3];  // unclamped voxel size (output scaling)
};

constexpr int kGridBlocks = 512;

__device__ __forceinline__ void grid_scaled(const GridParams& p, const GridHeader* h, int64_t i, float (&s)[3]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        float v = p.pos[3 * i + a];
        if (p.centralize) v = __fsub_rn(v, h->center[a]);
        s[a] = __fdiv_rn(v, p.vs[a]);
    }
}

// ---- items --------------------------------------------------------------------------------------------------------------------
// A call works on a BATCH of point sets (the _batched entry points, ABI 2.21): item b is positions[rs[b] .. rs[b + 1]) and the
// result is the concatenation, item after item, of what the call returns for each slice alone -- bit for bit, in the same order.
// The un-batched entry points are the case of ONE item: every kernel but the pass is instantiated twice, and ITEMS = false takes
// the item's size from n and never reads rs (NULL) -- no load.  The pass alone stays two kernels, grid_pass for one item and
// grid_pass_batched (see there).  What makes the identity so:
//   centre : blockIdx.y = item.  Each item sums over its LOCAL index with the block count a call on n_b points alone launches
//            (grid_item_blocks), so every partial sum has the same addends in the same order
//   bounds : one GridHeader per item; a cell index is local to the item's own box and offset by the cells of the items before it
//            (cell_off, the item as the outermost digit): two items at the same coordinates never share a cell
//   rows   : item b owns rows [2 rs[b], 2 rs[b + 1]): its first-half rows, then its second-half rows -- (item, half, local point).
//            The candidate rank row * n_off + off keeps an item's candidates in the relative order they have alone, and the scan
//            over the rows gives item-grouped output; out_row_splits[b] = row_off[2 rs[b]]
struct GridItems {
    const int64_t* rs;        // [batch + 1] row splits
    const int64_t* cell_off;  // [batch + 1] exclusive sum of the items' cells (grid_cell_offsets)
    int batch;
};
template <bool ITEMS>
__device__ __forceinline__ int64_t grid_item_begin(const GridItems& it, int b) { return ITEMS ? it.rs[b] : 0; }
template <bool ITEMS>
__device__ __forceinline__ int64_t grid_item_end(const GridItems& it, int b, int64_t n) { return ITEMS ? it.rs[b + 1] : n; }

// blocks of the two reductions over an item of n points (the summation order of the mean depends on it)
__host__ __device__ __forceinline__ int grid_item_blocks(int64_t n) {
    const int64_t want = (n + 255) / 256;
    return (int)(want < 1 ? 1 : (want > kGridBlocks ? kGridBlocks : want));
}

// the item that holds global point i: the last b with rs[b] <= i (empty items are stepped over)
__device__ __forceinline__ int grid_item_of(const int64_t* __restrict__ rs, int batch, int64_t i) {
    int lo = 0, hi = batch;  // invariant: rs[lo] <= i < rs[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (rs[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

// stage 1 of the mean: per-block double sums of item blockIdx.y; part[(item * gridDim.x + block) * 3 + axis].  The grid has the
// blocks of the largest possible item (all n points): the surplus blocks of a smaller one return
template <bool ITEMS>
__global__ __launch_bounds__(256) void grid_sum(const float* __restrict__ pos, int64_t n_all, const GridItems it,
                                                double* __restrict__ part) {
    const int64_t b0 = grid_item_begin<ITEMS>(it, blockIdx.y), n = grid_item_end<ITEMS>(it, blockIdx.y, n_all) - b0;
    const int nb = grid_item_blocks(n);
    if ((int)blockIdx.x >= nb) return;
    const float* __restrict__ q = pos + 3 * b0;
    double s[3] = {0.0, 0.0, 0.0};
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)nb * 256) {
        s[0] += (double)q[3 * i];
        s[1] += (double)q[3 * i + 1];
        s[2] += (double)q[3 * i + 2];
    }
    __shared__ double red[3][4];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) s[a] += __shfl_xor(s[a], d, kWave);
        if (lane_id() == 0) red[a][threadIdx.x >> 6] = s[a];
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int a = threadIdx.x;
        part[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 3 + a] = (red[a][0] + red[a][1]) + (red[a][2] + red[a][3]);
    }
}

// one wavefront per item (blockIdx.x): lane l sums the item's blocks l, l + 64, ... in rising order, the 64 partial sums meet in a
// fixed butterfly -- deterministic (a serial loop over the blocks was 54 us of dependent double adds behind dependent loads).
// given: [batch, 3] or NULL
template <bool ITEMS>
__global__ void grid_center(const double* __restrict__ part, int nbx, int64_t n_all, const GridItems it,
                            const float* __restrict__ given, GridHeader* hs) {
    const int lane = lane_id();
    GridHeader* h = hs + blockIdx.x;
    if (given) {
        if (lane < 3) h->center[lane] = given[3 * blockIdx.x + lane];
        return;
    }
    const int64_t n = grid_item_end<ITEMS>(it, blockIdx.x, n_all) - grid_item_begin<ITEMS>(it, blockIdx.x);
    const int nblocks = grid_item_blocks(n);
    part += (size_t)blockIdx.x * nbx * 3;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        double s = 0.0;
        for (int b = lane; b < nblocks; b += kWave) s += part[b * 3 + a];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, kWave);
        if (lane == 0) h->center[a] = n > 0 ? (float)(s / (double)n) : 0.0f;
    }
}

// extrema of the scaled positions of item blockIdx.y, per block (min / max: any order gives the same bits, the block count only
// has to cover the item)
template <bool ITEMS>
__global__ __launch_bounds__(256) void grid_extrema(const GridParams p, const GridHeader* hs, const GridItems it,
                                                    float* __restrict__ part) {
    const int64_t b0 = grid_item_begin<ITEMS>(it, blockIdx.y), e0 = grid_item_end<ITEMS>(it, blockIdx.y, p.n);
    const GridHeader* h = hs + blockIdx.y;
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int64_t i = b0 + (int64_t)blockIdx.x * 256 + threadIdx.x; i < e0; i += (int64_t)gridDim.x * 256) {
        float s[3];
        grid_scaled(p, h, i, s);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            // fminf / fmaxf drop NaNs: turn any non-finite coordinate into infinite extrema (reported as an error)
            const bool ok = fabsf(s[a]) < INFINITY;
            mn[a] = ok ? fminf(mn[a], s[a]) : -INFINITY;
            mx[a] = ok ? fmaxf(mx[a], s[a]) : INFINITY;
        }
    }
    __shared__ float red[2][3][4];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            mn[a] = fminf(mn[a], __shfl_xor(mn[a], d, kWave));
            mx[a] = fmaxf(mx[a], __shfl_xor(mx[a], d, kWave));
        }
        if (lane_id() == 0) {
            red[0][a][threadIdx.x >> 6] = mn[a];
            red[1][a][threadIdx.x >> 6] = mx[a];
        }
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int a = threadIdx.x;
        float* o = part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 6;
        o[a] = fminf(fminf(red[0][a][0], red[0][a][1]), fminf(red[0][a][2], red[0][a][3]));
        o[3 + a] = fmaxf(fmaxf(red[1][a][0], red[1][a][1]), fmaxf(red[1][a][2], red[1][a][3]));
    }
}

// one wavefront per item (blockIdx.x): the blocks' extrema by lanes, then a butterfly -> the item's header
template <bool ITEMS>
__global__ void grid_finish_bounds(const GridParams p, const float* __restrict__ part, int nbx, const GridItems it,
                                   GridHeader* hs) {
    const int lane = lane_id();
    GridHeader* h = hs + blockIdx.x;
    const int64_t n = grid_item_end<ITEMS>(it, blockIdx.x, p.n) - grid_item_begin<ITEMS>(it, blockIdx.x);
    part += (size_t)blockIdx.x * nbx * 6;
    float mns[3], mxs[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        float mn = INFINITY, mx = -INFINITY;
        for (int b = lane; b < nbx; b += kWave) {
            mn = fminf(mn, part[b * 6 + a]);
            mx = fmaxf(mx, part[b * 6 + 3 + a]);
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            mn = fminf(mn, __shfl_xor(mn, d, kWave));
            mx = fmaxf(mx, __shfl_xor(mx, d, kWave));
        }
        mns[a] = mn;
        mxs[a] = mx;
    }
    if (lane != 0) return;
    int64_t cells = n > 0 ? 1 : 0;
    for (int a = 0; a < 3; ++a) {
        const float mn = mns[a], mx = mxs[a];
        int lo = 0, d = 0;
        if (n > 0 && isfinite(mn) && isfinite(mx)) {
            // :167-170 -- floor is monotone: the extrema of the candidates follow from the extrema of the positions
            lo = (int)floorf(__fsub_rn(mn, p.h[a])) + p.lo[a];
            const int hi = (int)floorf(__fadd_rn(mx, p.h[a])) + p.lo[a] + p.len[a] - 1;
            d = hi - lo + 1;
        } else if (n > 0) {
            cells = -1;  // non-finite positions: the caller reports an error
        }
        h->minp[a] = lo;
        h->dims[a] = d;
        if (cells > 0) cells *= d;
    }
    h->cells = cells;
    h->total = 0;
}

// cell_off[b] = cells of the items before b (an item with non-finite positions counts as empty: the caller reports the error).
// One thread: a batch is tens of items, and this runs once per call behind the per-item wavefronts above.  (One item: base 0.)
__global__ void grid_cell_offsets(const GridHeader* __restrict__ hs, int64_t batch, int64_t* __restrict__ cell_off) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    int64_t acc = 0;
    for (int64_t b = 0; b < batch; ++b) {
        cell_off[b] = acc;
        const int64_t c = hs[b].cells;
        acc += c > 0 ? c : 0;
    }
    cell_off[batch] = acc;
}

// the two candidate base cells of particle i (relative to minp); returns whether the "+h" cell differs from the "-h" one
__device__ __forceinline__ bool grid_bases(const GridParams& p, const GridHeader* h, int64_t i, int (&c0)[3], int (&c1)[3]) {
    float s[3];
    grid_scaled(p, h, i, s);
    bool diff = false;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        c0[a] = (int)floorf(__fsub_rn(s[a], p.h[a])) - h->minp[a];
        c1[a] = (int)floorf(__fadd_rn(s[a], p.h[a])) - h->minp[a];
        diff |= c0[a] != c1[a];
    }
    return diff;
}

// A scene that has dissolved into spray (the 100k dam break after ~40 steps, the 1M box once particles leave the shell) has a
// bounding box of billions of cells for a million occupied ones: the dense table `first[cell]` does not fit.  HASHED table
// (table_cells < 0 at the entry points: -table_cells slots, a power of two): slot = open addressing on the 64-bit cell index,
// first[slot] as before, the keys behind the `first` array.  Same three passes, same owners, same order: bit-identical output
// (round 6; until then a sort-based torch formulation with six host round trips took over -- 25 ms per step of the dam break).
constexpr unsigned long long kGridEmpty = ~0ull;
__device__ __forceinline__ uint32_t grid_hash(int64_t cell, uint32_t mask) {
    return (uint32_t)(((unsigned long long)cell * 0x9E3779B97F4A7C15ull) >> 32) & mask;
}
template <bool INSERT>
__device__ __forceinline__ int64_t grid_slot(unsigned long long* keys, uint32_t mask, int64_t cell) {
    uint32_t s = grid_hash(cell, mask);
    for (uint32_t probe = 0; probe <= mask; ++probe, s = (s + 1) & mask) {
        if (INSERT) {
            const unsigned long long old = atomicCAS(keys + s, kGridEmpty, (unsigned long long)cell);
            if (old == kGridEmpty || old == (unsigned long long)cell) return s;
        } else {
            const unsigned long long k = keys[s];
            if (k == (unsigned long long)cell) return s;
            if (k == kGridEmpty) return -1;
        }
    }
    return -1;  // (table full: the caller sized it for every candidate, so this does not happen)
}

// The pass is the one step that stays two kernels, this one for one item and grid_pass_batched below: folded into one template,
// the one-item instantiation measured 0.4 us of 44 slower per call of MODE 1 on a million points and 0.4 of 50 in MODE 2
// (profiles/grid_pos_unified.md).  A fix to the candidate ranks, the hashed table or the lane-below rule goes into both.
// MODE 0: atomicMin pass; MODE 1: count owners per row; MODE 2: write owners
template <int MODE>
__global__ __launch_bounds__(256) void grid_pass(const GridParams p, const GridHeader* __restrict__ h,
                                                 uint32_t* __restrict__ first, int32_t* __restrict__ counts,
                                                 const int64_t* __restrict__ row_off, float* __restrict__ out,
                                                 int64_t out_capacity, int64_t table_cells) {
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = row < 2 * p.n;
    const bool second = row >= p.n;
    const int64_t i = live ? (second ? row - p.n : row) : 0;
    int c0[3] = {0, 0, 0}, c1[3] = {0, 0, 0};
    const bool diff = p.n > 0 && grid_bases(p, h, i, c0, c1);
    const int* c = second ? c1 : c0;
    const int64_t d0 = h->dims[0], d01 = d0 * h->dims[1];
    const bool active = live && (!second || diff);
    if (MODE == 0) {
        // A row whose base cell equals that of the row in the lane below proposes the same cells with larger ranks: it can win
        // none of them.  Particles mostly arrive in spatial order (neighbours in the array share a voxel), so this removes
        // about half of the atomics -- the same-address ones, which serialise in L2.
        const int64_t key = active ? c[0] + c[1] * d0 + c[2] * d01 : -1 - (int64_t)(threadIdx.x & 63);
        const int64_t below = __shfl_up(key, 1, 64);
        if (!active || ((threadIdx.x & 63) != 0 && below == key)) return;
    } else if (!active) {
        if (MODE == 1 && live) counts[row] = 0;
        return;
    }
    const int noff = p.len[0] * p.len[1] * p.len[2];
    const uint32_t k0 = (uint32_t)row * (uint32_t)noff;
    int cnt = 0;
    int64_t w = MODE == 2 ? row_off[row] : 0;
    int o = 0;
    for (int i0 = 0; i0 < p.len[0]; ++i0)
        for (int i1 = 0; i1 < p.len[1]; ++i1)
            for (int i2 = 0; i2 < p.len[2]; ++i2, ++o) {
                const int g0 = c[0] + p.lo[0] + i0, g1 = c[1] + p.lo[1] + i1, g2 = c[2] + p.lo[2] + i2;
                int64_t cell = g0 + g1 * d0 + g2 * d01;
                if (table_cells < 0) {
                    const uint32_t mask = (uint32_t)(-table_cells) - 1u;
                    unsigned long long* keys = (unsigned long long*)(first + (-table_cells));
                    cell = MODE == 0 ? grid_slot<true>(keys, mask, cell) : grid_slot<false>(keys, mask, cell);
                    if (cell < 0) continue;
                } else if (cell < 0 || cell >= table_cells) continue;  // table smaller than the header says: never out of bounds
                const uint32_t k = k0 + (uint32_t)o;
                if (MODE == 0) {
                    atomicMin(first + cell, k);
                } else if (first[cell] == k) {
                    if (MODE == 1) {
                        ++cnt;
                    } else if (w < out_capacity) {
                        // :172-179
                        const int g[3] = {g0 + h->minp[0], g1 + h->minp[1], g2 + h->minp[2]};
#pragma unroll
                        for (int a = 0; a < 3; ++a) {
                            const float t = __fmul_rn((float)g[a], p.voxel[a]);
                            out[3 * w + a] = p.centralize ? __fadd_rn(t, h->center[a]) : __fadd_rn(t, __fdiv_rn(p.voxel[a], 2.0f));
                        }
                        ++w;
                    }
                }
            }
    if (MODE == 1) counts[row] = cnt;
}

// grid_pass with items: row r of [0, 2 n) belongs to the item that holds point r / 2's slot (rows [2 rs[b], 2 rs[b + 1])).
// The dense table index and the hashed key are cell_off[item] + the cell index in the item's own box.
template <int MODE>
__global__ __launch_bounds__(256) void grid_pass_batched(const GridParams p, const GridHeader* __restrict__ hs,
                                                         const int64_t* __restrict__ rs, int batch,
                                                         const int64_t* __restrict__ cell_off, uint32_t* __restrict__ first,
                                                         int32_t* __restrict__ counts, const int64_t* __restrict__ row_off,
                                                         float* __restrict__ out, int64_t out_capacity, int64_t table_cells) {
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = row < 2 * p.n;
    const int item = live ? grid_item_of(rs, batch, row >> 1) : 0;
    const int64_t b0 = rs[item], nb = rs[item + 1] - b0;
    const int64_t lrow = live ? row - 2 * b0 : 0;
    const bool second = lrow >= nb;
    const int64_t i = live ? b0 + (second ? lrow - nb : lrow) : 0;
    const GridHeader* h = hs + item;
    int c0[3] = {0, 0, 0}, c1[3] = {0, 0, 0};
    const bool diff = live && grid_bases(p, h, i, c0, c1);
    const int* c = second ? c1 : c0;
    const int64_t d0 = h->dims[0], d01 = d0 * h->dims[1];
    const int64_t cells = h->cells, base = cell_off[item];
    const bool active = live && (!second || diff);
    if (MODE == 0) {
        // (see grid_pass: the row in the lane below with the same base cell -- of the same item: `base` makes the key global)
        const int64_t key = active ? base + c[0] + c[1] * d0 + c[2] * d01 : -1 - (int64_t)(threadIdx.x & 63);
        const int64_t below = __shfl_up(key, 1, 64);
        if (!active || ((threadIdx.x & 63) != 0 && below == key)) return;
    } else if (!active) {
        if (MODE == 1 && live) counts[row] = 0;
        return;
    }
    const int noff = p.len[0] * p.len[1] * p.len[2];
    const uint32_t k0 = (uint32_t)row * (uint32_t)noff;
    int cnt = 0;
    int64_t w = MODE == 2 ? row_off[row] : 0;
    int o = 0;
    for (int i0 = 0; i0 < p.len[0]; ++i0)
        for (int i1 = 0; i1 < p.len[1]; ++i1)
            for (int i2 = 0; i2 < p.len[2]; ++i2, ++o) {
                const int g0 = c[0] + p.lo[0] + i0, g1 = c[1] + p.lo[1] + i1, g2 = c[2] + p.lo[2] + i2;
                int64_t cell = g0 + g1 * d0 + g2 * d01;
                if (cell < 0 || cell >= cells) continue;  // outside the item's own box: never into another item's cells
                cell += base;
                if (table_cells < 0) {
                    const uint32_t mask = (uint32_t)(-table_cells) - 1u;
                    unsigned long long* keys = (unsigned long long*)(first + (-table_cells));
                    cell = MODE == 0 ? grid_slot<true>(keys, mask, cell) : grid_slot<false>(keys, mask, cell);
                    if (cell < 0) continue;
                } else if (cell >= table_cells) continue;  // table smaller than the headers say: never out of bounds
                const uint32_t k = k0 + (uint32_t)o;
                if (MODE == 0) {
                    atomicMin(first + cell, k);
                } else if (first[cell] == k) {
                    if (MODE == 1) {
                        ++cnt;
                    } else if (w < out_capacity) {
                        const int g[3] = {g0 + h->minp[0], g1 + h->minp[1], g2 + h->minp[2]};
#pragma unroll
                        for (int a = 0; a < 3; ++a) {
                            const float t = __fmul_rn((float)g[a], p.voxel[a]);
                            out[3 * w + a] = p.centralize ? __fadd_rn(t, h->center[a]) : __fadd_rn(t, __fdiv_rn(p.voxel[a], 2.0f));
                        }
                        ++w;
                    }
                }
            }
    if (MODE == 1) counts[row] = cnt;
}

// out_row_splits[b] = first output row of item b (b = batch: the number of lattice points; not written where NULL);
// header b's total = item b's points
template <bool ITEMS>
__global__ void grid_store_totals(const int64_t* __restrict__ row_off, int64_t n_all, const GridItems it, GridHeader* hs,
                                  int64_t* __restrict__ out_row_splits) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b > it.batch) return;
    // (b = batch is past the last item: its "begin" is the end of the call, n_all -- rs[batch] for the validated row splits the
    // header asks of the caller)
    const int64_t lo = row_off[2 * (b < it.batch ? grid_item_begin<ITEMS>(it, (int)b) : n_all)];
    if (out_row_splits) out_row_splits[b] = lo;
    if (b < it.batch) hs[b].total = row_off[2 * grid_item_end<ITEMS>(it, (int)b, n_all)] - lo;
}

constexpr int64_t kGridMaxBatch = 65535;  // the item is blockIdx.y of the two reductions

// the workspace of a call of `batch` items (the un-batched entry points: 1); header 0 is at offset 0
struct GridLayout {
    size_t off_headers, off_celloff, off_part, off_counts, off_rowoff, off_scan, total;
    int nbx;  // blocks per item of the two reductions: what the largest possible item (all n points) gets
};

static GridLayout grid_layout(int64_t n, int64_t batch) {
    GridLayout L;
    L.nbx = grid_item_blocks(n);
    size_t o = 0;
    L.off_headers = o; o += align_up((size_t)batch * sizeof(GridHeader), 256);
    L.off_celloff = o; o += align_up((size_t)(batch + 1) * 8, 256);
    L.off_part = o; o += align_up((size_t)batch * L.nbx * 6 * sizeof(double), 256);
    L.off_counts = o; o += align_up((size_t)(2 * n + 1) * 4, 256);
    L.off_rowoff = o; o += align_up((size_t)(2 * n + 2) * 8, 256);
    L.off_scan = o; o += align_up(scan_tmp_bytes(2 * n + 1), 256);
    L.total = o;
    return L;
}

static int grid_params(GridParams& p, const float* pos, int64_t n, const float* voxel, int centralize, int pad,
                       float hyst) {
    if (n < 0 || (n > 0 && !pos) || !voxel || pad < 0 || pad > 8) return DMCF_EINVAL;
    p.pos = pos;
    p.n = n;
    p.centralize = centralize ? 1 : 0;
    int64_t noff = 1;
    for (int a = 0; a < 3; ++a) {
        const bool active = voxel[a] >= 1e-5f;
        p.voxel[a] = voxel[a];
        p.vs[a] = active ? voxel[a] : 1e-5f;
        p.h[a] = active ? hyst : 0.0f;
        p.lo[a] = active ? -pad : 0;           // :151-161
        p.len[a] = active ? 2 + 2 * pad : 1;
        noff *= p.len[a];
    }
    if (2 * n * noff >= (int64_t)0xffffffffLL) return DMCF_EUNSUPPORTED;  // candidate ranks are 32-bit
    return DMCF_OK;
}

// What the three phases share: the argument checks, in the order of precedence the ABI tests pin, and the carved workspace.
// ITEMS = false is an un-batched entry point: rs = NULL, batch = 1.  bad_items / bad_args: the phase's own DMCF_EINVAL
// conditions, checked before grid_params with the row splits and after it with the workspace.
struct GridCall {
    GridParams p;
    GridLayout L;
    GridItems it;
    char* ws;
    GridHeader* hs;
};

template <bool ITEMS>
static int grid_call(GridCall& c, const float* pos, int64_t n, const int64_t* rs, int64_t batch, const float* voxel,
                     int centralize, int pad, float hyst, void* workspace, size_t workspace_bytes, bool bad_items,
                     bool bad_args) {
    if (ITEMS && (batch < 1 || !rs || bad_items)) return DMCF_EINVAL;
    const int rc = grid_params(c.p, pos, n, voxel, centralize, pad, hyst);
    if (rc != DMCF_OK) return rc;
    if (batch > kGridMaxBatch) return DMCF_EUNSUPPORTED;
    if (!workspace || ((uintptr_t)workspace & 255) || bad_args) return DMCF_EINVAL;
    c.L = grid_layout(n, batch);
    if (workspace_bytes < c.L.total) return DMCF_EWORKSPACE;
    c.ws = (char*)workspace;
    c.hs = (GridHeader*)(c.ws + c.L.off_headers);
    c.it = GridItems{rs, ITEMS ? (const int64_t*)(c.ws + c.L.off_celloff) : nullptr, (int)batch};
    return DMCF_OK;
}

// pass MODE over the 2 n rows of the call (n > 0): the one-item kernel or the items kernel
template <int MODE, bool ITEMS>
static void grid_launch_pass(const GridCall& c, uint32_t* first, int32_t* counts, const int64_t* row_off, float* out,
                             int64_t out_capacity, int64_t table_cells, hipStream_t stream) {
    const dim3 g((unsigned)((2 * c.p.n + 255) / 256));
    const GridHeader* hs = c.hs;
    if (ITEMS)
        hipLaunchKernelGGL((grid_pass_batched<MODE>), g, dim3(256), 0, stream, c.p, hs, c.it.rs, c.it.batch, c.it.cell_off, first,
                           counts, row_off, out, out_capacity, table_cells);
    else
        hipLaunchKernelGGL((grid_pass<MODE>), g, dim3(256), 0, stream, c.p, hs, first, counts, row_off, out, out_capacity,
                           table_cells);
}

template <bool ITEMS>
static int grid_bounds(const float* pos, int64_t n, const int64_t* rs, int64_t batch, const float* voxel, int centralize,
                       const float* centers, int pad, float hyst, void* workspace, size_t workspace_bytes, hipStream_t stream) {
    GridCall c;
    const int rc = grid_call<ITEMS>(c, pos, n, rs, batch, voxel, centralize, pad, hyst, workspace, workspace_bytes, false, false);
    if (rc != DMCF_OK) return rc;
    const dim3 blocks(c.L.nbx, (unsigned)batch), waves((unsigned)batch);
    if (c.p.centralize) {
        double* part = (double*)(c.ws + c.L.off_part);
        if (!centers) hipLaunchKernelGGL(grid_sum<ITEMS>, blocks, dim3(256), 0, stream, pos, n, c.it, part);
        hipLaunchKernelGGL(grid_center<ITEMS>, waves, dim3(64), 0, stream, part, c.L.nbx, n, c.it, centers, c.hs);
    }
    float* fpart = (float*)(c.ws + c.L.off_part);
    hipLaunchKernelGGL(grid_extrema<ITEMS>, blocks, dim3(256), 0, stream, c.p, c.hs, c.it, fpart);
    hipLaunchKernelGGL(grid_finish_bounds<ITEMS>, waves, dim3(64), 0, stream, c.p, fpart, c.L.nbx, c.it, c.hs);
    if (ITEMS)
        hipLaunchKernelGGL(grid_cell_offsets, dim3(1), dim3(64), 0, stream, c.hs, batch, (int64_t*)(c.ws + c.L.off_celloff));
    return check_launch();
}

template <bool ITEMS>
static int grid_count(const float* pos, int64_t n, const int64_t* rs, int64_t batch, const float* voxel, int centralize, int pad,
                      float hyst, void* workspace, size_t workspace_bytes, void* cell_table, int64_t table_cells,
                      int64_t* out_row_splits, hipStream_t stream) {
    GridCall c;
    const bool hashed_bad = table_cells < 0 && ((-table_cells) & (-table_cells - 1));  // hashed: a power of two of slots
    int rc = grid_call<ITEMS>(c, pos, n, rs, batch, voxel, centralize, pad, hyst, workspace, workspace_bytes, !out_row_splits,
                              (table_cells != 0 && !cell_table) || hashed_bad);
    if (rc != DMCF_OK) return rc;
    uint32_t* first = (uint32_t*)cell_table;
    int32_t* counts = (int32_t*)(c.ws + c.L.off_counts);
    int64_t* row_off = (int64_t*)(c.ws + c.L.off_rowoff);
    const int64_t rows = 2 * n;
    // (hashed: 4 bytes of `first` + 8 bytes of key per slot, all ones = empty)
    const size_t table_bytes = table_cells >= 0 ? (size_t)table_cells * 4 : (size_t)(-table_cells) * 12;
    if (table_bytes > 0 && hipMemsetAsync(first, 0xff, table_bytes, stream) != hipSuccess) return DMCF_ELAUNCH;
    if (rows > 0) {
        grid_launch_pass<0, ITEMS>(c, first, counts, nullptr, nullptr, 0, table_cells, stream);
        grid_launch_pass<1, ITEMS>(c, first, counts, nullptr, nullptr, 0, table_cells, stream);
    }
    rc = scan_counts_to_row_splits(counts, row_off, rows, c.ws + c.L.off_scan, c.L.total - c.L.off_scan, stream);
    if (rc != DMCF_OK) return rc;
    hipLaunchKernelGGL(grid_store_totals<ITEMS>, dim3((unsigned)((batch + 256) / 256)), dim3(256), 0, stream, row_off, n, c.it,
                       c.hs, out_row_splits);
    return check_launch();
}

template <bool ITEMS>
static int grid_write(const float* pos, int64_t n, const int64_t* rs, int64_t batch, const float* voxel, int centralize, int pad,
                      float hyst, void* workspace, size_t workspace_bytes, const void* cell_table, int64_t table_cells, float* out,
                      int64_t out_capacity, hipStream_t stream) {
    GridCall c;
    const int rc = grid_call<ITEMS>(c, pos, n, rs, batch, voxel, centralize, pad, hyst, workspace, workspace_bytes, false,
                                    out_capacity < 0 || (out_capacity > 0 && (!out || !cell_table)));
    if (rc != DMCF_OK) return rc;
    const int64_t rows = 2 * n;
    if (rows > 0 && out_capacity > 0)
        grid_launch_pass<2, ITEMS>(c, (uint32_t*)cell_table, (int32_t*)(c.ws + c.L.off_counts),
                                   (const int64_t*)(c.ws + c.L.off_rowoff), out, out_capacity, table_cells, stream);
    return check_launch();
}

}  // namespace dmcf

using namespace dmcf;

extern "C" {

size_t dmcf_grid_pos_workspace_bytes(int64_t n_points) {
    if (n_points < 0) return 0;
    return grid_layout(n_points, 1).total;
}

int dmcf_grid_pos_bounds(const float* positions, int64_t n_points, const float* voxel_size, int centralize,
                         const float* center, int pad, float hyst, void* workspace, size_t workspace_bytes,
                         dmcf_stream_t stream) {
    return grid_bounds<false>(positions, n_points, nullptr, 1, voxel_size, centralize, center, pad, hyst, workspace,
                              workspace_bytes, (hipStream_t)stream);
}

int dmcf_grid_pos_count(const float* positions, int64_t n_points, const float* voxel_size, int centralize, int pad,
                        float hyst, void* workspace, size_t workspace_bytes, void* cell_table, int64_t table_cells,
                        dmcf_stream_t stream) {
    return grid_count<false>(positions, n_points, nullptr, 1, voxel_size, centralize, pad, hyst, workspace, workspace_bytes,
                             cell_table, table_cells, nullptr, (hipStream_t)stream);
}

int dmcf_grid_pos_write(const float* positions, int64_t n_points, const float* voxel_size, int centralize, int pad,
                        float hyst, void* workspace, size_t workspace_bytes, const void* cell_table, int64_t table_cells,
                        float* out, int64_t out_capacity, dmcf_stream_t stream) {
    return grid_write<false>(positions, n_points, nullptr, 1, voxel_size, centralize, pad, hyst, workspace, workspace_bytes,
                             cell_table, table_cells, out, out_capacity, (hipStream_t)stream);
}

size_t dmcf_grid_pos_workspace_bytes_batched(int64_t n_points, int64_t batch) {
    if (n_points < 0 || batch < 1 || batch > kGridMaxBatch) return 0;
    return grid_layout(n_points, batch).total;
}

int dmcf_grid_pos_bounds_batched(const float* positions, int64_t n_points, const int64_t* row_splits, int64_t batch,
                                 const float* voxel_size, int centralize, const float* centers, int pad, float hyst,
                                 void* workspace, size_t workspace_bytes, dmcf_stream_t stream) {
    return grid_bounds<true>(positions, n_points, row_splits, batch, voxel_size, centralize, centers, pad, hyst, workspace,
                             workspace_bytes, (hipStream_t)stream);
}

int dmcf_grid_pos_count_batched(const float* positions, int64_t n_points, const int64_t* row_splits, int64_t batch,
                                const float* voxel_size, int centralize, int pad, float hyst, void* workspace,
                                size_t workspace_bytes, void* cell_table, int64_t table_cells, int64_t* out_row_splits,
                                dmcf_stream_t stream) {
    return grid_count<true>(positions, n_points, row_splits, batch, voxel_size, centralize, pad, hyst, workspace, workspace_bytes,
                            cell_table, table_cells, out_row_splits, (hipStream_t)stream);
}

int dmcf_grid_pos_write_batched(const float* positions, int64_t n_points, const int64_t* row_splits, int64_t batch,
                                const float* voxel_size, int centralize, int pad, float hyst, void* workspace,
                                size_t workspace_bytes, const void* cell_table, int64_t table_cells, float* out,
                                int64_t out_capacity, dmcf_stream_t stream) {
    return grid_write<true>(positions, n_points, row_splits, batch, voxel_size, centralize, pad, hyst, workspace, workspace_bytes,
                            cell_table, table_cells, out, out_capacity, (hipStream_t)stream);
}

}  // extern "C"
