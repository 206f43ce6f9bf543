// Split plan of the all-pairs metric passes (metrics.hip) and their gradients (metrics_bwd.hip): a workgroup holds 256 rows,
// one per lane, and walks one contiguous chunk of the other set through LDS in tiles of 256 points.
#pragma once
#include <math.h>
#include <stdint.h>

namespace dmcf {

constexpr int kMtThreads = 256;         // rows per workgroup, one per lane
constexpr int kMtTile = 256;            // points of the other set per LDS tile
constexpr int64_t kMtTargetBlocks = 2048;  // split the columns until rows x splits reaches this many workgroups
constexpr int kMtMaxGridYZ = 65535;

struct MtPlan {
    int64_t row_blocks, nsplit, chunk;
};

// columns split into nsplit chunks of whole tiles; depends on (rows, cols, batch) only
inline MtPlan mt_plan(int64_t rows, int64_t cols, int64_t batch = 1) {
    MtPlan p;
    p.row_blocks = (rows + kMtThreads - 1) / kMtThreads;
    const int64_t tiles = cols > 0 ? (cols + kMtTile - 1) / kMtTile : 1;
    const int64_t want = (kMtTargetBlocks + p.row_blocks * batch - 1) / (p.row_blocks * batch);
    int64_t ns = want < tiles ? want : tiles;
    if (ns < 1) ns = 1;
    const int64_t per = (tiles + ns - 1) / ns;
    p.nsplit = (tiles + per - 1) / per;
    p.chunk = per * kMtTile;
    return p;
}

// upper bound of nsplit * rows over every rows <= rows_max, cols <= cols_max (batch 1): the workspace of the passes
inline int64_t mt_partial_bound(int64_t rows_max, int64_t cols_max) {
    const int64_t tiles = cols_max > 0 ? (cols_max + kMtTile - 1) / kMtTile : 1;
    const int64_t a = tiles * rows_max;
    const int64_t b = kMtTargetBlocks * kMtThreads + rows_max + kMtThreads;
    return a < b ? a : b;
}

// approximate match: ten levels, level L = -4^(7 - L) for L < 9 and 0 for the last (the order of the passes)
constexpr int kAmLevels = 10;
inline float am_level(int L) {
    const int j = 7 - L;
    return j == -2 ? 0.0f : -powf(4.0f, (float)j);
}

// host counts of the batch items (NULL = all): every one in [0, limit] (metrics.hip)
bool valid_counts(const int32_t* counts, int64_t b, int64_t limit);

// host row splits of `batch` items over `total` rows: start at 0, do not decrease, end at total (metrics.hip)
bool valid_row_splits(const int64_t* rs, int64_t batch, int64_t total);

// the argument checks of the ragged EMD entry points and their workspace queries: 1 <= batch <= 2^26, totals that leave room
// for int32 indices, HOST row splits that start at 0, do not decrease and end at the totals (metrics.hip)
bool er_valid(int64_t n_total, const int64_t* rs1, int64_t m_total, const int64_t* rs2, int64_t batch);

}  // namespace dmcf
