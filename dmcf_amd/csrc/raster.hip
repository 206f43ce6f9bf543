// The disc rasterizer of the renderer (dmcf_amd/utils/draw_sim2d.py): filled, anti-aliased discs of one colour drawn into a
// batch of F frames of W x H float RGB pixels, composited over what the image holds -- the reference's per-particle
// canvas.drawCircle loop (utils/draw_sim2d.py:29-43) as one data-parallel pass per point group.  Pixel model: include/dmcf_hip.h.
//
// Kernels (the count call: a memset, raster_count and the scan; the raster call: a memset, raster_fill and raster_tiles):
//   raster_count  per (source frame, disc): the 16 x 16 tiles the disc's support reaches, integer-counted per bin
//                 (bin = source frame x tile; a frame stride of 0 has one source frame, binned once for all F frames)
//   (scan)        the bin counts -> int64 bin offsets (misc.hip's scan), the last one the total the caller reads
//   raster_fill   the same walk again: each (disc, tile) pair writes the disc's float2 centre into its bin at an
//                 integer-atomic cursor; the order inside a bin is therefore arbitrary
//   raster_tiles  one 256-lane workgroup per (frame, tile), one lane per pixel: the bin is staged through LDS in chunks of
//                 256 centres (every lane then reads the same address: broadcast) and each lane sums log(1 - a cov) of
//                 its pixel in 2^-32 fixed point
// Why fixed point: a sum of int64 terms is exactly associative, so the transmittance T = exp(sum) is the same bits whatever
// order the fill left the bin in and whatever the launch geometry -- no sort of the bins, and no float atomics anywhere.
// Every term is <= 0 and the running sum is clamped at kRasterFloor, which is order independent as well (the partial sums of
// non-positive terms only fall).
#include <math.h>

#include "common.h"

namespace dmcf {

constexpr int kRasterTile = 16;                     // tile edge in pixels: one lane per pixel of a 256-lane workgroup
constexpr int kRasterThreads = kRasterTile * kRasterTile;
constexpr int kRasterMaxSide = 32768;               // W, H limit: pixel coordinates stay where float has 2^-8 resolution
constexpr float kRasterFix = 4294967296.0f;         // 2^32: fixed-point scale of the log transmittance
constexpr float kRasterTermMin = -128.0f;           // one disc's log factor (log 0 = -inf for a = cov = 1)
constexpr long long kRasterFloor = -(1LL << 62);    // clamp of the running sum; exp(-2^30) is 0 in float
constexpr float kRasterSlack = 0.25f;               // binning margin in pixels beyond the support (covers float rounding)

typedef float raster_f32x2 __attribute__((ext_vector_type(2)));

struct RasterGeom {
    int64_t n, stride;   // points per frame, points between frames (0: the same points in every frame)
    int src_frames;      // frames that are binned (1 when stride == 0)
    int width, height, tiles_x, tiles_y;
    float reach;         // r + 0.5 + kRasterSlack: pixel centres closer than r + 0.5 can be covered
};

// the tile rectangle [tx0, tx1] x [ty0, ty1] a disc with centre (cx, cy) can touch; false when it touches none
__device__ __forceinline__ bool raster_tile_range(const RasterGeom& g, float cx, float cy, int& tx0, int& tx1, int& ty0, int& ty1) {
    if (!(isfinite(cx) && isfinite(cy))) return false;
    // pixel i (centre i + 0.5) is a candidate when |i + 0.5 - c| < reach
    const float x0 = floorf(__fsub_rn(__fsub_rn(cx, g.reach), 0.5f)), x1 = floorf(__fsub_rn(__fadd_rn(cx, g.reach), 0.5f));
    const float y0 = floorf(__fsub_rn(__fsub_rn(cy, g.reach), 0.5f)), y1 = floorf(__fsub_rn(__fadd_rn(cy, g.reach), 0.5f));
    if (x1 < 0.0f || y1 < 0.0f || x0 > (float)(g.width - 1) || y0 > (float)(g.height - 1)) return false;
    tx0 = (int)fmaxf(x0, 0.0f) / kRasterTile;
    tx1 = (int)fminf(x1, (float)(g.width - 1)) / kRasterTile;
    ty0 = (int)fmaxf(y0, 0.0f) / kRasterTile;
    ty1 = (int)fminf(y1, (float)(g.height - 1)) / kRasterTile;
    return true;
}

__global__ __launch_bounds__(256) void raster_count(const float* __restrict__ xy, const RasterGeom g, int32_t* __restrict__ bin_count) {
    const int64_t total = g.n * g.src_frames, tiles = (int64_t)g.tiles_x * g.tiles_y;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < total; k += (int64_t)gridDim.x * blockDim.x) {
        const int64_t f = k / g.n, i = k - f * g.n;
        const raster_f32x2 c = *reinterpret_cast<const raster_f32x2*>(xy + 2 * (f * g.stride + i));
        int tx0, tx1, ty0, ty1;
        if (!raster_tile_range(g, c.x, c.y, tx0, tx1, ty0, ty1)) continue;
        for (int ty = ty0; ty <= ty1; ++ty)
            for (int tx = tx0; tx <= tx1; ++tx) atomicAdd(bin_count + f * tiles + (int64_t)ty * g.tiles_x + tx, 1);
    }
}

__global__ __launch_bounds__(256) void raster_fill(const float* __restrict__ xy, const RasterGeom g, const int64_t* __restrict__ bin_begin,
                                                   int32_t* __restrict__ cursor, raster_f32x2* __restrict__ bins, int64_t capacity) {
    const int64_t total = g.n * g.src_frames, tiles = (int64_t)g.tiles_x * g.tiles_y;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < total; k += (int64_t)gridDim.x * blockDim.x) {
        const int64_t f = k / g.n, i = k - f * g.n;
        const raster_f32x2 c = *reinterpret_cast<const raster_f32x2*>(xy + 2 * (f * g.stride + i));
        int tx0, tx1, ty0, ty1;
        if (!raster_tile_range(g, c.x, c.y, tx0, tx1, ty0, ty1)) continue;
        for (int ty = ty0; ty <= ty1; ++ty)
            for (int tx = tx0; tx <= tx1; ++tx) {
                const int64_t b = f * tiles + (int64_t)ty * g.tiles_x + tx;
                const int64_t at = bin_begin[b] + atomicAdd(cursor + b, 1);
                if (at < capacity) bins[at] = c;  // (a caller's short buffer loses entries, never writes past its end)
            }
    }
}

struct RasterShade {
    float r, R2, R, k;       // radius, (r + 0.5)^2, r + 0.5, min(1, 2 r)
    float a;                 // alpha / 255
    float cr, cg, cb;        // colour / 255
};

__global__ __launch_bounds__(kRasterThreads) void raster_tiles(const RasterGeom g, const RasterShade s, const int64_t* __restrict__ bin_begin,
                                                              const raster_f32x2* __restrict__ bins, int64_t capacity, float* __restrict__ image) {
    __shared__ raster_f32x2 stage[kRasterThreads];
    const int tile = blockIdx.x, frame = blockIdx.y;
    const int ty = tile / g.tiles_x, tx = tile - ty * g.tiles_x;
    const int px = tx * kRasterTile + (threadIdx.x & (kRasterTile - 1)), py = ty * kRasterTile + (threadIdx.x / kRasterTile);
    const float fx = (float)px + 0.5f, fy = (float)py + 0.5f;
    const int64_t b = (g.src_frames == 1 ? 0 : (int64_t)frame) * ((int64_t)g.tiles_x * g.tiles_y) + tile;
    const int64_t begin = bin_begin[b];
    int64_t end = bin_begin[b + 1];
    end = end < capacity ? end : capacity;
    long long acc = 0;
    for (int64_t base = begin; base < end; base += kRasterThreads) {
        const int64_t m64 = end - base;
        const int m = m64 < kRasterThreads ? (int)m64 : kRasterThreads;
        if ((int)threadIdx.x < m) stage[threadIdx.x] = bins[base + threadIdx.x];
        __syncthreads();
        for (int j = 0; j < m; ++j) {
            const raster_f32x2 c = stage[j];
            const float dx = __fsub_rn(fx, c.x), dy = __fsub_rn(fy, c.y);
            const float d2 = __fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy));
            if (d2 < s.R2) {
                const float cov = __fmul_rn(fminf(__fsub_rn(s.R, __fsqrt_rn(d2)), 1.0f), s.k);
                if (cov > 0.0f) {
                    const float t = fmaxf(log1pf(-__fmul_rn(s.a, cov)), kRasterTermMin);
                    acc += __float2ll_rn(__fmul_rn(t, kRasterFix));
                    acc = acc > kRasterFloor ? acc : kRasterFloor;
                }
            }
        }
        __syncthreads();
    }
    if (px >= g.width || py >= g.height || acc == 0) return;
    const float T = expf((float)((double)acc * 0x1p-32));
    const float u = __fsub_rn(1.0f, T);
    float* C = image + (((int64_t)frame * g.height + py) * g.width + px) * 3;
    C[0] = __fadd_rn(__fmul_rn(C[0], T), __fmul_rn(s.cr, u));
    C[1] = __fadd_rn(__fmul_rn(C[1], T), __fmul_rn(s.cg, u));
    C[2] = __fadd_rn(__fmul_rn(C[2], T), __fmul_rn(s.cb, u));
}

struct RasterPlan {
    RasterGeom g;
    int64_t bins;            // source frames x tiles
    size_t off_begin, off_cursor, off_tmp, ws_bytes;
    bool draws;              // false: nothing can be drawn (no points, no frames, r not positive / finite)
};

static int raster_plan(int64_t n_points, int64_t n_frames, int64_t frame_stride, float radius, int32_t width, int32_t height,
                       RasterPlan& p) {
    if (n_points < 0 || n_frames < 0 || frame_stride < 0 || width <= 0 || height <= 0) return DMCF_EINVAL;
    if (width > kRasterMaxSide || height > kRasterMaxSide || n_frames > 65535) return DMCF_EINVAL;
    if (frame_stride > 0 && frame_stride < n_points) return DMCF_EINVAL;  // frames may not overlap
    const int src = frame_stride == 0 ? (n_frames > 0 ? 1 : 0) : (int)n_frames;
    if (n_points > INT32_MAX) return DMCF_EINVAL;  // (int32 bin counts and cursors: a bin holds each disc at most once)
    p.g.n = n_points;
    p.g.stride = frame_stride;
    p.g.src_frames = src;
    p.g.width = width;
    p.g.height = height;
    p.g.tiles_x = (width + kRasterTile - 1) / kRasterTile;
    p.g.tiles_y = (height + kRasterTile - 1) / kRasterTile;
    p.g.reach = __builtin_isfinite(radius) ? radius + 0.5f + kRasterSlack : 0.0f;
    p.draws = n_points > 0 && n_frames > 0 && __builtin_isfinite(radius) && radius > 0.0f;
    p.bins = (int64_t)src * p.g.tiles_x * p.g.tiles_y;
    p.off_begin = align_up(sizeof(int32_t) * (size_t)p.bins, 256);       // counts | begin (bins + 1) | cursor | scan tmp
    p.off_cursor = p.off_begin + align_up(sizeof(int64_t) * (size_t)(p.bins + 1), 256);
    p.off_tmp = p.off_cursor + align_up(sizeof(int32_t) * (size_t)p.bins, 256);
    p.ws_bytes = p.off_tmp + scan_tmp_bytes(p.bins);
    return DMCF_OK;
}

static unsigned raster_grid(int64_t work) {
    const int64_t cap = (int64_t)device_cu_count() * 8, blocks = (work + 255) / 256;
    return (unsigned)(blocks < cap ? (blocks > 0 ? blocks : 1) : cap);
}

}  // namespace dmcf

using namespace dmcf;

extern "C" {

size_t dmcf_raster_workspace_bytes(int64_t n_points, int64_t n_frames, int64_t frame_stride, int32_t width, int32_t height) {
    RasterPlan p;
    if (raster_plan(n_points, n_frames, frame_stride, 1.0f, width, height, p) != DMCF_OK) return 0;
    return p.ws_bytes;
}

int dmcf_raster_count(const float* xy, int64_t n_points, int64_t n_frames, int64_t frame_stride, float radius, int32_t width,
                      int32_t height, void* workspace, size_t workspace_bytes, int64_t* total, dmcf_stream_t stream) {
    RasterPlan p;
    int rc = raster_plan(n_points, n_frames, frame_stride, radius, width, height, p);
    if (rc != DMCF_OK) return rc;
    if (!total || !workspace || (n_points > 0 && n_frames > 0 && !xy) || ((uintptr_t)xy & 7)) return DMCF_EINVAL;
    if (workspace_bytes < p.ws_bytes) return DMCF_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    int32_t* counts = (int32_t*)ws;
    int64_t* begin = (int64_t*)(ws + p.off_begin);
    if (p.bins > 0 && hipMemsetAsync(counts, 0, sizeof(int32_t) * (size_t)p.bins, st) != hipSuccess) return DMCF_ELAUNCH;
    if (p.draws) {
        hipLaunchKernelGGL(raster_count, dim3(raster_grid(n_points * p.g.src_frames)), dim3(256), 0, st, xy, p.g, counts);
        rc = check_launch();
        if (rc != DMCF_OK) return rc;
    }
    rc = scan_counts_to_row_splits(counts, begin, p.bins, ws + p.off_tmp, workspace_bytes - p.off_tmp, st);
    if (rc != DMCF_OK) return rc;
    if (hipMemcpyAsync(total, begin + p.bins, sizeof(int64_t), hipMemcpyDeviceToDevice, st) != hipSuccess) return DMCF_ELAUNCH;
    return DMCF_OK;
}

int dmcf_raster_discs(const float* xy, int64_t n_points, int64_t n_frames, int64_t frame_stride, float radius, uint32_t color_argb,
                      int32_t width, int32_t height, float* image, void* workspace, size_t workspace_bytes, float* bins,
                      int64_t bin_capacity, dmcf_stream_t stream) {
    RasterPlan p;
    int rc = raster_plan(n_points, n_frames, frame_stride, radius, width, height, p);
    if (rc != DMCF_OK) return rc;
    if (bin_capacity < 0 || !workspace || (n_frames > 0 && !image) || (n_points > 0 && n_frames > 0 && !xy)) return DMCF_EINVAL;
    if ((bin_capacity > 0 && !bins) || (((uintptr_t)xy | (uintptr_t)bins) & 7)) return DMCF_EINVAL;  // (float2 accesses)
    if (workspace_bytes < p.ws_bytes) return DMCF_EWORKSPACE;
    const uint32_t alpha = color_argb >> 24;
    if (!p.draws || alpha == 0) return DMCF_OK;  // nothing is drawn: the image stays as it is
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    const int64_t* begin = (const int64_t*)(ws + p.off_begin);
    int32_t* cursor = (int32_t*)(ws + p.off_cursor);
    if (hipMemsetAsync(cursor, 0, sizeof(int32_t) * (size_t)p.bins, st) != hipSuccess) return DMCF_ELAUNCH;
    raster_f32x2* b2 = reinterpret_cast<raster_f32x2*>(bins);
    hipLaunchKernelGGL(raster_fill, dim3(raster_grid(n_points * p.g.src_frames)), dim3(256), 0, st, xy, p.g, begin, cursor, b2,
                       bin_capacity);
    rc = check_launch();
    if (rc != DMCF_OK) return rc;
    RasterShade s;
    s.r = radius;
    s.R = radius + 0.5f;
    s.R2 = s.R * s.R;
    s.k = fminf(1.0f, 2.0f * radius);
    s.a = (float)alpha / 255.0f;
    s.cr = (float)((color_argb >> 16) & 255u) / 255.0f;
    s.cg = (float)((color_argb >> 8) & 255u) / 255.0f;
    s.cb = (float)(color_argb & 255u) / 255.0f;
    hipLaunchKernelGGL(raster_tiles, dim3((unsigned)(p.g.tiles_x * p.g.tiles_y), (unsigned)n_frames), dim3(kRasterThreads), 0, st,
                       p.g, s, begin, (const raster_f32x2*)b2, bin_capacity, image);
    return check_launch();
}

}  // extern "C"
