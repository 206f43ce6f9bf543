// The depth-tested sphere splat of the 3-D renderer (dmcf_amd/utils/draw_sim3d.py): every particle is a sphere impostor seen
// through a pinhole or an orthographic camera.  Pixel model, bit for bit: include/dmcf_hip.h.
//
// Kernels (one launch per call, no workspace, no memset):
//   splat_depth  per (frame, sphere): project, clip the footprint to the image, and for every covered pixel centre
//                atomicMin(keys + pixel, (bits(z) << 32) | index)  -- with DMCF_SPLAT_FARTHEST the complement of bits(z).
//                A lane walks its own footprint while that holds at most kSplatLaneMax pixels of bounding box; larger ones
//                are handed to the whole wavefront afterwards, one sphere at a time (ballot, broadcast from the owning lane,
//                the 64 lanes over consecutive pixels of the box), so a sphere that fills the image costs box / 64 steps of
//                one wave and never a serial walk on one lane.
//   splat_shade  one lane per pixel: decode up to 4 layers' keys, take the nearest (ties: the lower layer), recompute that
//                sphere's footprint terms exactly as splat_depth does, shade and composite.
// Why integer keys: min over uint64 is associative and commutative, so the key map does not depend on launch geometry or on
// arrival order, and equal depths go to the lowest index -- no float atomics, no sort.  A key only ever falls, so a plain
// load that shows a value <= the candidate proves the atomic would change nothing (a stale value is only larger): hidden
// samples, most of a dense frame, then issue no atomic.
#include <math.h>

#include "common.h"

namespace dmcf {

constexpr int kSplatMaxSide = 32768;  // W, H limit (as the disc rasterizer: pixel coordinates keep 2^-8 resolution in float)
constexpr int kSplatLaneMax = 256;    // bounding boxes of more pixels (R above some 7 px) go to the whole wavefront
constexpr int kSplatThreads = 256;
constexpr unsigned long long kSplatEmpty = ~0ull;

struct SplatView {
    float v[12];
    float focal, cx, cy, near;
    int ortho;
};

// what the pixel test of one sphere needs, and its clipped bounding box
struct SplatFoot {
    float sx, sy, R, R2, zc, m;
    int x0, y0, w, h;  // box [x0, x0 + w) x [y0, y0 + h); w * h <= 2^30
};

// the correctly rounded square root (clang lowers sqrtf to the IEEE sequence; __fsqrt_rn is the 1-ulp native form in the HIP
// headers unless OCML's basic rounded operations are enabled, and one ulp of depth breaks bit equality with the restatement)
__device__ __forceinline__ float splat_sqrt(float x) { return sqrtf(x); }

// projection of one centre (the header's operation order); false: the sphere is skipped
__device__ __forceinline__ bool splat_project(const SplatView& c, const float* __restrict__ p, float radius, float min_px, SplatFoot& s) {
    const float x = p[0], y = p[1], z = p[2];
    if (!(isfinite(x) && isfinite(y) && isfinite(z))) return false;
    const float xc = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(c.v[0], x), __fmul_rn(c.v[1], y)), __fmul_rn(c.v[2], z)), c.v[3]);
    const float yc = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(c.v[4], x), __fmul_rn(c.v[5], y)), __fmul_rn(c.v[6], z)), c.v[7]);
    const float zc = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(c.v[8], x), __fmul_rn(c.v[9], y)), __fmul_rn(c.v[10], z)), c.v[11]);
    if (!(zc > c.near)) return false;
    s.zc = zc;
    s.m = c.ortho ? c.focal : __fdiv_rn(c.focal, zc);
    s.sx = __fadd_rn(c.cx, __fmul_rn(s.m, xc));
    s.sy = __fadd_rn(c.cy, __fmul_rn(s.m, yc));
    s.R = fmaxf(__fmul_rn(s.m, radius), min_px);
    s.R2 = __fmul_rn(s.R, s.R);
    // (a value that is not finite here covers no pixel under the model: d2 < R2 fails or z is NaN)
    return isfinite(s.sx) && isfinite(s.sy) && isfinite(s.R2) && s.m > 0.0f;
}

// the clipped box of pixels whose centre can pass d2 < R2: a passing pixel has |px + 0.5 - sx| < R up to a few ulp, so
// floor(sx - R - 0.5) <= px <= ceil(sx + R - 0.5), bounds that leave up to a pixel of slack on each side against rounding errors
// that stay below 2^-8 pixel wherever they fall inside the image; false: no pixel
__device__ __forceinline__ bool splat_box(SplatFoot& s, int width, int height) {
    const float x0 = fmaxf(floorf(__fsub_rn(__fsub_rn(s.sx, s.R), 0.5f)), 0.0f);
    const float y0 = fmaxf(floorf(__fsub_rn(__fsub_rn(s.sy, s.R), 0.5f)), 0.0f);
    const float x1 = fminf(ceilf(__fsub_rn(__fadd_rn(s.sx, s.R), 0.5f)), (float)(width - 1));
    const float y1 = fminf(ceilf(__fsub_rn(__fadd_rn(s.sy, s.R), 0.5f)), (float)(height - 1));
    if (!(x0 <= x1 && y0 <= y1)) return false;
    s.x0 = (int)x0;
    s.y0 = (int)y0;
    s.w = (int)x1 - s.x0 + 1;
    s.h = (int)y1 - s.y0 + 1;
    return true;
}

// the sample of sphere s at pixel (px, py): true with its depth when the sphere covers the pixel centre in front of `near`
__device__ __forceinline__ bool splat_sample(const SplatFoot& s, float near, int px, int py, float& z, float& rest) {
    const float dx = __fsub_rn(__fadd_rn((float)px, 0.5f), s.sx), dy = __fsub_rn(__fadd_rn((float)py, 0.5f), s.sy);
    const float d2 = __fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy));
    if (!(d2 < s.R2)) return false;
    rest = splat_sqrt(__fsub_rn(s.R2, d2));
    z = __fsub_rn(s.zc, __fdiv_rn(rest, s.m));
    return isfinite(z) && z > near;
}

__device__ __forceinline__ void splat_put(unsigned long long* __restrict__ frame_keys, int width, int px, int py, float z, bool farthest,
                                          uint32_t index) {
    const uint32_t zb = __float_as_uint(z);
    const unsigned long long key = ((unsigned long long)(farthest ? ~zb : zb) << 32) | index;
    unsigned long long* at = frame_keys + (int64_t)py * width + px;
    if (key < __hip_atomic_load(at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(at, key);
}

__global__ __launch_bounds__(kSplatThreads) void splat_depth(const float* __restrict__ xyz, int64_t n, int64_t stride, int64_t total,
                                                            float radius, float min_px, const SplatView cam, int width, int height,
                                                            int farthest, unsigned long long* __restrict__ keys) {
    const int lane = lane_id();
    const int64_t step = (int64_t)gridDim.x * blockDim.x, plane = (int64_t)width * height;
    // (the trip count is the same for the 64 lanes of a wave: the cooperative part below needs all of them)
    for (int64_t k0 = (int64_t)blockIdx.x * blockDim.x + (threadIdx.x - lane); k0 < total; k0 += step) {
        const int64_t k = k0 + lane;
        SplatFoot s = {};
        bool live = false;
        int64_t f = 0;
        uint32_t index = 0;
        if (k < total) {
            f = k / n;
            const int64_t i = k - f * n;
            index = (uint32_t)i;
            live = splat_project(cam, xyz + 3 * (f * stride + i), radius, min_px, s) && splat_box(s, width, height);
        }
        const int area = live ? s.w * s.h : 0;
        const bool big = area > kSplatLaneMax;
        if (live && !big) {
            unsigned long long* fk = keys + f * plane;
            for (int py = s.y0; py < s.y0 + s.h; ++py)
                for (int px = s.x0; px < s.x0 + s.w; ++px) {
                    float z, rest;
                    if (splat_sample(s, cam.near, px, py, z, rest)) splat_put(fk, width, px, py, z, farthest != 0, index);
                }
        }
        unsigned long long todo = __ballot(big);
        while (todo) {
            const int src = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            SplatFoot b;
            b.sx = __shfl(s.sx, src);
            b.sy = __shfl(s.sy, src);
            b.R = __shfl(s.R, src);
            b.R2 = __shfl(s.R2, src);
            b.zc = __shfl(s.zc, src);
            b.m = __shfl(s.m, src);
            b.x0 = __shfl(s.x0, src);
            b.y0 = __shfl(s.y0, src);
            b.w = __shfl(s.w, src);
            b.h = __shfl(s.h, src);
            const uint32_t bindex = (uint32_t)__shfl((int)index, src);
            // (k0 + src and k0 + lane lie in one frame or in two; the frame is taken from the owning lane)
            const int64_t bf = (k0 + src) / n;
            unsigned long long* fk = keys + bf * plane;
            const uint32_t barea = (uint32_t)b.w * (uint32_t)b.h, bw = (uint32_t)b.w;
            for (uint32_t q = (uint32_t)lane; q < barea; q += kWave) {
                const uint32_t row = q / bw;
                const int px = b.x0 + (int)(q - row * bw), py = b.y0 + (int)row;
                float z, rest;
                if (splat_sample(b, cam.near, px, py, z, rest)) splat_put(fk, width, px, py, z, farthest != 0, bindex);
            }
        }
    }
}

struct SplatLayerDev {
    const unsigned long long* keys;
    const float* xyz;
    int64_t n, stride;
    float radius, a, cr, cg, cb;
    int farthest;
};

struct SplatLayers {
    SplatLayerDev l[4];
    int count;
};

__global__ __launch_bounds__(kSplatThreads) void splat_shade(const SplatLayers L, const SplatView cam, float min_px, float ambient, int width,
                                                            int height, float* __restrict__ image, float* __restrict__ depth) {
    const int64_t plane = (int64_t)width * height, p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= plane) return;
    const int64_t frame = blockIdx.y, at = frame * plane + p;
    float best = INFINITY;
    int which = -1;
    uint32_t index = 0;
    for (int j = 0; j < L.count; ++j) {
        const unsigned long long key = L.l[j].keys[at];
        if (key == kSplatEmpty) continue;
        const uint32_t hi = (uint32_t)(key >> 32), lo = (uint32_t)key;
        const float z = __uint_as_float(L.l[j].farthest ? ~hi : hi);
        // (an index past the layer's points cannot come from splat_depth on these points: such a key is treated as empty)
        if ((int64_t)lo < L.l[j].n && z < best) {
            best = z;
            which = j;
            index = lo;
        }
    }
    if (depth) depth[at] = best;
    if (which < 0) return;
    // (select, not a dynamic index into the kernel argument: the layer table stays in scalar registers)
    SplatLayerDev w = L.l[0];
    if (which == 1) w = L.l[1];
    if (which == 2) w = L.l[2];
    if (which == 3) w = L.l[3];
    SplatFoot s;
    if (!splat_project(cam, w.xyz + 3 * (frame * w.stride + index), w.radius, min_px, s)) return;
    const int py = (int)(p / width), px = (int)(p - (int64_t)py * width);
    const float dx = __fsub_rn(__fadd_rn((float)px, 0.5f), s.sx), dy = __fsub_rn(__fadd_rn((float)py, 0.5f), s.sy);
    const float d2 = __fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy));
    const float nz = __fdiv_rn(splat_sqrt(fmaxf(__fsub_rn(s.R2, d2), 0.0f)), s.R);
    const float shade = __fadd_rn(ambient, __fmul_rn(__fsub_rn(1.0f, ambient), nz));
    const float keep = __fsub_rn(1.0f, w.a);
    float* C = image + at * 3;
    C[0] = __fadd_rn(__fmul_rn(C[0], keep), __fmul_rn(__fmul_rn(w.cr, shade), w.a));
    C[1] = __fadd_rn(__fmul_rn(C[1], keep), __fmul_rn(__fmul_rn(w.cg, shade), w.a));
    C[2] = __fadd_rn(__fmul_rn(C[2], keep), __fmul_rn(__fmul_rn(w.cb, shade), w.a));
}

static int splat_view(const dmcf_camera* camera, float min_px, SplatView& v) {
    if (!camera) return DMCF_EINVAL;
    for (int i = 0; i < 12; ++i) {
        if (!__builtin_isfinite(camera->view[i])) return DMCF_EINVAL;
        v.v[i] = camera->view[i];
    }
    if (!(__builtin_isfinite(camera->focal) && camera->focal > 0.0f)) return DMCF_EINVAL;
    if (!(__builtin_isfinite(camera->cx) && __builtin_isfinite(camera->cy))) return DMCF_EINVAL;
    if (!(__builtin_isfinite(camera->near) && camera->near >= 0.0f)) return DMCF_EINVAL;  // z > near >= 0: bits(z) order as z does
    if (!(__builtin_isfinite(min_px) && min_px >= 0.0f)) return DMCF_EINVAL;
    v.focal = camera->focal;
    v.cx = camera->cx;
    v.cy = camera->cy;
    v.near = camera->near;
    v.ortho = camera->orthographic != 0;
    return DMCF_OK;
}

static int splat_sizes(int64_t n_points, int64_t n_frames, int64_t frame_stride, int32_t width, int32_t height) {
    if (n_points < 0 || n_frames < 0 || frame_stride < 0 || width <= 0 || height <= 0) return DMCF_EINVAL;
    if (width > kSplatMaxSide || height > kSplatMaxSide || n_frames > 65535) return DMCF_EINVAL;
    if (frame_stride > 0 && frame_stride < n_points) return DMCF_EINVAL;  // frames may not overlap
    if (n_points > INT32_MAX) return DMCF_EINVAL;                         // (the index is the key's low word)
    return DMCF_OK;
}

}  // namespace dmcf

using namespace dmcf;

extern "C" {

int dmcf_splat_depth(const float* xyz, int64_t n_points, int64_t n_frames, int64_t frame_stride, float radius, float min_px,
                     const dmcf_camera* camera, int32_t width, int32_t height, int32_t flags, uint64_t* keys, dmcf_stream_t stream) {
    int rc = splat_sizes(n_points, n_frames, frame_stride, width, height);
    if (rc != DMCF_OK) return rc;
    SplatView v;
    rc = splat_view(camera, min_px, v);
    if (rc != DMCF_OK) return rc;
    if (flags & ~DMCF_SPLAT_FARTHEST) return DMCF_EINVAL;
    if ((n_frames > 0 && !keys) || (n_points > 0 && n_frames > 0 && !xyz)) return DMCF_EINVAL;
    if (((uintptr_t)keys & 7) || ((uintptr_t)xyz & 3)) return DMCF_EINVAL;
    if (n_points == 0 || n_frames == 0 || !(__builtin_isfinite(radius) && radius > 0.0f)) return DMCF_OK;  // keys stay as they are
    const int64_t total = n_points * n_frames;
    const int64_t cap = (int64_t)device_cu_count() * 8, blocks = (total + kSplatThreads - 1) / kSplatThreads;
    hipLaunchKernelGGL(splat_depth, dim3((unsigned)(blocks < cap ? blocks : cap)), dim3(kSplatThreads), 0, (hipStream_t)stream, xyz,
                       n_points, frame_stride, total, radius, min_px, v, (int)width, (int)height, (int)(flags & DMCF_SPLAT_FARTHEST),
                       reinterpret_cast<unsigned long long*>(keys));
    return check_launch();
}

int dmcf_splat_shade(const dmcf_splat_layer* layers, int32_t n_layers, const dmcf_camera* camera, float min_px, float ambient,
                     int32_t width, int32_t height, int64_t n_frames, float* image, float* depth, dmcf_stream_t stream) {
    if (n_layers < 0 || n_layers > DMCF_SPLAT_MAX_LAYERS || (n_layers > 0 && !layers)) return DMCF_EINVAL;
    if (n_frames < 0 || n_frames > 65535 || width <= 0 || height <= 0 || width > kSplatMaxSide || height > kSplatMaxSide) return DMCF_EINVAL;
    SplatView v;
    int rc = splat_view(camera, min_px, v);
    if (rc != DMCF_OK) return rc;
    if (!(ambient >= 0.0f && ambient <= 1.0f)) return DMCF_EINVAL;
    if ((n_frames > 0 && !image) || (((uintptr_t)image | (uintptr_t)depth) & 3)) return DMCF_EINVAL;
    SplatLayers L;
    L.count = 0;
    for (int j = 0; j < n_layers; ++j) {
        const dmcf_splat_layer& in = layers[j];
        rc = splat_sizes(in.n_points, n_frames, in.frame_stride, width, height);
        if (rc != DMCF_OK) return rc;
        if ((in.flags & ~DMCF_SPLAT_FARTHEST) || (n_frames > 0 && !in.keys) || ((uintptr_t)in.keys & 7)) return DMCF_EINVAL;
        if ((in.n_points > 0 && n_frames > 0 && !in.xyz) || ((uintptr_t)in.xyz & 3)) return DMCF_EINVAL;
        // a layer that cannot have drawn (no points, radius not positive / finite) is left out; one with alpha 0 stays: its
        // samples still hide what lies behind them and still have a depth
        const bool drew = in.n_points > 0 && __builtin_isfinite(in.radius) && in.radius > 0.0f;
        if (!drew) continue;
        SplatLayerDev& d = L.l[L.count++];
        d.keys = reinterpret_cast<const unsigned long long*>(in.keys);
        d.xyz = in.xyz;
        d.n = in.n_points;
        d.stride = in.frame_stride;
        d.radius = in.radius;
        d.a = (float)(in.color_argb >> 24) / 255.0f;
        d.cr = (float)((in.color_argb >> 16) & 255u) / 255.0f;
        d.cg = (float)((in.color_argb >> 8) & 255u) / 255.0f;
        d.cb = (float)(in.color_argb & 255u) / 255.0f;
        d.farthest = (in.flags & DMCF_SPLAT_FARTHEST) != 0;
    }
    for (int j = L.count; j < DMCF_SPLAT_MAX_LAYERS; ++j) L.l[j] = SplatLayerDev{nullptr, nullptr, 0, 0, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0};
    if (n_frames == 0 || (L.count == 0 && !depth)) return DMCF_OK;  // the image stays as it is
    const int64_t plane = (int64_t)width * height;
    hipLaunchKernelGGL(splat_shade, dim3((unsigned)((plane + kSplatThreads - 1) / kSplatThreads), (unsigned)n_frames), dim3(kSplatThreads),
                       0, (hipStream_t)stream, L, v, min_px, ambient, (int)width, (int)height, image, depth);
    return check_launch();
}

}  // extern "C"
