// Continuous convolution (CConv) and antisymmetric CConv (ASCC) for gfx950.
//
// Replaces ml3d.ops.continuous_conv as called from the reference at utils/convolutions.py:414-431 and
// the ASCC body utils/convolutions.py:410-412,433-458 (see include/dmcf_hip.h for the contract).
//
// Formulation (same factorisation as the Open3D CPU code, which is what makes the op cheap):
//   B_i[k,c] = sum_{j in N(i)} a_ij * w_k(Lambda(x_j - x_i)) * f_j[c]        (gather + trilinear splat)
//   out_i[o] = sum_{k,c} B_i[k,c] * W[k,c,o]                                  (dense contraction)
//
// MI355X mapping (one workgroup = 8 wavefronts = a tile of 16 consecutive output points, two
// workgroups per CU so that one tile's LDS-bound splat overlaps the other's MFMA-bound contraction):
//   * B of the tile lives in LDS as [16][K*CC+4] floats, channel-chunked by CC (8, or 4 for Cin <= 4).
//   * splat, phase 1 -- ONE LANE PER NEIGHBOUR, 64 at a time: index, distance, position and the CC
//     feature floats of the neighbour are gathered with independent (batched) loads, the window
//     function and the ball->cube mapping (sqrt, atan, divisions) are evaluated once per pair at full
//     lane utilisation, and the 8 trilinear corner weights plus the importance-scaled features are
//     parked in a per-wave LDS staging area.
//   * splat, phase 2 -- lanes re-mapped to (corner, channel): per pair one v_readlane (base cell), two
//     LDS reads (corner weight, feature), one multiply and one ds_add_f32 into B.  A pair's 8 corners
//     are 8 distinct cells and a point's row of B belongs to one wave, so the adds never collide.
//   * contraction on the matrix cores in exact fp32: v_mfma_f32_16x16x4_f32, M = the 16 points,
//     N = 16 output channels per tile, K = the K*CC splat entries of the chunk split over the 8
//     waves; A fragments come from B with ds_read_b128, the filter is pre-packed (pack_filter) into
//     the B-fragment order so each lane fetches its 4 values with one coalesced 16-byte load from L2.
//     Accumulators stay in registers across channel chunks; the 8 partial tiles are reduced through
//     LDS, then normalisation, bias and the add_merge accumulation are applied in the store.
//   * ASCC is the same kernel with pair features (f_j + f_i) and the mirrored kernel, i.e. the fused
//     single-pass form of the reference's two continuous_conv calls + batched matmul.
//   * consecutive tiles go to the same XCD (blockIdx swizzle) so neighbouring outputs share one L2.
//   * individual extents (continuous_conv with extents [n_out, 1], dmcf_cconv_forward_extents): the same kernel with the extent
//     of each output row read once per row (cconv_ext_kernel; the body is cconv_generic_body.inc).
#include <type_traits>

#include <stdio.h>

#include "cconv_common.h"

namespace dmcf {

constexpr int kThreads = 512;
constexpr int kWaves = kThreads / 64;
constexpr int TM = 16;           // output points per workgroup (MFMA M)
constexpr int kMaxNT = 4;        // N tiles of 16 output channels (Cout <= 64)
constexpr int kWStride = 8;      // staged corner weights per pair
constexpr int kFStride = 8;      // staged features per pair
constexpr int kStage = 64 * (kWStride + kFStride + 1);  // floats per wave: weights, features, base offset per pair

// Layout of one row of B (floats): [z plane][y row][x cell][channel].  z planes are padded to "PS" floats so
// that the +z corners of a pair fall on other LDS banks than the -z corners (make_cfg picks the padding with a
// small bank model).  A rotation of odd y rows that also separates the +-y corners in the 32-bank write
// model was tried and removed: the extra v_readlane / bit-field work in the splat loop, which is co-limited
// by instruction issue and the LDS pipe, cost more (+48 % kernel time) than the conflicts it removed.

template <int CC, bool GENERIC>
__global__ __launch_bounds__(kThreads, 4) void cconv_kernel(const CconvParams p) {
    constexpr bool EXT = false;
    const float* const out_ext = nullptr;
#include "cconv_generic_body.inc"
}

// individual extents (dmcf_cconv_forward_extents): the generic kernel with the extent of each output row read from out_ext
template <int CC>
__global__ __launch_bounds__(kThreads, 4) void cconv_ext_kernel(const CconvParams p, const float* __restrict__ out_ext) {
    constexpr bool GENERIC = true, EXT = true;
#include "cconv_generic_body.inc"
}

// Packs [K][cin][cout] (optionally mirrored: ASCC, utils/convolutions.py:410-412) into the B-fragment
// order of v_mfma_f32_16x16x4_f32 per channel chunk, following the padded row layout of B:
//   Wp[chunk][blk][g][n][j][q] = W[cell][c0 + cc][16 n + j],  kc' = 16 blk + 4 g + q,
//   plane z = kc' / PS, r = kc' % PS, cell = z*sx*sy + r / CC, cc = r % CC   (r < sx*sy*CC)
// zero for padding entries, c0+cc >= cin or 16n+j >= cout.
__global__ void pack_filter(const float* __restrict__ src, float* __restrict__ dst, int d0, int d1, int d2, int cin,
                            int cout, int CC, int PS, int nchunks, int nblocks, int NT, int symmetric, int sym_axis) {
    const int PR = d1 * d2 * CC;
    const int64_t total = (int64_t)nchunks * nblocks * 4 * NT * 16 * 4;
    const int hd[3] = {(symmetric && sym_axis == 0) ? d0 / 2 : d0, (symmetric && sym_axis == 1) ? d1 / 2 : d1,
                       (symmetric && sym_axis == 2) ? d2 / 2 : d2};
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        int64_t s = e;
        const int q = (int)(s & 3); s >>= 2;
        const int j = (int)(s & 15); s >>= 4;
        const int n = (int)(s % NT); s /= NT;
        const int g = (int)(s & 3); s >>= 2;
        const int blk = (int)(s % nblocks); s /= nblocks;
        const int chunk = (int)s;
        const int kc = 16 * blk + 4 * g + q, cz = kc / PS, r = kc % PS;
        const int ci = chunk * CC + r % CC, o = 16 * n + j;
        float v = 0.0f;
        if (cz < d0 && r < PR && ci < cin && o < cout) {
            const int cp = r / CC;
            int c3[3] = {cz, cp / d2, cp % d2};
            float sign = 1.0f;
            if (symmetric) {
                const int hh = hd[sym_axis];
                if (c3[sym_axis] >= hh) {
                    c3[sym_axis] -= hh;
                } else {
                    sign = -1.0f;
                    for (int a = 0; a < 3; ++a) c3[a] = hd[a] - 1 - c3[a];
                }
            }
            v = sign * src[((((int64_t)c3[0] * hd[1] + c3[1]) * hd[2] + c3[2]) * cin + ci) * cout + o];
        }
        dst[e] = v;
    }
}

struct LaunchCfg {
    int CC, PS, KCp, nblocks, NT, nchunks, zgroup;
    size_t lds, packed_floats, bfloats;
};

static LaunchCfg make_cfg(int sx, int sy, int sz, int cin, int cout) {
    LaunchCfg c;
    c.CC = cin <= 4 ? 4 : 8;
    const int PR = sx * sy * c.CC;
    // Plane stride: the smallest padding of the z plane for which the 8 corners of a pair are conflict free
    // in the LDS bank models of the splat's accesses (CC = 8: 64-bit reads see 64 banks over the 8 corners of
    // a half-wave, 64-bit writes 32 banks over 4 corners at a time; CC = 4: 32-bit accesses, 32 banks over all
    // 8 corners), while one workgroup's B tile still fits.
    auto conflicts = [&](int PS, int zgroup) {
        int bad = 0;
        for (int by = 0; by < 2; ++by)
            for (int bx = 0; bx < 2; ++bx) {
                int off[8];
                for (int t = 0; t < 8; ++t) {
                    const int tx = (t & 1) && sx >= 2, ty = ((t >> 1) & 1) && sy >= 2, tz = ((t >> 2) & 1) && sz >= 2;
                    off[t] = tz * PS + ((by + ty) * sx + bx + tx) * c.CC;
                }
                for (int a = 0; a < 8; ++a)
                    for (int b = a + 1; b < 8; ++b) {
                        if (off[a] == off[b]) continue;  // collapsed corners are masked off in the kernel
                        const int rd = c.CC == 8 ? 64 : 32;
                        if ((off[a] % rd) / c.CC == (off[b] % rd) / c.CC) ++bad;                        // read model
                        // write model: a 16-lane store group holds the 4 corners with equal z bit, or (zgroup) equal y bit
                        const int ga = zgroup ? (a >> 1) & 1 : a >> 2, gb = zgroup ? (b >> 1) & 1 : b >> 2;
                        if (ga == gb && (off[a] % 32) / c.CC == (off[b] % 32) / c.CC) ++bad;
                    }
            }
        return bad;
    };
    const bool has_dead = sx < 2 || sy < 2 || sz < 2;
    auto lds_bytes = [&](int PS) {
        const int KCx = (sz * PS + 15) / 16 * 16;
        const size_t kcp = KCx + ((4 - KCx % 64) + 64) % 64;
        size_t bf = (size_t)TM * kcp;
        const size_t rf = (size_t)kWaves * TM * 16 * ((cout + 15) / 16);
        if (bf < rf) bf = rf;
        return (bf + TM + (size_t)kWaves * kStage + (has_dead ? 2 * kThreads : 0)) * sizeof(float);
    };
    const int PS0 = (PR + 7) / 8 * 8;
    const size_t step = lds_bytes(PS0) <= 80 * 1024 ? 80 * 1024 : 160 * 1024;  // keep the occupancy step of the unpadded tile
    int best = PS0, best_bad = 1 << 30, best_group = 0;
    for (int zgroup = 0; zgroup < 2 && best_bad > 0; ++zgroup)
        for (int k = 0; k < 12; ++k) {
            const int PS = PS0 + 8 * k;
            if (k > 0 && (sz < 2 || lds_bytes(PS) > step)) break;
            const int bad = conflicts(PS, zgroup);
            if (bad < best_bad) { best_bad = bad; best = PS; best_group = zgroup; }
            if (bad == 0) break;
        }
    c.PS = best;
    c.zgroup = best_group;
    const int KC = (sz * c.PS + 15) / 16 * 16;  // multiple of 16 (k blocks of the contraction)
    c.nblocks = KC / 16;
    // row stride == 4 (mod 64) floats: the 16 rows read by one ds_read_b128 of the contraction spread over all banks
    c.KCp = KC + ((4 - KC % 64) + 64) % 64;
    c.NT = (cout + 15) / 16;
    c.nchunks = (cin + c.CC - 1) / c.CC;
    size_t b_floats = (size_t)TM * c.KCp;
    const size_t red_floats = (size_t)kWaves * TM * 16 * c.NT;
    if (b_floats < red_floats) b_floats = red_floats;  // the reduction buffer reuses B
    c.bfloats = b_floats;
    c.lds = lds_bytes(c.PS);
    c.packed_floats = (size_t)c.nchunks * c.nblocks * 4 * c.NT * 16 * 4;
    return c;
}

}  // namespace dmcf

using namespace dmcf;

extern "C" {

static int validate(const dmcf_cconv_args* a, bool forward = true) {
    if (!a) return DMCF_EINVAL;
    for (int d = 0; d < 5; ++d)
        if (a->filter_dims[d] < 1) return DMCF_EINVAL;
    if (a->n_out < 0 || a->n_inp < 0) return DMCF_EINVAL;
    if (!(a->extent > 0.0f)) return DMCF_EINVAL;
    if (a->window < DMCF_WINDOW_NONE || a->window > DMCF_WINDOW_CUBIC_GRAD) return DMCF_EINVAL;
    if (a->coordinate_mapping < 0 || a->coordinate_mapping > 2) return DMCF_EINVAL;
    if (a->interpolation < 0 || a->interpolation > 2) return DMCF_EINVAL;
    if (a->flags & DMCF_FLAG_SYMMETRIC) {
        if (a->sym_axis < 0 || a->sym_axis > 2) return DMCF_EINVAL;
        if (a->n_inp < a->n_out) return DMCF_EINVAL;  // out points are inp points 0..n_out-1
    }
    if (a->filter_dims[4] > 16 * kMaxNT) return DMCF_EUNSUPPORTED;
    if (a->n_out > 0) {
        if (!a->out_positions || !a->neighbors_row_splits) return DMCF_EINVAL;
        if (forward && (!a->filters || !a->out || !a->inp_features)) return DMCF_EINVAL;
        if (a->window == DMCF_WINDOW_EXPLICIT && !a->neighbors_value) return DMCF_EINVAL;
    }
    return DMCF_OK;
}

static void full_dims(const dmcf_cconv_args* a, int& dz, int& dy, int& dx) {
    dz = a->filter_dims[0]; dy = a->filter_dims[1]; dx = a->filter_dims[2];
    if (a->flags & DMCF_FLAG_SYMMETRIC) {
        if (a->sym_axis == 0) dz *= 2;
        if (a->sym_axis == 1) dy *= 2;
        if (a->sym_axis == 2) dx *= 2;
    }
}

// the fields of CconvParams every form takes from the arguments as they are
static void fill_params(const dmcf_cconv_args* a, int dz, int dy, int dx, CconvParams& p) {
    p.partial = nullptr;
    p.csplit = 0;
    p.cin = a->filter_dims[3];
    p.cout = a->filter_dims[4];
    p.sx = dx; p.sy = dy; p.sz = dz;
    p.K = dx * dy * dz;
    p.out_pos = a->out_positions;
    p.inp_pos = a->inp_positions;
    p.inp_feat = a->inp_features;
    p.inp_imp = a->inp_importance;
    p.idx = a->neighbors_index;
    p.rs = a->neighbors_row_splits;
    p.cnt = a->neighbors_row_count;
    // (the hint covers input channels < 32 and output channels < 64: wider layers multiply every block)
    p.wmask = (a->filter_tile_mask && a->filter_dims[3] <= 32 && a->filter_dims[4] <= 64) ? a->filter_tile_mask : 0xffffffffu;
    p.nval = a->neighbors_value;
    p.n_out = a->n_out;
    p.n_inp = a->n_inp;
    p.pair_cap = a->n_pairs;
    p.inv_extent = 1.0f / a->extent;
    const float radius = 0.5f * a->extent;
    p.inv_r2 = 1.0f / (radius * radius);
    p.window_fac = a->window_fac;
    p.window = a->window;
    p.mapping = a->coordinate_mapping;
    p.interp = a->interpolation;
    p.flags = a->flags;
    p.bias = a->bias;
    p.out = a->out;
}

// ---- the generic LDS-splat form: any filter shape and flag set, its own filter packing and LDS budget.  Last in the table, and
// alone behind dmcf_cconv_forward_extents (ext: cconv_ext_kernel, which always packs).
static void generic_pick(const dmcf_cconv_args* a, int dz, int dy, int dx, bool ext, CconvPick& k) {
    const LaunchCfg cfg = make_cfg(dx, dy, dz, a->filter_dims[3], a->filter_dims[4]);
    // the flag set every DMCF model uses gets a specialised instantiation (the printed name does not tell the two apart)
    const bool generic = !cconv_specialised(a);
    CconvKernel f;
    if (ext)
        f = cfg.CC == 8 ? CCONV_KERNEL(cconv_ext_kernel<8>) : CCONV_KERNEL(cconv_ext_kernel<4>);
    else if (cfg.CC == 8)
        f = {generic ? (const void*)cconv_kernel<8, true> : (const void*)cconv_kernel<8, false>, "cconv_kernel<8>"};
    else
        f = {generic ? (const void*)cconv_kernel<4, true> : (const void*)cconv_kernel<4, false>, "cconv_kernel<4>"};
    k = {f.fn, f.name, cfg.lds, kThreads, cfg.packed_floats};
}

static int generic_launch(CconvParams p, const dmcf_cconv_args* a, int dz, int dy, int dx, const CconvPick& k, const float* out_ext,
                          void* workspace, hipStream_t stream) {
    const LaunchCfg cfg = make_cfg(dx, dy, dz, p.cin, p.cout);
    if (cfg.lds > 160 * 1024) return DMCF_EUNSUPPORTED;
    float* packed = (float*)workspace;
    const unsigned g = (unsigned)((cfg.packed_floats + 255) / 256);
    if (out_ext || !(a->flags & DMCF_FLAG_FILTER_PACKED))  // (else the workspace still holds it: dmcf_hip.h)
        hipLaunchKernelGGL(pack_filter, dim3(g < 2048u ? g : 2048u), dim3(256), 0, stream, a->filters, packed, dz, dy, dx,
                           p.cin, p.cout, cfg.CC, cfg.PS, cfg.nchunks, cfg.nblocks, cfg.NT,
                           (a->flags & DMCF_FLAG_SYMMETRIC) ? 1 : 0, a->sym_axis);
    p.Wp = packed;
    p.KCp = cfg.KCp;
    p.PS = cfg.PS;
    p.zgroup = cfg.zgroup;
    p.nblocks = cfg.nblocks;
    p.NT = cfg.NT;
    p.nchunks = cfg.nchunks;
    p.bfloats = (int)cfg.bfloats;
    if (!cconv_set_tiles(p, TM)) return DMCF_EUNSUPPORTED;
    void* kargs[] = {(void*)&p, (void*)&out_ext};
    return cconv_launch_kernel(k, dim3((unsigned)p.tiles_per_xcd * 8u), kargs, stream);
}

static const CconvForm generic_form = {
    0, [](const dmcf_cconv_args*, int, int, int, bool) { return true; },
    [](const dmcf_cconv_args* a, int dz, int dy, int dx, CconvPick& k) { generic_pick(a, dz, dy, dx, false, k); },
    [](const dmcf_cconv_args* a, int dz, int dy, int dx, bool) {
        return make_cfg(dx, dy, dz, a->filter_dims[3], a->filter_dims[4]).packed_floats;
    },
    [](CconvParams p, const dmcf_cconv_args* a, int dz, int dy, int dx, const CconvPick& k, void* workspace, hipStream_t stream) {
        return generic_launch(p, a, dz, dy, dx, k, nullptr, workspace, stream);
    }};

// ---- THE dispatch table of dmcf_cconv_forward: the first form that accepts a call takes it.  A new form is one more row here (and
// its CconvForm next to its kernel); the kernel name, the workspace size and the launch all follow from the row.
static const CconvForm* const kForms[] = {&cconv_direct_form, &cconv_ws_form,  &cconv_pair_form, &cconv_p16_form, &cconv_z3_form,
                                          &cconv_cls_form,    &cconv_blk_form, &cconv_mfma_form, &generic_form};

// could the dispatch give the call to this form, were no earlier one to take it?  forced: cconv_forced_key()
static bool form_accepts(const CconvForm& f, const dmcf_cconv_args* a, int dz, int dy, int dx, int forced) {
    if (f.key && forced >= 0 && forced != f.key) return false;
    return f.eligible(a, dz, dy, dx, forced >= 0);
}

// The form validated arguments dispatch to, and what it launches for them.
static int cconv_select(const dmcf_cconv_args* a, int dz, int dy, int dx, const CconvForm*& form, CconvPick& k) {
    const int forced = cconv_forced_key();
    for (const CconvForm* f : kForms) {
        if (!form_accepts(*f, a, dz, dy, dx, forced)) continue;
        // (only the direct form tests a pair's index against its row)
        if ((a->flags & DMCF_FLAG_SKIP_SELF) && f != &cconv_direct_form) return DMCF_EUNSUPPORTED;
        form = f;
        f->pick(a, dz, dy, dx, k);
        return DMCF_OK;
    }
    return DMCF_EUNSUPPORTED;  // (not reached: the generic form accepts everything)
}

size_t dmcf_cconv_workspace_bytes(const dmcf_cconv_args* a) {
    if (!a || validate(a) != DMCF_OK) return 256;
    int dz, dy, dx;
    full_dims(a, dz, dy, dx);
    const int forced = cconv_forced_key();
    size_t floats = 0;
    for (const CconvForm* f : kForms) {
        const size_t ff = f->workspace_floats(a, dz, dy, dx, form_accepts(*f, a, dz, dy, dx, forced));
        if (floats < ff) floats = ff;
    }
    return 256 + align_up(floats * sizeof(float), 256);
}

int dmcf_cconv_forward(const dmcf_cconv_args* a, void* workspace, size_t workspace_bytes, dmcf_stream_t stream_) {
    int rc = validate(a);
    if (rc != DMCF_OK) return rc;
    if (a->n_out == 0) return DMCF_OK;
    if (!workspace || ((uintptr_t)workspace & 255)) return DMCF_EINVAL;
    if (workspace_bytes < dmcf_cconv_workspace_bytes(a)) return DMCF_EWORKSPACE;

    CconvParams p;
    int dz, dy, dx;
    full_dims(a, dz, dy, dx);
    fill_params(a, dz, dy, dx, p);
    const CconvForm* form;
    CconvPick k;
    rc = cconv_select(a, dz, dy, dx, form, k);
    if (rc != DMCF_OK) return rc;
    return form->launch(p, a, dz, dy, dx, k, workspace, (hipStream_t)stream_);
}

// dmcf_cconv_forward_extents ignores args->extent: validate (and size the workspace) as for any positive one
static int validate_extents(const dmcf_cconv_args* a, const float* out_extents, dmcf_cconv_args& b) {
    if (!a) return DMCF_EINVAL;
    b = *a;
    b.extent = 1.0f;
    const int rc = validate(&b);
    if (rc != DMCF_OK) return rc;
    if (a->flags & DMCF_FLAG_SKIP_SELF) return DMCF_EUNSUPPORTED;
    if (a->n_out > 0 && !out_extents) return DMCF_EINVAL;
    return DMCF_OK;
}

int dmcf_cconv_forward_extents(const dmcf_cconv_args* a, const float* out_extents, void* workspace, size_t workspace_bytes,
                               dmcf_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    dmcf_cconv_args b;
    const int rc = validate_extents(a, out_extents, b);
    if (rc != DMCF_OK) return rc;
    if (b.n_out == 0) return DMCF_OK;
    if (!workspace || ((uintptr_t)workspace & 255)) return DMCF_EINVAL;
    if (workspace_bytes < dmcf_cconv_workspace_bytes(&b)) return DMCF_EWORKSPACE;
    CconvParams p;
    int dz, dy, dx;
    full_dims(&b, dz, dy, dx);
    fill_params(&b, dz, dy, dx, p);
    CconvPick k;
    generic_pick(&b, dz, dy, dx, true, k);
    return generic_launch(p, &b, dz, dy, dx, k, out_extents, workspace, stream);
}

int dmcf_cconv_kernel_name(const dmcf_cconv_args* a, char* name, size_t name_bytes) {
    if (!name || name_bytes < 2) return DMCF_EINVAL;
    int rc = validate(a, false);
    if (rc != DMCF_OK) return rc;
    int dz, dy, dx;
    full_dims(a, dz, dy, dx);
    const CconvForm* form;
    CconvPick k;
    rc = cconv_select(a, dz, dy, dx, form, k);
    if (rc != DMCF_OK) return rc;
    snprintf(name, name_bytes, "%s", k.name);
    return DMCF_OK;
}

int dmcf_cconv_extents_kernel_name(const dmcf_cconv_args* a, char* name, size_t name_bytes) {
    if (!name || name_bytes < 2 || !a) return DMCF_EINVAL;
    dmcf_cconv_args b = *a;
    b.extent = 1.0f;
    const int rc = validate(&b, false);
    if (rc != DMCF_OK) return rc;
    if (a->flags & DMCF_FLAG_SKIP_SELF) return DMCF_EUNSUPPORTED;
    int dz, dy, dx;
    full_dims(&b, dz, dy, dx);
    CconvPick k;
    generic_pick(&b, dz, dy, dx, true, k);
    snprintf(name, name_bytes, "%s", k.name);
    return DMCF_OK;
}

}  // extern "C"
