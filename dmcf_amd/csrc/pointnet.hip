// PointNet's layer (dmcf_neighbor_dense_forward / _backward): a Dense followed by a ragged sum over the fixed-radius
// neighbours, as the reference's models/pointnet.py:137-145 computes it,
//     out_r = sum_{p in row r} (act(x_{idx[p]}) W + b)  (+ residual_r)
// reordered as
//     out_r = S_r W + c_r b (+ residual_r),   S_r = sum_{p in row r, idx[p] < n_in} act(x_{idx[p]}),   c_r = #those pairs.
// A neighbour index outside [0, n_in) contributes nothing, neither features nor bias: TensorFlow's GPU gather returns zeros
// for such rows and its gradient drops them (layer 0 of the reference gathers fluid-only rows with indices over fluid AND
// boundary points).
//
// Kernels (the names dmcf_neighbor_dense_kernel_names reports):
//   nd_gather_mfma       one launch per layer.  A wave owns a tile of 16 output rows at a time (persistent over the tiles):
//                        it sums the 16 rows' gathered input rows in pair order, lane = channel, all 16 rows in flight at
//                        once, into a 16 x Cin image in LDS; then contracts that image with W (staged in LDS once per
//                        workgroup) on v_mfma_f32_16x16x4_f32 and adds c_r b, the residual and (backward) the ReLU mask
//                        in the epilogue.  No barrier between the waves after W is staged: one wave's gather overlaps
//                        another's contraction.
//   nd_bwd_weight        the backward's dW = S^T G and db = sum_r c_r G_r: one workgroup per (row slab, 64 channels of
//                        [S | c]) on the matrix cores, partials per slab
//   nd_bwd_weight_reduce the slabs summed in slab order
// The backward's input gradient is nd_gather_mfma on the inverted list with W^T and the mask x > 0 (ReLU).
// No float atomics anywhere: every output element is written by one lane, so two identical calls give identical bits.
#include <stdio.h>
#include <string.h>

#include "common.h"

namespace dmcf {

typedef float nd_f32x4 __attribute__((ext_vector_type(4)));

constexpr int kNdWaves = 8;        // waves per workgroup of nd_gather_mfma
constexpr int kNdRows = 16;        // output rows per wave tile (the M of one 16x16x4 instruction)
constexpr int kNdMaxC = 128;       // Cin, Cout limit: two channels per lane in the gather, 8 accumulators in the contraction
constexpr int kNdLds = 160 * 1024;
constexpr int kNdSlabRows = 128;   // backward: at least this many rows per slab ...
constexpr int kNdMaxSlabs = 2048;  // ... and at most this many slabs (about 24 waves per CU at 10^6 rows)

struct NdParams {
    const float* x;
    int64_t n_in;
    int cin, cout, cin_p, cout_p;   // padded: cin_p a multiple of 4, cout_p of 16
    int s_stride, w_stride;         // LDS row strides (floats) of the S image and of W
    const float* W;
    int w_transposed;
    const float* bias;
    const float* residual;
    const float* mask;
    const int32_t* idx;
    const int64_t* rs;
    const int32_t* cnt;
    int64_t n_out, n_pairs;
    float* out;
    float* rec_s;
    float* rec_c;
    int relu;
    int64_t n_tiles;
};

// LDS strides: W rows 16 floats past a multiple of 32 (the four k rows of a B fragment fall on distinct bank halves),
// S rows 2 past a multiple of 4 (the 16 rows x 4 k of an A fragment on distinct banks)
static int nd_w_stride(int cout_p) { return cout_p + 16; }
static int nd_s_stride(int cin_p) { return cin_p + 2; }
static size_t nd_lds_bytes(int cin_p, int cout_p) {
    return sizeof(float) * ((size_t)cin_p * nd_w_stride(cout_p) + (size_t)kNdWaves * kNdRows * nd_s_stride(cin_p) + kNdWaves * kNdRows);
}

template <int CPL>
__global__ __launch_bounds__(kNdWaves * 64) void nd_gather_mfma(const NdParams p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float* Wl = smem;                                                       // [cin_p][w_stride]
    float* Sl = Wl + (size_t)p.cin_p * p.w_stride + (size_t)wv * kNdRows * p.s_stride;  // this wave's [16][s_stride]
    float* Cl = smem + (size_t)p.cin_p * p.w_stride + (size_t)kNdWaves * kNdRows * p.s_stride + wv * kNdRows;  // [16] counts
    // stage W (zero padded to cin_p x cout_p); B[k][col] = W[k][col], or W[col][k] when transposed
    for (int e = threadIdx.x; e < p.cin_p * p.cout_p; e += blockDim.x) {
        const int k = e / p.cout_p, col = e % p.cout_p;
        float v = 0.0f;
        if (k < p.cin && col < p.cout) v = p.w_transposed ? p.W[(size_t)col * p.cin + k] : p.W[(size_t)k * p.cout + col];
        Wl[k * p.w_stride + col] = v;
    }
    __syncthreads();

    const int64_t wave = (int64_t)blockIdx.x * kNdWaves + wv, nwaves = (int64_t)gridDim.x * kNdWaves;
    const int r16 = lane & 15, q = lane >> 4;
    for (int64_t tile = wave; tile < p.n_tiles; tile += nwaves) {
        const int64_t row0 = tile * kNdRows;
        // the 16 rows' pair ranges: lane r < 16 holds row r's [rb, re); empty for rows past n_out or out of the list
        int64_t myb = 0, mye = 0;
        if (lane < kNdRows && row0 + lane < p.n_out) {
            const int64_t r = row0 + lane;
            myb = p.rs[r];
            mye = p.cnt ? myb + p.cnt[r] : p.rs[r + 1];
            if (myb < 0 || mye < myb || mye > p.n_pairs) mye = myb;
        }
        // (read out lane by lane: the ranges, the indices and every branch below are wave-uniform, in scalar registers)
        int64_t rb[kNdRows];
        int len[kNdRows];
        int maxlen = 0;
        const int mylen = (int)(mye - myb);
#pragma unroll
        for (int r = 0; r < kNdRows; ++r) {
            const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)myb, r);
            const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)myb >> 32), r);
            rb[r] = (int64_t)(((uint64_t)hi << 32) | lo);
            len[r] = __builtin_amdgcn_readlane(mylen, r);
            maxlen = max(maxlen, len[r]);
        }
        float acc[kNdRows][CPL];
        int cnt[kNdRows];
#pragma unroll
        for (int r = 0; r < kNdRows; ++r) {
            cnt[r] = 0;
#pragma unroll
            for (int c = 0; c < CPL; ++c) acc[r][c] = 0.0f;
        }
        // pairs k0 .. k0 + 63 of the 16 rows: their indices first (one coalesced load per row, lane = pair), then pair k of
        // every row in turn -- each row's sum is formed in pair order, the 16 rows' feature loads are independent
        for (int k0 = 0; k0 < maxlen; k0 += 64) {
            int jv[kNdRows];
#pragma unroll
            for (int r = 0; r < kNdRows; ++r) jv[r] = lane < len[r] - k0 ? p.idx[rb[r] + k0 + lane] : -1;
            const int kend = min(64, maxlen - k0);
            for (int k = 0; k < kend; ++k) {
                // every row's load first, then the sums: a load consumed right away would wait for its round trip 16 times
                float v[kNdRows][CPL];
                bool ok[kNdRows];
#pragma unroll
                for (int r = 0; r < kNdRows; ++r) {
                    const int j = __builtin_amdgcn_readlane(jv[r], k);
                    ok[r] = j >= 0 && (int64_t)j < p.n_in;
                    const float* xr = p.x + (int64_t)(ok[r] ? j : 0) * p.cin;
#pragma unroll
                    for (int c = 0; c < CPL; ++c) {
                        const int ch = lane + 64 * c;
                        v[r][c] = (ok[r] && ch < p.cin) ? xr[ch] : 0.0f;
                    }
                }
#pragma unroll
                for (int r = 0; r < kNdRows; ++r) {
                    if (!ok[r]) continue;
#pragma unroll
                    for (int c = 0; c < CPL; ++c) acc[r][c] += p.relu ? fmaxf(v[r][c], 0.0f) : v[r][c];
                    ++cnt[r];
                }
            }
        }
#pragma unroll
        for (int r = 0; r < kNdRows; ++r) {
#pragma unroll
            for (int c = 0; c < CPL; ++c) {
                const int ch = lane + 64 * c;
                if (ch < p.cin_p) Sl[r * p.s_stride + ch] = acc[r][c];
            }
        }
        if (lane < kNdRows) {
            float cr = 0.0f;
#pragma unroll
            for (int r = 0; r < kNdRows; ++r)
                if (r == lane) cr = (float)cnt[r];
            Cl[lane] = cr;
        }
        if (p.rec_s) {
#pragma unroll
            for (int r = 0; r < kNdRows; ++r) {
                if (row0 + r >= p.n_out) continue;
#pragma unroll
                for (int c = 0; c < CPL; ++c) {
                    const int ch = lane + 64 * c;
                    if (ch < p.cin) p.rec_s[(row0 + r) * p.cin + ch] = acc[r][c];
                }
            }
            if (lane < kNdRows && row0 + lane < p.n_out) p.rec_c[row0 + lane] = Cl[lane];
        }
        // (LDS operations of one wave complete in order; the fence keeps the compiler from moving the reads up)
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();

        // out tile [16, cout_p] = S [16, cin_p] W [cin_p, cout_p]: A[i][kk] = S[i][4s + kk], B[kk][jj] = W[4s + kk][16t + jj]
        nd_f32x4 d[kNdMaxC / 16];
#pragma unroll
        for (int t = 0; t < kNdMaxC / 16; ++t) d[t] = (nd_f32x4){0.0f, 0.0f, 0.0f, 0.0f};
        const int nt = p.cout_p >> 4;
        for (int s = 0; s < (p.cin_p >> 2); ++s) {
            const float a = Sl[r16 * p.s_stride + 4 * s + q];
            const float* wrow = Wl + (4 * s + q) * p.w_stride + r16;
#pragma unroll
            for (int t = 0; t < kNdMaxC / 16; ++t)
                if (t < nt) d[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, wrow[16 * t], d[t], 0, 0, 0);
        }
        // D: lane holds rows 4 q + e, column 16 t + r16
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int rr = 4 * q + e;
            const int64_t orow = row0 + rr;
            if (orow >= p.n_out) continue;
            const float cr = Cl[rr];
#pragma unroll
            for (int t = 0; t < kNdMaxC / 16; ++t) {
                const int col = 16 * t + r16;
                if (t >= nt || col >= p.cout) continue;
                float v = d[t][e];
                if (p.bias) v += cr * p.bias[col];
                if (p.residual) v += p.residual[orow * p.cout + col];
                if (p.mask && !(p.mask[orow * p.cout + col] > 0.0f)) v = 0.0f;
                p.out[orow * p.cout + col] = v;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}

// dW / db partials: slab z of rows, channels 64 y + 16 w + (0..15) of [S | c] (channel cin is the count), all columns of G.
__global__ __launch_bounds__(256) void nd_bwd_weight(const float* __restrict__ S, const float* __restrict__ C, const float* __restrict__ G,
                                                     int64_t n, int cin, int cout, int64_t rows_per_slab, float* __restrict__ part) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int r16 = lane & 15, q = lane >> 4;
    const int ch = 64 * blockIdx.y + 16 * wv + r16;
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_slab, r1 = min(n, r0 + rows_per_slab);
    const int nt = (cout + 15) >> 4;
    nd_f32x4 d[kNdMaxC / 16];
#pragma unroll
    for (int t = 0; t < kNdMaxC / 16; ++t) d[t] = (nd_f32x4){0.0f, 0.0f, 0.0f, 0.0f};
    // operands of rows rbase .. rbase + 3 (lane row q): loaded one step ahead of the instructions that consume them
    auto load = [&](int64_t rbase, float& a, float (&b)[kNdMaxC / 16]) {
        const int64_t r = rbase + q;
        a = 0.0f;
        if (r < r1) a = ch < cin ? S[r * cin + ch] : (ch == cin ? C[r] : 0.0f);
#pragma unroll
        for (int t = 0; t < kNdMaxC / 16; ++t) {
            const int col = 16 * t + r16;
            b[t] = (t < nt && r < r1 && col < cout) ? G[r * cout + col] : 0.0f;
        }
    };
    float a0, b0[kNdMaxC / 16];
    load(r0, a0, b0);
    for (int64_t rbase = r0; rbase < r1; rbase += 4) {
        float a1, b1[kNdMaxC / 16];
        load(rbase + 4, a1, b1);
#pragma unroll
        for (int t = 0; t < kNdMaxC / 16; ++t)
            if (t < nt) d[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0[t], d[t], 0, 0, 0);
        a0 = a1;
#pragma unroll
        for (int t = 0; t < kNdMaxC / 16; ++t) b0[t] = b1[t];
    }
    // D: rows (channels) 64 y + 16 w + 4 q + e, column 16 t + r16 -> part[z][ch][col] over (cin + 1) x cout
    float* dst = part + (size_t)blockIdx.x * (cin + 1) * cout;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int c = 64 * blockIdx.y + 16 * wv + 4 * q + e;
        if (c > cin) continue;
#pragma unroll
        for (int t = 0; t < kNdMaxC / 16; ++t) {
            const int col = 16 * t + r16;
            if (t < nt && col < cout) dst[(size_t)c * cout + col] = d[t][e];
        }
    }
}

__global__ void nd_bwd_weight_reduce(const float* __restrict__ part, int nslabs, int cin, int cout, float* __restrict__ dW,
                                     float* __restrict__ db) {
    const int64_t n = (int64_t)(cin + 1) * cout;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        float v = 0.0f;
        for (int s = 0; s < nslabs; ++s) v += part[(size_t)s * n + e];
        if (e < (int64_t)cin * cout) {
            if (dW) dW[e] = v;
        } else if (db) {
            db[e - (int64_t)cin * cout] = v;
        }
    }
}

// ---- host side ----
static int nd_check_host_splits(const int64_t* hs, const int32_t* cnt, int64_t n_out, int64_t n_pairs) {
    if (!hs) return DMCF_OK;
    if (cnt) {  // padded rows: begins only, each inside the list
        for (int64_t i = 0; i < n_out; ++i)
            if (hs[i] < 0 || hs[i] > n_pairs) return DMCF_EINVAL;
        return DMCF_OK;
    }
    if (hs[0] != 0 || hs[n_out] != n_pairs) return DMCF_EINVAL;
    for (int64_t i = 0; i < n_out; ++i)
        if (hs[i + 1] < hs[i]) return DMCF_EINVAL;
    return DMCF_OK;
}

static int nd_plan(const dmcf_neighbor_dense_args* a, NdParams& p, size_t& lds) {
    if (!a || a->struct_size < sizeof(dmcf_neighbor_dense_args)) return DMCF_EINVAL;
    if (a->flags & ~(DMCF_ND_RELU | DMCF_ND_W_TRANSPOSED)) return DMCF_EINVAL;
    if (a->cin <= 0 || a->cout <= 0 || a->n_in < 0 || a->n_out < 0 || a->n_pairs < 0) return DMCF_EINVAL;
    if (a->n_in > INT32_MAX) return DMCF_EINVAL;
    if (!a->kernel || !a->neighbors_row_splits || (a->n_out > 0 && !a->out)) return DMCF_EINVAL;
    if (a->n_in > 0 && !a->x) return DMCF_EINVAL;
    if (a->n_pairs > 0 && !a->neighbors_index) return DMCF_EINVAL;
    if ((a->record_s == nullptr) != (a->record_count == nullptr)) return DMCF_EINVAL;
    int rc = nd_check_host_splits(a->host_row_splits, a->neighbors_row_count, a->n_out, a->n_pairs);
    if (rc != DMCF_OK) return rc;
    if (a->cin > kNdMaxC || a->cout > kNdMaxC) return DMCF_EUNSUPPORTED;
    p.x = a->x;
    p.n_in = a->n_in;
    p.cin = a->cin;
    p.cout = a->cout;
    p.cin_p = (a->cin + 3) & ~3;
    p.cout_p = (a->cout + 15) & ~15;
    p.w_stride = nd_w_stride(p.cout_p);
    p.s_stride = nd_s_stride(p.cin_p);
    p.W = a->kernel;
    p.w_transposed = (a->flags & DMCF_ND_W_TRANSPOSED) ? 1 : 0;
    p.bias = a->bias;
    p.residual = a->residual;
    p.mask = a->mask;
    p.idx = a->neighbors_index;
    p.rs = a->neighbors_row_splits;
    p.cnt = a->neighbors_row_count;
    p.n_out = a->n_out;
    p.n_pairs = a->n_pairs;
    p.out = a->out;
    p.rec_s = a->record_s;
    p.rec_c = a->record_count;
    p.relu = (a->flags & DMCF_ND_RELU) ? 1 : 0;
    p.n_tiles = (a->n_out + kNdRows - 1) / kNdRows;
    lds = nd_lds_bytes(p.cin_p, p.cout_p);
    if (lds > (size_t)kNdLds) return DMCF_EUNSUPPORTED;
    return DMCF_OK;
}

static const char* nd_gather_name(int cin) { return cin > 64 ? "nd_gather_mfma<2>" : "nd_gather_mfma<1>"; }

static int nd_launch(const NdParams& p, size_t lds, hipStream_t stream) {
    if (p.n_tiles == 0) return DMCF_OK;
    const void* fn = p.cin > 64 ? (const void*)nd_gather_mfma<2> : (const void*)nd_gather_mfma<1>;
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) { g_last_hip_error = (int)e; return DMCF_ELAUNCH; }
    // persistent: as many workgroups as fit on the device at once (LDS- and wave-limited), or fewer when the tiles are few
    const int per_cu = max(1, min(32 / kNdWaves, (int)(kNdLds / lds)));
    const int64_t want = (p.n_tiles + kNdWaves - 1) / kNdWaves;
    const unsigned grid = (unsigned)min(want, (int64_t)device_cu_count() * per_cu);
    if (p.cin > 64)
        hipLaunchKernelGGL(nd_gather_mfma<2>, dim3(grid), dim3(kNdWaves * 64), lds, stream, p);
    else
        hipLaunchKernelGGL(nd_gather_mfma<1>, dim3(grid), dim3(kNdWaves * 64), lds, stream, p);
    return check_launch();
}

struct NdBwdPlan {
    bool want_x, want_w;
    int64_t rows_per_slab;
    int nslabs;
    size_t ws_bytes;
};

static int nd_bwd_plan(const dmcf_neighbor_dense_backward_args* b, NdBwdPlan& pl) {
    if (!b || b->struct_size < sizeof(dmcf_neighbor_dense_backward_args)) return DMCF_EINVAL;
    if (b->flags & ~DMCF_ND_RELU) return DMCF_EINVAL;
    if (b->cin <= 0 || b->cout <= 0 || b->n_in < 0 || b->n_out < 0 || b->inv_n_pairs < 0) return DMCF_EINVAL;
    if (b->n_out > INT32_MAX) return DMCF_EINVAL;
    if (!b->kernel) return DMCF_EINVAL;
    if (b->n_out > 0 && !b->grad_out) return DMCF_EINVAL;
    pl.want_x = b->grad_x != nullptr;
    pl.want_w = b->grad_kernel != nullptr || b->grad_bias != nullptr;
    if (pl.want_x) {
        if (!b->inv_row_splits) return DMCF_EINVAL;
        if (b->n_in > 0 && (b->flags & DMCF_ND_RELU) && !b->x) return DMCF_EINVAL;
        if (b->inv_n_pairs > 0 && !b->inv_index) return DMCF_EINVAL;
    }
    if (pl.want_w && b->n_out > 0 && (!b->s || !b->count)) return DMCF_EINVAL;
    if (b->cin > kNdMaxC || b->cout > kNdMaxC) return DMCF_EUNSUPPORTED;
    if (nd_lds_bytes((b->cout + 3) & ~3, (b->cin + 15) & ~15) > (size_t)kNdLds) return DMCF_EUNSUPPORTED;
    int64_t S = (b->n_out + kNdSlabRows - 1) / kNdSlabRows;
    S = max((int64_t)1, min(S, (int64_t)kNdMaxSlabs));
    pl.rows_per_slab = (b->n_out + S - 1) / S;
    pl.rows_per_slab = (pl.rows_per_slab + 3) & ~(int64_t)3;
    pl.nslabs = (int)max((int64_t)1, (b->n_out + pl.rows_per_slab - 1) / max(pl.rows_per_slab, (int64_t)1));
    pl.ws_bytes = pl.want_w ? sizeof(float) * (size_t)pl.nslabs * (b->cin + 1) * b->cout : 0;
    return DMCF_OK;
}

}  // namespace dmcf

using namespace dmcf;

extern "C" {

int dmcf_neighbor_dense_forward(const dmcf_neighbor_dense_args* a, dmcf_stream_t stream) {
    NdParams p;
    size_t lds = 0;
    const int rc = nd_plan(a, p, lds);
    if (rc != DMCF_OK) return rc;
    return nd_launch(p, lds, (hipStream_t)stream);
}

size_t dmcf_neighbor_dense_backward_workspace_bytes(const dmcf_neighbor_dense_backward_args* b) {
    NdBwdPlan pl;
    if (nd_bwd_plan(b, pl) != DMCF_OK) return 0;
    return pl.ws_bytes;
}

int dmcf_neighbor_dense_backward(const dmcf_neighbor_dense_backward_args* b, void* workspace, size_t workspace_bytes,
                                 dmcf_stream_t stream) {
    NdBwdPlan pl;
    int rc = nd_bwd_plan(b, pl);
    if (rc != DMCF_OK) return rc;
    if (workspace_bytes < pl.ws_bytes || (pl.ws_bytes && !workspace)) return DMCF_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    if (pl.want_x) {
        // dx_j = act'(x_j) (sum_{r : j in row r} G_r) W^T: the forward kernel on the inverted list (rows = inputs j, entries =
        // output rows r), W read transposed, x > 0 as the epilogue mask
        dmcf_neighbor_dense_args f;
        memset(&f, 0, sizeof(f));
        f.struct_size = sizeof(f);
        f.flags = DMCF_ND_W_TRANSPOSED;
        f.x = b->grad_out;
        f.n_in = b->n_out;
        f.cin = b->cout;
        f.cout = b->cin;
        f.kernel = b->kernel;
        f.mask = (b->flags & DMCF_ND_RELU) ? b->x : nullptr;
        f.neighbors_index = b->inv_index;
        f.neighbors_row_splits = b->inv_row_splits;
        f.n_out = b->n_in;
        f.n_pairs = b->inv_n_pairs;
        f.out = b->grad_x;
        NdParams p;
        size_t lds = 0;
        rc = nd_plan(&f, p, lds);
        if (rc != DMCF_OK) return rc;
        rc = nd_launch(p, lds, st);
        if (rc != DMCF_OK) return rc;
    }
    if (pl.want_w) {
        float* part = (float*)workspace;
        if (b->n_out > 0) {
            hipLaunchKernelGGL(nd_bwd_weight, dim3((unsigned)pl.nslabs, (unsigned)((b->cin + 1 + 63) / 64)), dim3(256), 0, st, b->s,
                               b->count, b->grad_out, b->n_out, b->cin, b->cout, pl.rows_per_slab, part);
            rc = check_launch();
            if (rc != DMCF_OK) return rc;
        } else {
            if (hipMemsetAsync(part, 0, pl.ws_bytes, st) != hipSuccess) return DMCF_ELAUNCH;
        }
        const int64_t n = (int64_t)(b->cin + 1) * b->cout;
        hipLaunchKernelGGL(nd_bwd_weight_reduce, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const float*)part, pl.nslabs,
                           b->cin, b->cout, b->grad_kernel, b->grad_bias);
        rc = check_launch();
        if (rc != DMCF_OK) return rc;
    }
    return DMCF_OK;
}

int dmcf_neighbor_dense_kernel_names(const dmcf_neighbor_dense_args* fwd, const dmcf_neighbor_dense_backward_args* bwd, char* names,
                                     size_t name_bytes) {
    if (!names || name_bytes < 2 || (!fwd && !bwd)) return DMCF_EINVAL;
    char buf[256];
    buf[0] = 0;
    auto add = [&](const char* s) {
        if (buf[0]) strncat(buf, ";", sizeof(buf) - strlen(buf) - 1);
        strncat(buf, s, sizeof(buf) - strlen(buf) - 1);
    };
    if (fwd) {
        NdParams p;
        size_t lds = 0;
        const int rc = nd_plan(fwd, p, lds);
        if (rc != DMCF_OK) return rc;
        if (p.n_tiles) add(nd_gather_name(p.cin));
    }
    if (bwd) {
        NdBwdPlan pl;
        const int rc = nd_bwd_plan(bwd, pl);
        if (rc != DMCF_OK) return rc;
        if (pl.want_x && bwd->n_in > 0) add(nd_gather_name(bwd->cout));
        if (pl.want_w) {
            if (bwd->n_out > 0) add("nd_bwd_weight");
            add("nd_bwd_weight_reduce");
        }
    }
    if (strlen(buf) + 1 > name_bytes) return DMCF_EINVAL;
    memcpy(names, buf, strlen(buf) + 1);
    return DMCF_OK;
}

}  // extern "C"
