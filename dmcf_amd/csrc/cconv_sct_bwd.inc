// Backward of the particles -> coarse lattice CConv, INPUT STATIONARY (dmcf_cconv_scatter_backward; included by cconv_sct.hip,
// inside namespace dmcf, so that it sees sct_scale, sct_fixed and lds_add_i64).  It is the forward's order of evaluation run
// backwards.  Per input point j, with pair weight a_p and the 8 trilinear corners (cell_k, w_k) as the forward forms them:
//
//     T_j[cell][o]   = sum_{pairs p = (i, j)} a_p sum_k [cell_k(p) == cell] w_k(p) G[i][o]          (64 x Cout values)
//     dF[j][c]       = sum_{cell, o} W[cell][c][o] T_j[cell][o]
//     dW[cell][c][o] = sum_j f_j[c] T_j[cell][o]
//
// so both gradients come out of ONE walk over the transposed list (row j = the outputs within R of input j: the list a search with
// the roles swapped returns, no inversion), 8 x Cout multiply-adds per pair with every lane a pair, and nothing of size
// pairs x channels touches memory.  No plan: rows go to workgroups statically in input-index order, and grad_out (n_out x Cout
// floats) is small enough to stay in L2 whatever the order.
//
// Workgroup = 4 waves, a step = a chunk of 16 consecutive rows:
//   * walk: a wave takes rows wave, wave + 4, ... of the chunk one at a time.  A lane loads its pair's output index, position and
//     grad_out row, forms the geometry with the forward's device functions, and adds its 8 x Cout terms into the wave's T (64 x
//     Cout 64-bit integers in LDS) as FIXED POINT, exactly as the forward adds into its slot box: round(term * 2^s), 2^s * max
//     |grad_out| * max(1, |window_fac|) <= 2^46 with the maximum formed on the device in the call.  Integer adds commute: the
//     LDS atomics give the same bits in any order.  After the row the wave converts T to float into the chunk's [16][64 Cout]
//     tile and clears its integers.
//   * products, on the matrix cores (v_mfma_f32_16x16x4_f32): dF chunk [16][Cin] = T . Wf^T -- the forward's chunk product
//     transposed; wave = (column tile of 16 channels, half of K = 64 Cout), the filter stays in registers as B fragments, the two
//     halves are added through LDS in a fixed order -- and dW partial [Cin][64 Cout] += F^T . T, each wave its share of the column
//     tiles, accumulated in registers over all of the workgroup's chunks and stored ONCE.
//   * sct_bwd_reduce adds the workgroups' partials in workgroup order.  The number of workgroups depends on n_inp only
//     (kSbMaxGroups), not on the device, so the float sums are the same on every device.
// No float atomics; two identical calls give identical bits.
//
// Resources (-Rpass-analysis=kernel-resource-usage, gfx950): see DESIGN.md section 4.6.

constexpr int kSbRows = 16;          // rows per chunk
constexpr int kSbWaves = 4;
constexpr int kSbMaxGroups = 1024;   // workgroups (and partial filter gradients) at most

struct SctBwdParams {
    const float* W;          // [4][4][4][cin][cout]
    const float* out_pos;    // [n_out][3]
    const float* inp_pos;    // [n_inp][3]
    const float* inp_feat;   // [n_inp][cin]
    const int32_t* t_idx;    // transposed list, as SctParams
    const int64_t* t_rs;
    const int32_t* t_cnt;
    int64_t t_cap;
    const float* gout;       // [n_out][cout]
    const uint32_t* bound;   // device [2]: float bits of max |grad_out| and of 1.0 (sct_bwd_bound_kernel), read by sct_scale
    float* partial;          // [groups][cin][64 cout] or NULL (no filter gradient wanted)
    float* dfeat;            // [n_inp][cin] or NULL
    int64_t n_out, n_inp;
    int n_chunks, cin;
    float inv_extent, inv_r2, window_fac;
    int window;
};

// max |grad_out| as float bits (non-negative floats order like their bits); the second factor of sct_scale's bound is 1
__global__ __launch_bounds__(256) void sct_bwd_bound_kernel(const float* __restrict__ g, int64_t n, uint32_t* __restrict__ bound) {
    float m = 0.0f;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) m = fmaxf(m, fabsf(g[i]));
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = fmaxf(m, __shfl_xor(m, d, kWave));
    if (lane_id() == 0 && m > 0.0f) atomicMax(&bound[0], __float_as_uint(m));
    if (blockIdx.x == 0 && threadIdx.x == 0) bound[1] = __float_as_uint(1.0f);
}

template <int COUT>
__global__ __launch_bounds__(64 * kSbWaves) void cconv_sct_bwd_kernel(const SctBwdParams p) {
    constexpr int GROW = 64 * COUT;               // floats per T row
    constexpr int TROW = GROW + 4;                // its stride in LDS: 16 rows read at one column fall into 16 different banks
    constexpr int NTW = GROW / 16 / kSbWaves;     // 16-column tiles of the dW partial per wave
    constexpr int KB = GROW / 2 / 16;             // blocks of 16 k per K half of the dF product
    __shared__ unsigned long long Acc[kSbWaves][GROW];
    __shared__ __attribute__((aligned(16))) float Tf[kSbRows * TROW];
    __shared__ float Dp[2][16][17];               // the upper K half's dF tiles
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r16 = lane & 15, q4 = lane >> 4;
    const int cin = p.cin;
    const int ct = wave & 1, kh = wave >> 1, kbase = kh * (GROW / 2);
    const bool df_tile = p.dfeat != nullptr && 16 * ct < cin;

    // dF: the filter as B fragments, Wf^T[k][c] = W[cell][c][o] with k = cell * COUT + o; lane (r16, q4) holds
    // Wf^T[kbase + 16 mb + 4 q4 + i][16 ct + r16] (the k order inside a block of 16 is the forward's: one 16-byte read of T per 4 products)
    float wb[KB][4];
#pragma unroll
    for (int mb = 0; mb < KB; ++mb)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int k = kbase + 16 * mb + 4 * q4 + i, c = 16 * ct + r16;
            wb[mb][i] = (df_tile && c < cin) ? p.W[((int64_t)(k / COUT) * cin + c) * COUT + (k % COUT)] : 0.0f;
        }
    f32x4 dw[2][NTW];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int tt = 0; tt < NTW; ++tt) dw[mt][tt] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
    for (int e = lane; e < GROW; e += 64) Acc[wave][e] = 0ull;
    const float S = sct_scale(p.bound, p.window_fac);
    const double inv_S = 1.0 / (double)S;  // (a power of two: exact)
    CconvParams gp;  // (only what filter_coords<false> reads)
    gp.inv_extent = p.inv_extent;
    gp.sx = gp.sy = gp.sz = 4;
    unsigned long long* const acc_w = Acc[wave];

    for (int ch = blockIdx.x; ch < p.n_chunks; ch += gridDim.x) {
        const int64_t j0 = (int64_t)ch * kSbRows;
        // ---- the walk: this wave's rows of the chunk, one at a time (everything about the row is wave uniform)
        for (int rr = 0; rr < kSbRows / kSbWaves; ++rr) {
            const int row = wave + kSbWaves * rr;
            const int64_t j = j0 + row;
            int64_t rb = 0;
            int cnt = 0;
            float px = 0.0f, py = 0.0f, pz = 0.0f;
            if (j < p.n_inp) {
                px = p.inp_pos[3 * j]; py = p.inp_pos[3 * j + 1]; pz = p.inp_pos[3 * j + 2];
                rb = p.t_rs[j];
                const int64_t c64 = p.t_cnt ? (int64_t)p.t_cnt[j] : p.t_rs[j + 1] - rb;
                // (a row past the buffer counts as empty, as in the forward; so does a row that is no row at all)
                cnt = (rb >= 0 && c64 > 0 && c64 < ((int64_t)1 << 31) && rb + c64 <= p.t_cap) ? (int)c64 : 0;
            }
            for (int k0 = 0; k0 < cnt; k0 += 64) {
                const int k = k0 + lane;
                bool valid = k < cnt;
                int i = valid ? p.t_idx[rb + k] : 0;
                valid = valid && (unsigned)i < (unsigned)p.n_out;
                i = valid ? i : 0;
                const float qx = p.out_pos[3 * (int64_t)i], qy = p.out_pos[3 * (int64_t)i + 1], qz = p.out_pos[3 * (int64_t)i + 2];
                f32x4 g[COUT / 4];
#pragma unroll
                for (int q = 0; q < COUT / 4; ++q) g[q] = *(const f32x4*)(p.gout + (int64_t)i * COUT + 4 * q);
                float x = px - qx, y = py - qy, z = pz - qz;
                float a = p.window == DMCF_WINDOW_NONE ? 1.0f : window_value(DMCF_WINDOW_POLY6, rel_dist2(x, y, z), p.inv_r2, p.window_fac);
                a *= S;
                filter_coords<false>(x, y, z, gp);
                int bx, by, bz;
                float wx0, wx1, wy0, wy1, wz0, wz1;
                axis_weights_linear(x, 4, bx, wx0, wx1);
                axis_weights_linear(y, 4, by, wy0, wy1);
                axis_weights_linear(z, 4, bz, wz0, wz1);
                if (valid) {
                    unsigned long long* const tc = acc_w + ((bz * 4 + by) * 4 + bx) * COUT;
                    // corner weights in Open3D's product order (x-weight * y-weight) * z-weight, times the window (and 2^s)
#pragma unroll
                    for (int zz = 0; zz < 2; ++zz) {
                        const float wza = (zz ? wz1 : wz0) * a;
#pragma unroll
                        for (int yy = 0; yy < 2; ++yy)
#pragma unroll
                            for (int xx = 0; xx < 2; ++xx) {
                                const float w = ((xx ? wx1 : wx0) * (yy ? wy1 : wy0)) * wza;
                                unsigned long long* const t = tc + (zz * 16 + yy * 4 + xx) * COUT;
#pragma unroll
                                for (int o = 0; o < COUT; ++o) lds_add_i64(t + o, sct_fixed(w * g[o / 4][o % 4]));
                            }
                    }
                }
            }
            // the row's T as floats into the chunk's tile; the integers are cleared for the next row (LDS serves a wave's
            // instructions in order; the fences keep the compiler from moving the plain accesses across the atomics)
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
            __builtin_amdgcn_wave_barrier();
            for (int e = lane; e < GROW; e += 64) {
                const long long v = (long long)acc_w[e];
                acc_w[e] = 0ull;
                Tf[row * TROW + e] = (float)((double)v * inv_S);
            }
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
            __builtin_amdgcn_wave_barrier();
        }
        __syncthreads();  // T of the chunk is complete

        // ---- dF[16][cin] = T[16][GROW] . Wf^T: this wave's column tile over its half of K, two accumulator chains
        f32x4 d0 = (f32x4){0.0f, 0.0f, 0.0f, 0.0f}, d1 = d0;
        if (df_tile) {
            const float* tr = Tf + r16 * TROW + kbase + 4 * q4;
#pragma unroll
            for (int mb = 0; mb < KB; mb += 2) {
                const f32x4 a0 = *(const f32x4*)(tr + 16 * mb), a1 = *(const f32x4*)(tr + 16 * mb + 16);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    d0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[i], wb[mb][i], d0, 0, 0, 0);
                    d1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[i], wb[mb + 1][i], d1, 0, 0, 0);
                }
            }
            d0 += d1;
            // D layout: lane (r16, q4) holds rows 4 q4 + rr, column r16
            if (kh == 1) {
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) Dp[ct][4 * q4 + rr][r16] = d0[rr];
            }
        }
        // ---- dW partial [cin][GROW] += F^T[cin][16] . T[16][GROW]: A = F^T (lane: channel 16 mt + r16, row 4 kk + q4)
        if (p.partial) {
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                if (16 * mt < cin) {
                    float fa[4];
#pragma unroll
                    for (int kk = 0; kk < 4; ++kk) {
                        const int64_t j = j0 + 4 * kk + q4;
                        const int c = 16 * mt + r16;
                        fa[kk] = (j < p.n_inp && c < cin) ? p.inp_feat[j * cin + c] : 0.0f;
                    }
#pragma unroll
                    for (int tt = 0; tt < NTW; ++tt) {
                        const float* tcol = Tf + q4 * TROW + 16 * (wave * NTW + tt) + r16;
#pragma unroll
                        for (int kk = 0; kk < 4; ++kk)
                            dw[mt][tt] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[kk], tcol[4 * kk * TROW], dw[mt][tt], 0, 0, 0);
                    }
                }
            }
        }
        __syncthreads();  // every wave is done with T (the next walk overwrites it); the upper halves are in Dp
        if (df_tile && kh == 0) {
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int64_t j = j0 + 4 * q4 + rr;
                const int c = 16 * ct + r16;
                if (j < p.n_inp && c < cin) p.dfeat[j * cin + c] = d0[rr] + Dp[ct][4 * q4 + rr][r16];
            }
        }
        // (Dp is written again only behind the next chunk's first barrier, which the lower-half waves reach after these reads)
    }
    if (p.partial) {
        float* part = p.partial + (int64_t)blockIdx.x * cin * GROW;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int tt = 0; tt < NTW; ++tt)
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) {
                    const int c = 16 * mt + 4 * q4 + rr;
                    if (c < cin) part[(int64_t)c * GROW + 16 * (wave * NTW + tt) + r16] = dw[mt][tt][rr];
                }
    }
}

// dW[cell][c][o] = the workgroups' partials [c][cell * cout + o] added in workgroup order
__global__ __launch_bounds__(256) void sct_bwd_reduce(const float* __restrict__ partial, int groups, int cin, int cout, float* __restrict__ dW) {
    const int grow = 64 * cout, total = cin * grow;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    float s = 0.0f;
#pragma unroll 8
    for (int g = 0; g < groups; ++g) s += partial[(int64_t)g * total + t];
    const int c = t / grow, col = t - c * grow;
    dW[((int64_t)(col / cout) * cin + c) * cout + (col % cout)] = s;
}

static int sct_bwd_groups(int64_t n_inp) {
    return (int)std::min<int64_t>((n_inp + kSbRows - 1) / kSbRows, kSbMaxGroups);
}

// workspace: the partial filter gradients [groups][cin][64 cout] | 256 bytes ([0..1] the bound's two factors)
static size_t sct_bwd_partial_bytes(const dmcf_cconv_scatter_args* a, const dmcf_cconv_scatter_backward_args* b) {
    if (b && !b->grad_filters) return 0;
    return align_up((size_t)sct_bwd_groups(a->n_inp) * a->filter_dims[3] * 64 * a->filter_dims[4] * 4, 256);
}

static int sct_bwd_check(const dmcf_cconv_scatter_args* a, const dmcf_cconv_scatter_backward_args* b) {
    if (!a || !b) return DMCF_EINVAL;
    if (b->struct_size < sizeof(dmcf_cconv_scatter_backward_args) || b->flags != 0) return DMCF_EINVAL;
    if (!a->filters || !a->out_positions || !a->inp_positions || !a->inp_features || !a->t_index || !a->t_row_begin) return DMCF_EINVAL;
    if (!b->grad_out || (!b->grad_filters && !b->grad_inp_features)) return DMCF_EINVAL;
    if ((uintptr_t)b->grad_out & 15) return DMCF_EINVAL;  // (its rows are read 16 bytes at a time)
    if (a->n_out <= 0 || a->n_inp <= 0 || a->filter_dims[3] <= 0 || !(a->extent > 0.0f) || a->t_capacity < 0) return DMCF_EINVAL;
    if (a->filter_dims[0] != 4 || a->filter_dims[1] != 4 || a->filter_dims[2] != 4 || (a->filter_dims[4] != 4 && a->filter_dims[4] != 8) ||
        a->filter_dims[3] > 32)
        return DMCF_EUNSUPPORTED;
    if (a->window != DMCF_WINDOW_NONE && a->window != DMCF_WINDOW_POLY6) return DMCF_EUNSUPPORTED;
    if (a->flags & ~(DMCF_FLAG_ALIGN_CORNERS | DMCF_FLAG_ACCUMULATE)) return DMCF_EUNSUPPORTED;
    if (!(a->flags & DMCF_FLAG_ALIGN_CORNERS)) return DMCF_EUNSUPPORTED;
    if (a->n_out >= ((int64_t)1 << 31) || a->n_inp >= ((int64_t)1 << 31)) return DMCF_EUNSUPPORTED;
    return DMCF_OK;
}

static size_t sct_bwd_workspace_bytes(const dmcf_cconv_scatter_args* a, const dmcf_cconv_scatter_backward_args* b) {
    if (!a || a->n_inp <= 0 || a->filter_dims[3] <= 0 || a->filter_dims[3] > 32 || (a->filter_dims[4] != 4 && a->filter_dims[4] != 8)) return 0;
    return sct_bwd_partial_bytes(a, b) + 256;
}

static int sct_backward(const dmcf_cconv_scatter_args* a, const dmcf_cconv_scatter_backward_args* b, void* workspace, size_t workspace_bytes,
                        hipStream_t stream) {
    const int rc = sct_bwd_check(a, b);
    if (rc != DMCF_OK) return rc;
    if (workspace_bytes < sct_bwd_workspace_bytes(a, b)) return DMCF_EWORKSPACE;
    if (!workspace || ((uintptr_t)workspace & 255)) return DMCF_EINVAL;
    const int cin = a->filter_dims[3], cout = a->filter_dims[4];
    if (a->t_capacity == 0) {  // no pair, no gradient
        if (b->grad_filters && hipMemsetAsync(b->grad_filters, 0, (size_t)64 * cin * cout * 4, stream) != hipSuccess) return check_launch();
        if (b->grad_inp_features && hipMemsetAsync(b->grad_inp_features, 0, (size_t)a->n_inp * cin * 4, stream) != hipSuccess) return check_launch();
        return DMCF_OK;
    }
    const size_t part_bytes = sct_bwd_partial_bytes(a, b);
    uint32_t* bound = (uint32_t*)((char*)workspace + part_bytes);
    if (hipMemsetAsync(bound, 0, 256, stream) != hipSuccess) {
        check_launch();
        return DMCF_ELAUNCH;
    }
    const int64_t ng = a->n_out * cout;
    hipLaunchKernelGGL(sct_bwd_bound_kernel, dim3((unsigned)std::min<int64_t>((ng + 255) / 256, 1024)), dim3(256), 0, stream, b->grad_out, ng, bound);
    SctBwdParams p;
    p.W = a->filters;
    p.out_pos = a->out_positions;
    p.inp_pos = a->inp_positions;
    p.inp_feat = a->inp_features;
    p.t_idx = a->t_index;
    p.t_rs = a->t_row_begin;
    p.t_cnt = a->t_row_count;
    p.t_cap = a->t_capacity;
    p.gout = b->grad_out;
    p.bound = bound;
    p.partial = b->grad_filters ? (float*)workspace : nullptr;
    p.dfeat = b->grad_inp_features;
    p.n_out = a->n_out;
    p.n_inp = a->n_inp;
    p.n_chunks = (int)((a->n_inp + kSbRows - 1) / kSbRows);
    p.cin = cin;
    p.inv_extent = 1.0f / a->extent;
    const float radius = 0.5f * a->extent;
    p.inv_r2 = 1.0f / (radius * radius);
    p.window_fac = a->window_fac;
    p.window = a->window;
    const int groups = sct_bwd_groups(a->n_inp);
    if (cout == 4) hipLaunchKernelGGL(cconv_sct_bwd_kernel<4>, dim3(groups), dim3(64 * kSbWaves), 0, stream, p);
    else hipLaunchKernelGGL(cconv_sct_bwd_kernel<8>, dim3(groups), dim3(64 * kSbWaves), 0, stream, p);
    if (b->grad_filters)
        hipLaunchKernelGGL(sct_bwd_reduce, dim3((unsigned)((cin * 64 * cout + 255) / 256)), dim3(256), 0, stream, (const float*)workspace, groups, cin,
                           cout, b->grad_filters);
    return check_launch();
}
