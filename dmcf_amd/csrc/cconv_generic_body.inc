// Body of the generic LDS-splat CConv kernel (cconv.hip), included by its two entry points:
//   cconv_kernel<CC, GENERIC>  dmcf_cconv_forward: one extent for every row (p.inv_extent / p.inv_r2);
//   cconv_ext_kernel<CC>       dmcf_cconv_forward_extents: EXT, every output row takes its own extent from out_ext[row] --
//                              loaded once per row, before the pair loop.
// (An include rather than a shared __device__ function: called through one, the existing instantiations compiled to other
// code -- other registers, other blocks -- than they did as kernels of their own.)
// In scope at the include: CC, GENERIC, EXT (compile-time), p (CconvParams), out_ext ([n_out] or NULL).
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int KCp = p.KCp, cin = p.cin, cout = p.cout, PS = p.PS;
    float* Bt = smem;                                   // [TM][KCp]
    float* norm = Bt + p.bfloats;                       // [TM]
    float* stage = norm + TM + (size_t)wave * kStage;
    float* wst = stage;                                 // [64][kWStride]
    float* fst = stage + 64 * kWStride;                 // [64][kFStride]
    int* bst = (int*)(fst + 64 * kFStride);             // [64] base cell offset of the pair (floats into its B row)
    float* deadbase = norm + TM + (size_t)kWaves * kStage;  // [kThreads][2], only if a filter axis is 1
    // XCD-aware tile order: blocks b, b+8, b+16.. (same XCD) take consecutive tiles
    const int tile = (int)(blockIdx.x % 8) * p.tiles_per_xcd + (int)(blockIdx.x / 8);
    if (tile >= p.ntiles) return;
    const int64_t pt0 = (int64_t)tile * TM;
    const bool symmetric = (p.flags & DMCF_FLAG_SYMMETRIC) != 0;

    // Each wave owns two points of the tile, one per half-wave (h): rows wave and wave + 8 of B.
    const int h = lane >> 5, pl = lane & 31;
    const int pt = wave + kWaves * h;
    const int64_t i = pt0 + pt;
    const bool pt_valid = i < p.n_out;
    int64_t rb = 0, re = 0;
    float ox = 0.0f, oy = 0.0f, oz = 0.0f;
    float row_inv_extent = 0.0f, row_inv_r2 = 0.0f;  // (EXT only)
    if (pt_valid) {
        rb = p.rs[i];
        re = p.cnt ? rb + p.cnt[i] : p.rs[i + 1];
        if (re > p.pair_cap) re = rb;
        ox = p.out_pos[3 * i]; oy = p.out_pos[3 * i + 1]; oz = p.out_pos[3 * i + 2];
        if (EXT) {
            // the host's arithmetic of dmcf_cconv_forward for a scalar extent, per row; an extent that is not positive and
            // finite empties the row (the result is the bias)
            const float e = out_ext[i];
            if (!(e > 0.0f) || !isfinite(e)) re = rb;
            row_inv_extent = __fdiv_rn(1.0f, e);
            const float radius = __fmul_rn(0.5f, e);
            row_inv_r2 = __fdiv_rn(1.0f, __fmul_rn(radius, radius));
        }
    }
    const int cnt = (int)(re - rb);
    const int cnt_max = max(__builtin_amdgcn_readlane(cnt, 0), __builtin_amdgcn_readlane(cnt, 32));
    const int nbatch = (cnt_max + 31) / 32;
    float* Brow = Bt + (size_t)pt * KCp;

    // phase-2 lane role inside a half-wave: corner x 4 channel groups.  The corner bits of the lane can be (x, Z, y)
    // instead of (x, y, z): a 64-bit LDS store is served in groups of 16 lanes = 4 corners against 32 banks, and with a 4-wide
    // filter the +y corner is 32 floats away (same banks, a 2-way conflict on every store) while the +z corner is one
    // padded plane away (make_cfg puts it 16 banks off): grouping (x, z) makes the stores conflict free.
    constexpr int CPL = CC / 4;  // channels per lane (2 -> 64-bit read-modify-write, 1 -> 32-bit)
    const int lt = pl >> 2, c4 = pl & 3;
    // staged-weight index (bit0 x, bit1 y, bit2 z) of this lane's corner; make_cfg picks the grouping per filter shape
    const int t = p.zgroup ? ((lt & 1) | ((lt & 4) >> 1) | ((lt & 2) << 1)) : lt;
    const int tx = (t & 1) && p.sx >= 2, ty = ((t >> 1) & 1) && p.sy >= 2, tz = ((t >> 2) & 1) && p.sz >= 2;
    const int lane_off = tz * PS + (ty * p.sx + tx) * CC + c4 * CPL;  // this corner's offset from the base cell
    // a "+1" corner along an axis of size 1 has weight 0 and would alias the base cell: such lanes stay idle
    const bool lane_live = !(((t & 1) && p.sx < 2) || ((t & 2) && p.sy < 2) || ((t & 4) && p.sz < 2));

    f32x4 acc[kMaxNT];
    #pragma unroll
    for (int n = 0; n < kMaxNT; ++n) acc[n] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};

    if (tid < TM) norm[tid] = 0.0f;
    const int mi = lane & 15, mg = lane >> 4;  // MFMA roles: A row / B column index, k index

    for (int chunk = 0; chunk < p.nchunks; ++chunk) {
        const int c0 = chunk * CC;
        for (int e = tid * 4; e < TM * KCp; e += kThreads * 4) *(f32x4*)(Bt + e) = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
        __syncthreads();
        // ---------------- splat ----------------
        float fi[CC];
    #pragma unroll
        for (int u = 0; u < CC; ++u)
            fi[u] = (symmetric && pt_valid && c0 + u < cin) ? p.inp_feat[i * cin + c0 + u] : 0.0f;
        float nsum = 0.0f;
        // Software pipeline over batches of 32 neighbours per half-wave: the (index, distance) loads run two
        // batches ahead and the dependent (position, feature) gathers one batch ahead of the splat that
        // consumes them, so the ~2 us index -> gather latency chain overlaps the LDS-bound phase 2.
        auto load_idx = [&](int bi, int& j, f32x4& g, int& gb, bool& valid) {
            const int64_t pp = rb + 32 * (int64_t)bi + pl;
            valid = pp < re;
            j = 0;
            gb = 0;
            g = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
            if (valid) {
                j = p.idx[pp];
                if (p.nval) g.w = p.nval[pp];
            }
        };
        auto gather = [&](int j, bool valid, float& px, float& py, float& pz, float (&f)[CC]) {
            px = py = pz = 0.0f;
    #pragma unroll
            for (int u = 0; u < CC; ++u) f[u] = 0.0f;
            if (valid) {
                const float* fp = p.inp_feat + (int64_t)j * cin + c0;
                if ((cin & 3) == 0) {  // rows are 16-byte aligned: vector gathers
    #pragma unroll
                    for (int u = 0; u < CC; u += 4) {
                        if (c0 + u < cin) {
                            const f32x4 v = *(const f32x4*)(fp + u);
                            f[u] = v.x; f[u + 1] = v.y; f[u + 2] = v.z; f[u + 3] = v.w;
                        }
                    }
                } else {
    #pragma unroll
                    for (int u = 0; u < CC; ++u)
                        if (c0 + u < cin) f[u] = fp[u];
                }
                px = p.inp_pos[3 * (int64_t)j];
                py = p.inp_pos[3 * (int64_t)j + 1];
                pz = p.inp_pos[3 * (int64_t)j + 2];
            }
        };
        int jA, jB, gbA, gbB;
        f32x4 gA, gB;
        bool vA, vB;
        load_idx(0, jA, gA, gbA, vA);
        load_idx(1, jB, gB, gbB, vB);
        float gx, gy, gz, gf[CC];
        gather(jA, vA, gx, gy, gz, gf);
        for (int bi = 0; bi < nbatch; ++bi) {
            // issue the loads of the following batches first
            float nx, ny, nz, nf[CC];
            gather(jB, vB, nx, ny, nz, nf);
            int jC, gbC;
            f32x4 gC;
            bool vC;
            load_idx(bi + 2, jC, gC, gbC, vC);
            // ---- phase 1: one lane per neighbour, 32 neighbours of each of the wave's two points
            int np_h = cnt - 32 * bi;  // pairs of this half in the batch (may be <= 0)
            np_h = min(max(np_h, 0), 32);
            int base = 0;
            {
                float a = 0.0f;
                int bx = 0, by = 0, bz = 0;
                float wx0 = 1.0f, wx1 = 0.0f, wy0 = 1.0f, wy1 = 0.0f, wz0 = 1.0f, wz1 = 0.0f;
                float x = 0.0f, y = 0.0f, z = 0.0f;
                if (vA) {
                    x = gx - ox;
                    y = gy - oy;
                    z = gz - oz;
                    a = window_value(p.window, p.nval ? gA.w : rel_dist2(x, y, z), EXT ? row_inv_r2 : p.inv_r2, p.window_fac);
                    nsum += a;
                    if (p.inp_imp) a *= p.inp_imp[jA];
                    filter_coords<GENERIC>(x, y, z, p, EXT ? row_inv_extent : p.inv_extent);
                }
                if (GENERIC) {
                    axis_weights(x, p.sx, p.interp, bx, wx0, wx1);
                    axis_weights(y, p.sy, p.interp, by, wy0, wy1);
                    axis_weights(z, p.sz, p.interp, bz, wz0, wz1);
                } else {
                    axis_weights_linear(x, p.sx, bx, wx0, wx1);
                    axis_weights_linear(y, p.sy, by, wy0, wy1);
                    axis_weights_linear(z, p.sz, bz, wz0, wz1);
                }
        
                base = bz * PS + (by * p.sx + bx) * CC;
                bst[lane] = base;
                // corner weights in Open3D's product order (x-weight * y-weight) * z-weight
                const float w00 = wx0 * wy0, w10 = wx1 * wy0, w01 = wx0 * wy1, w11 = wx1 * wy1;
                // the two float4 halves of a pair's weights swap places every 4 lanes: conflict-free b128 stores
                float* wr = wst + lane * kWStride;
                const int wsw = (lane >> 2) & 1;
                *(f32x4*)(wr + 4 * wsw) = (f32x4){w00 * wz0, w10 * wz0, w01 * wz0, w11 * wz0};
                *(f32x4*)(wr + 4 * (wsw ^ 1)) = (f32x4){w00 * wz1, w10 * wz1, w01 * wz1, w11 * wz1};
                float* fr = fst + lane * kFStride;
                if (symmetric && vA) {
    #pragma unroll
                    for (int u = 0; u < CC; ++u) gf[u] += fi[u];
                }
    #pragma unroll
                for (int u = 0; u < CC; u += 4)  // same half swap as the weights (CC = 8): conflict-free b128 stores
                    *(f32x4*)(fr + (CC == 8 ? (u ^ (4 * wsw)) : u)) = (f32x4){gf[u] * a, gf[u + 1] * a, gf[u + 2] * a, gf[u + 3] * a};
            }
            // The staging area is private to this wave and LDS operations of one wave are processed in
            // order, so no barrier is needed between the phases.
            // ---- phase 2: per half-wave lanes = (corner, channel group); both points advance together.
            // Plain read-modify-write instead of ds_add_f32: the LDS float atomic retires ~1 lane per
            // 3 clocks on gfx950 (measured ~200 clk per 64-lane instruction).  Race free: a row of B
            // belongs to one half-wave, the active lanes of a half hit distinct addresses (8 distinct
            // cells x channels; lanes whose "+1" cell collapses onto the base cell because that filter
            // axis has size 1 carry weight 0 and are parked on a private slot), and the two halves work
            // on two rows.  Branch-free body: slots beyond a half's pair count hold zero features
            // (phase 1 wrote f*a = 0 and a valid base cell for them), so they add 0.
            const int nq = max(__builtin_amdgcn_readlane(np_h, 0), __builtin_amdgcn_readlane(np_h, 32));
            // Groups of 8 slots, fully unrolled: the half-swap of the staging layout has period 8, so every staging
            // address is a loop-carried lane pointer + an immediate; the base cell comes from the staging area with
            // one broadcast read (it used to take 2 v_readlane + 2 v_mov + v_cndmask per pair of pairs) and the only
            // VALU work left per iteration is one address add, the multiply and the add of the read-modify-write.
            // Slots beyond a half's pair count hold zero features and a valid base cell: a group may run past nq.
            const float* wq0 = wst + (32 * h) * kWStride + t;        // slots with (q >> 2) even
            const float* wq1 = wst + (32 * h) * kWStride + (t ^ 4);  // ... odd
            const float* fq0 = fst + (32 * h) * kFStride + (CPL == 2 ? c4 * 2 : c4);
            const float* fq1 = fst + (32 * h) * kFStride + (CPL == 2 ? ((c4 * 2) ^ 4) : c4);
            const int* bq = bst + 32 * h;
            float* const brow = Brow + lane_off;
            float* const dead = deadbase + 2 * tid;
            auto splat8 = [&](auto all_live_tag) {
                constexpr bool ALL_LIVE = decltype(all_live_tag)::value;
                for (int q0 = 0; q0 < nq; q0 += 8) {
    #pragma unroll
                    for (int g = 0; g < 2; ++g) {  // g = (q >> 2) & 1 selects the swapped staging halves
                        const float* wq = g ? wq1 : wq0;
                        const float* fq = g ? fq1 : fq0;
                        // staging reads of four pairs first (they never alias B), then the four dependent read-modify-writes
                        float w[4];
                        int boff[4];
                        f32x2 fv2[4];
                        float fv1[4];
    #pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            const int q = q0 + 4 * g + u;
                            w[u] = wq[q * kWStride];
                            boff[u] = bq[q];
                            if constexpr (CPL == 2)
                                fv2[u] = *(const f32x2*)(fq + q * kFStride);
                            else
                                fv1[u] = fq0[q * kFStride];
                        }
    #pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            float* d = (ALL_LIVE || lane_live) ? brow + boff[u] : dead;
                            if constexpr (CPL == 2) {
                                f32x2* dst = (f32x2*)d;
                                f32x2 o = *dst;
                                o.x += w[u] * fv2[u].x;
                                o.y += w[u] * fv2[u].y;
                                *dst = o;
                            } else {
                                *d = *d + w[u] * fv1[u];
                            }
                        }
                    }
                }
            };
            if (p.sx >= 2 && p.sy >= 2 && p.sz >= 2)  // 3-D filters: every corner lane is live
                splat8(std::true_type{});
            else
                splat8(std::false_type{});
            // rotate the pipeline registers
            jA = jB; gA = gB; gbA = gbB; vA = vB;
            jB = jC; gB = gC; gbB = gbC; vB = vC;
            gx = nx; gy = ny; gz = nz;
    #pragma unroll
            for (int u = 0; u < CC; ++u) gf[u] = nf[u];
        }
        if (chunk == 0 && (p.flags & DMCF_FLAG_NORMALIZE)) {
    #pragma unroll
            for (int d = 16; d >= 1; d >>= 1) nsum += __shfl_xor(nsum, d, 64);
            if (pl == 0 && pt_valid) norm[pt] = nsum;
        }
        __syncthreads();
        // ---------------- contraction of this channel chunk on the matrix cores ----------------
        // out[16 x 16*NT] += B[16 x KC] * Wp_chunk[KC x 16*NT], k blocks of 16 dealt round-robin to the waves
        const float* Wc = p.Wp + (size_t)chunk * p.nblocks * (4 * p.NT * 16 * 4);
        for (int blk = wave; blk < p.nblocks; blk += kWaves) {
            const f32x4 av = *(const f32x4*)(Bt + (size_t)mi * KCp + blk * 16 + mg * 4);
            const float* wb = Wc + ((size_t)(blk * 4 + mg) * p.NT * 16 + mi) * 4;
    #pragma unroll
            for (int n = 0; n < kMaxNT; ++n) {
                if (n < p.NT) {
                    const f32x4 bv = *(const f32x4*)(wb + n * 64);
                    acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, bv.x, acc[n], 0, 0, 0);
                    acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, bv.y, acc[n], 0, 0, 0);
                    acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, bv.z, acc[n], 0, 0, 0);
                    acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, bv.w, acc[n], 0, 0, 0);
                }
            }
        }
        __syncthreads();
    }

    // ---------------- cross-wave reduction + epilogue ----------------
    // D layout of 16x16x4: lane l, reg r -> row (point) 4*(l>>4)+r, column (channel) l&15
    float* red = Bt;  // [kWaves][TM][16*NT]  (B is dead now; 8*16*64*4 = 32 KiB at most)
    const int ncol = 16 * p.NT;
    #pragma unroll
    for (int n = 0; n < kMaxNT; ++n) {
        if (n < p.NT) {
    #pragma unroll
            for (int r = 0; r < 4; ++r)
                red[((size_t)wave * TM + 4 * mg + r) * ncol + n * 16 + mi] = acc[n][r];
        }
    }
    __syncthreads();
    for (int e = tid; e < TM * cout; e += kThreads) {
        const int ptt = e / cout, o = e % cout;
        const int64_t ii = pt0 + ptt;
        if (ii >= p.n_out) continue;
        float v = 0.0f;
    #pragma unroll
        for (int w = 0; w < kWaves; ++w) v += red[((size_t)w * TM + ptt) * ncol + o];
        if (p.flags & DMCF_FLAG_NORMALIZE) {
            const float nv = norm[ptt];
            if (nv != 0.0f) v /= nv;
        }
        if (p.bias) v += p.bias[o];
        float* dst = p.out + ii * cout + o;
        if (p.flags & DMCF_FLAG_ACCUMULATE) v += *dst;
        *dst = v;
    }
