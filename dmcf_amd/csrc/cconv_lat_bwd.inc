// Backward of the lattice form (dmcf_lattice_conv_backward; included by cconv_lat.hip, inside namespace dmcf, so that it
// differentiates the forward's own operands: the packed per-offset matrices W_d of lat_build_filters, the compacted row list
// of lat_rows_*, the geometry of lat_offset_taps).  With out_i = sum_d W_d^T f_{cell(i) + d}:
//
//   filter gradient   dW_d = sum_i f_{cell(i) + d} (x) G_i          lat_bwd_filter: per SLAB of kLatSlab rows of the list and
//                                                                   16 offsets one wave, v_mfma_f32_16x16x4_f32 with
//                                                                   M = 16 offsets of one input channel, N = 16 output channels,
//                                                                   K = 4 consecutive rows; its sum goes to the slab's own buffer
//                     dW[cell_t] += window(d) w_t(d) dW_d           lat_bwd_reduce adds the slabs in slab order, lat_bwd_fold
//                                                                   gathers per filter element over parts and offsets in order
//   input gradient    df_v = sum_d W_d G_{row of out cell (v - d)}  lat_bwd_input: tile = 16 cells of the VOLUME (one residue
//                                                                   class of the cells modulo inp_step, so that all 16 share a
//                                                                   sub-stencil), N = input channels, K = 4 offsets of one
//                                                                   output channel; a gather, every cell written once
//
// No float atomics anywhere: every sum has one owner and a fixed order, two calls return the same bits.
constexpr int kLatSlab = 1024;     // rows of the list whose filter-gradient sum one workgroup forms (tests state this number)
constexpr int kLatSlabChunk = 256; // ... staged through LDS this many rows at a time
constexpr int kLatClsHead = 16;    // ints in front of a part's class-sorted offset list: the first position of each class

struct LatBwd {
    const float* gout;   // [n_out][cout]
    int64_t n_out;
    int cin, cout, C, NT, N16;  // C = channels of a volume cell (= cin), N16 = 16 NT
    int Smax;                   // most offsets of any part
    // filter gradient
    float* partial;      // [slab][Smax][C][N16]
    float* red;          // [part][Smax][C][N16]
    int32_t* tcell;      // [part][Smax][8]: filter cell of each trilinear corner, -1: weight 0
    float* tw;           // [part][Smax][8]
    float* ta;           // [part][Smax]: window value
    int64_t dw_stride;   // Smax C N16
    // input gradient
    float* gp;           // [n_out + 1][coutp]: grad_out padded to whole 16-byte pieces, the last row zeros
    int coutp;
    int32_t* cls;        // [part][cls_stride]: kLatClsHead ints, then the offsets' indices sorted by residue class (-1: padding)
    int cls_stride;
    float* wt;           // [part][group of 4 sorted offsets][coutp][64]: lane (q, c) holds W_d[c][o] -- W_d^T as the B operand
    int64_t wt_stride;
    int step, nclass;
    int umin[3], udim[3]; // the volume's cells are v = step u + r, u in this box, r the residue class
    int tiles_x2;         // pairs of 16-cell tiles along x
    int64_t units;        // nclass * udim z * udim y * tiles_x2: one wave each
    float* gvol;
};

__device__ __forceinline__ int lat_first_rowb(const LatParams& p) {  // a cell every launch may read: padding rows use it
    return (((p.amin[2] * p.inp_step - p.imin[2]) * p.idim[1] + (p.amin[1] * p.inp_step - p.imin[1])) * p.idim[0] +
            (p.amin[0] * p.inp_step - p.imin[0])) * p.cin * 4;
}

// slab `sl` of the call: its part, first row and the end of the part's rows (false: past the last slab)
__device__ __forceinline__ bool lat_slab(const LatBatch& b, int64_t sl, int& part, int64_t& row0, int64_t& rend) {
    int64_t first = 0;
    for (int i = 0; i < b.n; ++i) {
        const int64_t ns = (b.count[i] + kLatSlab - 1) / kLatSlab;
        if (sl < first + ns) {
            part = i;
            row0 = b.start[i] + (sl - first) * kLatSlab;
            rend = b.start[i] + b.count[i];
            return true;
        }
        first += ns;
    }
    return false;
}

// grid (slabs, y): the waves of workgroup (sl, y) take the groups of 16 offsets 4 y + wave, + 4 gridDim.y, ...
template <int NTT, int KST>
__global__ __launch_bounds__(256) void lat_bwd_filter(const LatBatch b, const LatBwd q) {
    __shared__ __attribute__((aligned(16))) float Gs[kLatSlabChunk / 4][NTT][64];  // grad_out rows as B fragments (k = row, n = channel)
    __shared__ int rowbs[kLatSlabChunk], oidxs[kLatSlabChunk];
    int part;
    int64_t row0, rend;
    if (!lat_slab(b, blockIdx.x, part, row0, rend)) return;
    const LatParams& p = b.part[part];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int m = lane & 15, k = lane >> 4;
    constexpr int C = 4 * KST;
    const int SG = (p.S + 15) / 16;
    const int64_t send = min(rend, row0 + kLatSlab);
    float* dst = q.partial + (int64_t)blockIdx.x * q.dw_stride;
    for (int og0 = blockIdx.y * 4; og0 < SG; og0 += 4 * gridDim.y) {
        const int og = og0 + wave;
        const bool active = og < SG;  // (the whole wave agrees; idle waves still stage and meet the barriers)
        int dof = 0;
        if (active) {
            const int32_t* d = p.stencil + 4 * min(16 * og + m, p.S - 1);  // offsets past S repeat the last one, never stored
            dof = ((d[2] * p.idim[1] + d[1]) * p.idim[0] + d[0]) * p.cin * 4;
        }
        f32x4 acc[C][NTT];
#pragma unroll
        for (int c = 0; c < C; ++c)
#pragma unroll
            for (int n = 0; n < NTT; ++n) acc[c][n] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
        for (int64_t base = row0; base < send; base += kLatSlabChunk) {
            __syncthreads();  // the previous chunk has been read
            {
                const int64_t e = base + threadIdx.x;
                lat_i32x2 rw = (lat_i32x2){lat_first_rowb(p), -1};
                if (e < send) rw = b.rows[e];
                rowbs[threadIdx.x] = rw.x;
                oidxs[threadIdx.x] = rw.y;
            }
            __syncthreads();
            for (int e = threadIdx.x; e < kLatSlabChunk / 4 * NTT * 64; e += 256) {
                const int l = e & 63, n = (e >> 6) % NTT, j = (e >> 6) / NTT;
                const int oi = oidxs[4 * j + (l >> 4)], o = 16 * n + (l & 15);
                Gs[j][n][l] = (oi >= 0 && o < q.cout) ? q.gout[(int64_t)oi * q.cout + o] : 0.0f;
            }
            __syncthreads();
            if (!active) continue;
            const int nj = (int)((min((int64_t)kLatSlabChunk, send - base) + 3) / 4);
            for (int j = 0; j < nj; ++j) {
                // lane (m, k): the cell of row 4 j + k at offset m of the group; the volume holds it (checked on the host)
                const f32x4* src = (const f32x4*)((const char*)p.vol + (size_t)(uint32_t)(rowbs[4 * j + k] + dof));
                f32x4 f[KST];
#pragma unroll
                for (int ks = 0; ks < KST; ++ks) f[ks] = src[ks];
#pragma unroll
                for (int n = 0; n < NTT; ++n) {
                    const float g = Gs[j][n][lane];
#pragma unroll
                    for (int c = 0; c < C; ++c) acc[c][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(f[c >> 2][c & 3], g, acc[c][n], 0, 0, 0);
                }
            }
        }
        if (!active) continue;
        // D layout: lane (4 k + r = offset of the group, m = output channel of the tile)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int s = 16 * og + 4 * k + r;
            if (s >= p.S) continue;
#pragma unroll
            for (int c = 0; c < C; ++c)
#pragma unroll
                for (int n = 0; n < NTT; ++n) dst[((int64_t)s * C + c) * q.N16 + 16 * n + m] = acc[c][n][r];
        }
    }
}

// grid (x, parts): red[part][e] = sum over the part's slabs, in slab order
__global__ __launch_bounds__(256) void lat_bwd_reduce(const LatBatch b, const LatBwd q) {
    const int part = blockIdx.y;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)b.part[part].S * q.C * q.N16) return;
    int64_t first = 0;
    for (int i = 0; i < part; ++i) first += (b.count[i] + kLatSlab - 1) / kLatSlab;
    const int64_t ns = (b.count[part] + kLatSlab - 1) / kLatSlab;
    float v = 0.0f;
    for (int64_t s = 0; s < ns; ++s) v += q.partial[(first + s) * q.dw_stride + e];
    q.red[(int64_t)part * q.dw_stride + e] = v;
}

// grid (x, parts): the eight filter cells and weights of every offset, as lat_build_filters reads them
struct LatTapArgs {
    CconvParams cp[kLatMaxParts];
    float voxel[kLatMaxParts][3], shift[kLatMaxParts][3];
};
__global__ __launch_bounds__(256) void lat_bwd_taps(const LatBatch b, const LatBwd q, const LatTapArgs t) {
    const int part = blockIdx.y, s = blockIdx.x * 256 + threadIdx.x;
    if (s >= b.part[part].S) return;
    const CconvParams& p = t.cp[part];
    const LatTaps g = lat_offset_taps(b.part[part].stencil, s, p, t.voxel[part][0], t.voxel[part][1], t.voxel[part][2], t.shift[part][0],
                                      t.shift[part][1], t.shift[part][2]);
    const int64_t at = (int64_t)part * q.Smax + s;
    q.ta[at] = g.a;
    for (int iz = 0; iz < 2; ++iz)
        for (int iy = 0; iy < 2; ++iy)
            for (int ix = 0; ix < 2; ++ix) {
                const float w = g.wz[iz] * g.wy[iy] * g.wx[ix];
                const int cz = min(g.bz + iz, p.sz - 1), cy = min(g.by + iy, p.sy - 1), cx = min(g.bx + ix, p.sx - 1);
                const int tap = (iz * 2 + iy) * 2 + ix;
                q.tcell[at * 8 + tap] = w == 0.0f ? -1 : (cz * p.sy + cy) * p.sx + cx;
                q.tw[at * 8 + tap] = w;
            }
}

// one thread per element of grad_filters: the transpose of lat_build_filters, parts and offsets in ascending order
__global__ __launch_bounds__(256) void lat_bwd_fold(const LatBatch b, const LatBwd q, float* __restrict__ gw, int64_t total) {
    typedef int i32x4 __attribute__((ext_vector_type(4)));
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int o = (int)(e % q.cout), c = (int)(e / q.cout % q.cin), cell = (int)(e / ((int64_t)q.cout * q.cin));
    float v = 0.0f;
    for (int part = 0; part < b.n; ++part) {
        if (b.count[part] == 0) continue;  // (nothing was reduced for a part without rows)
        const int64_t at0 = (int64_t)part * q.Smax;
        const float* red = q.red + (int64_t)part * q.dw_stride + (int64_t)c * q.N16 + o;
        for (int s = 0; s < b.part[part].S; ++s) {
            const i32x4 c0 = *(const i32x4*)(q.tcell + (at0 + s) * 8), c1 = *(const i32x4*)(q.tcell + (at0 + s) * 8 + 4);
            const f32x4 w0 = *(const f32x4*)(q.tw + (at0 + s) * 8), w1 = *(const f32x4*)(q.tw + (at0 + s) * 8 + 4);
            float w = 0.0f;
            bool hit = false;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                if (c0[t] == cell) { w += w0[t]; hit = true; }
                if (c1[t] == cell) { w += w1[t]; hit = true; }
            }
            if (hit) v += w * (q.ta[at0 + s] * red[(int64_t)s * q.C * q.N16]);
        }
    }
    gw[e] = v;
}

// gp[row][o] = grad_out[row][o], rows of coutp floats, row n_out zeros
__global__ __launch_bounds__(256) void lat_bwd_pad(const LatBwd q) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (q.n_out + 1) * q.coutp) return;
    const int64_t row = e / q.coutp;
    const int o = (int)(e % q.coutp);
    q.gp[e] = (row < q.n_out && o < q.cout) ? q.gout[row * q.cout + o] : 0.0f;
}

// Residue class of an offset modulo the input step (step 1: one class; step 2: the eight parities).  An input cell v = step u + r
// is reached through the offsets of class r alone: (v - d) / step must be a whole base vector.
__device__ __forceinline__ int lat_class(const int32_t* d, int step) {
    const int mk = step - 1;  // step is 1 or 2
    return (((d[2] & mk) * step) + (d[1] & mk)) * step + (d[0] & mk);
}

// one wave per part: the offsets' indices sorted by class (stable), every class padded to whole groups of 4
__global__ __launch_bounds__(64) void lat_bwd_classes(const LatBatch b, const LatBwd q) {
    const LatParams& p = b.part[blockIdx.x];
    int32_t* head = q.cls + (int64_t)blockIdx.x * q.cls_stride;
    int32_t* list = head + kLatClsHead;
    const int lane = threadIdx.x;
    int at = 0;
    for (int r = 0; r < q.nclass; ++r) {
        if (lane == 0) head[r] = at;
        for (int s0 = 0; s0 < p.S; s0 += 64) {
            const int s = s0 + lane;
            const bool mine = s < p.S && lat_class(p.stencil + 4 * s, q.step) == r;
            const uint64_t mk = __ballot(mine);
            if (mine) list[at + __popcll(mk & ((1ull << lane) - 1ull))] = s;
            at += __popcll(mk);
        }
        const int pad = (4 - (at & 3)) & 3;
        if (lane < pad) list[at + lane] = -1;
        at += pad;
    }
    if (lane == 0) head[q.nclass] = at;
}

// grid (x, parts): W_d^T of the sorted offsets in B-fragment order, from the forward's packed matrices (its bits)
__global__ __launch_bounds__(256) void lat_bwd_wt(const LatBatch b, const LatBwd q) {
    const int part = blockIdx.y;
    const LatParams& p = b.part[part];
    const int32_t* head = q.cls + (int64_t)part * q.cls_stride;
    const int64_t total = (int64_t)(head[q.nclass] / 4) * q.coutp * 64;
    float* wt = q.wt + (int64_t)part * q.wt_stride;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int l = (int)(e & 63), o = (int)((e >> 6) % q.coutp);
        const int64_t g = (e >> 6) / q.coutp;
        const int s = head[kLatClsHead + 4 * g + (l >> 4)], c = l & 15;
        float v = 0.0f;
        if (s >= 0 && c < q.cin && o < q.cout) v = p.Wp[(((int64_t)(s >> 2) * q.C + c) * p.NT + (o >> 4)) * 64 + (s & 3) * 16 + (o & 15)];
        wt[e] = v;
    }
}

// One wave per pair of 16-cell tiles of the volume (cells of one residue class, consecutive along x in units of the step).
// Per part and group of 4 offsets of the class: lane (m, k) finds the output row that reaches cell m through offset k -- base
// vector a = u - (d - r) / step inside the part's box, output cell a * out_stride + phase in the table -- and loads its padded
// grad_out row (the zero row if there is none); register o of that load is the A operand for output channel o.
template <int KQ>
__global__ __launch_bounds__(256) void lat_bwd_input(const LatBatch b, const LatBwd q) {
    typedef int i32x4 __attribute__((ext_vector_type(4)));
    const int lane = threadIdx.x & 63;
    const int m = lane & 15, k = lane >> 4;
    const int64_t unit = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (unit >= q.units) return;
    const int xb2 = (int)(unit % q.tiles_x2);
    int64_t t_ = unit / q.tiles_x2;
    const int uy = q.umin[1] + (int)(t_ % q.udim[1]); t_ /= q.udim[1];
    const int uz = q.umin[2] + (int)(t_ % q.udim[2]);
    const int r = (int)(t_ / q.udim[2]);
    const int step = q.step;
    const int rx = r % step, ry = r / step % step, rz = r / (step * step);
    const LatParams& p0 = b.part[0];  // (all parts share the volume)
    const int vy = step * uy + ry - p0.imin[1], vz = step * uz + rz - p0.imin[2];  // volume coordinates of the tiles' cells
    if ((unsigned)vy >= (unsigned)p0.idim[1] || (unsigned)vz >= (unsigned)p0.idim[2]) return;
    const int ux0 = q.umin[0] + xb2 * 32;
    f32x4 acc[2] = {(f32x4){0.0f, 0.0f, 0.0f, 0.0f}, (f32x4){0.0f, 0.0f, 0.0f, 0.0f}};
    for (int part = 0; part < b.n; ++part) {
        const LatParams& p = b.part[part];
        if (b.count[part] == 0) continue;
        const int32_t* head = q.cls + (int64_t)part * q.cls_stride;
        const float* wt = q.wt + (int64_t)part * q.wt_stride;
        for (int pos = head[r]; pos < head[r + 1]; pos += 4) {
            const int s = head[kLatClsHead + pos + k];
            const i32x4 d = *(const i32x4*)(p.stencil + 4 * max(s, 0));
            // (d - r is a multiple of the step for the offsets of class r)
            const int ay = uy - (d.y - ry) / step - p.amin[1], az = uz - (d.z - rz) / step - p.amin[2];
            const int oy = (ay + p.amin[1]) * p.out_stride + p.phase[1] - p.omin[1], oz = (az + p.amin[2]) * p.out_stride + p.phase[2] - p.omin[2];
            const bool okyz = s >= 0 && (unsigned)ay < (unsigned)p.adim[1] && (unsigned)az < (unsigned)p.adim[2] &&
                              (unsigned)oy < (unsigned)p.odim[1] && (unsigned)oz < (unsigned)p.odim[2];
            int64_t row[2];
            bool any = false;
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int ax = ux0 + 16 * t + m - (d.x - rx) / step - p.amin[0];
                const int ox = (ax + p.amin[0]) * p.out_stride + p.phase[0] - p.omin[0];
                int oi = -1;
                if (okyz && (unsigned)ax < (unsigned)p.adim[0] && (unsigned)ox < (unsigned)p.odim[0])
                    oi = p.otab[((int64_t)oz * p.odim[1] + oy) * p.odim[0] + ox];
                any |= oi >= 0;
                row[t] = oi >= 0 ? oi : q.n_out;
            }
            if (__ballot(any) == 0) continue;  // no output row reaches these 32 cells through these 4 offsets
            f32x4 g[2][KQ];
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int j = 0; j < KQ; ++j) g[t][j] = *(const f32x4*)(q.gp + row[t] * q.coutp + 4 * j);
            const float* w = wt + (int64_t)(pos >> 2) * q.coutp * 64 + lane;
#pragma unroll
            for (int o = 0; o < 4 * KQ; ++o) {
                const float wv = w[o * 64];
#pragma unroll
                for (int t = 0; t < 2; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(g[t][o >> 2][o & 3], wv, acc[t], 0, 0, 0);
            }
        }
    }
    // D layout: lane (cell 4 k + i of the tile, column m = input channel)
    if (m >= q.cin) return;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int vx = step * (ux0 + 16 * t + 4 * k + i) + rx - p0.imin[0];
            if ((unsigned)vx >= (unsigned)p0.idim[0]) continue;
            q.gvol[(((int64_t)vz * p0.idim[1] + vy) * p0.idim[0] + vx) * q.cin + m] = acc[t][i];
        }
}

static inline int64_t lat_floor_div(int64_t a, int64_t b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

static_assert(sizeof(LatBatch) + sizeof(LatBwd) + sizeof(LatTapArgs) < 4000, "kernel arguments of lat_bwd_taps");

struct LatBwdLayout {
    LatLayout F;  // the forward's workspace comes first
    size_t off_gp, off_cls, off_wt, off_partial, off_red, off_tcell, off_tw, off_ta, total;
    int coutp, Smax, cls_stride;
    int64_t wt_stride, dw_stride, max_slabs;
};

static LatBwdLayout lat_bwd_layout(const dmcf_lattice_conv_args* parts, int n_parts) {
    LatBwdLayout B;
    B.F = lat_layout(parts, n_parts);
    const int cin = parts[0].filter_dims[3], cout = parts[0].filter_dims[4];
    const int kq = (cout + 3) / 4;
    B.coutp = 4 * (kq <= 2 ? kq : kq <= 4 ? 4 : kq <= 6 ? 6 : 8);  // (the instantiations of lat_bwd_input)
    B.Smax = 0;
    for (int i = 0; i < n_parts; ++i) B.Smax = std::max(B.Smax, (int)parts[i].n_offsets);
    const int step = parts[0].inp_step, nclass = step * step * step;
    const int cap = (B.Smax + 3) / 4 * 4 + 4 * nclass;  // every class padded to whole groups of 4
    B.cls_stride = kLatClsHead + cap;
    B.wt_stride = (int64_t)(cap / 4) * B.coutp * 64;
    B.dw_stride = (int64_t)B.Smax * cin * ((cout + 15) / 16 * 16);
    B.max_slabs = B.F.rows_capacity / kLatSlab + n_parts + 1;
    size_t off = align_up(B.F.total, 256);
    B.off_gp = off;       off += align_up((size_t)(parts[0].n_out + 1) * B.coutp * 4, 256);
    B.off_cls = off;      off += align_up((size_t)n_parts * B.cls_stride * 4, 256);
    B.off_wt = off;       off += align_up((size_t)n_parts * B.wt_stride * 4, 256);
    B.off_partial = off;  off += align_up((size_t)B.max_slabs * B.dw_stride * 4, 256);
    B.off_red = off;      off += align_up((size_t)n_parts * B.dw_stride * 4, 256);
    B.off_tcell = off;    off += align_up((size_t)n_parts * B.Smax * 8 * 4, 256);
    B.off_tw = off;       off += align_up((size_t)n_parts * B.Smax * 8 * 4, 256);
    B.off_ta = off;       off += align_up((size_t)n_parts * B.Smax * 4, 256);
    B.total = off;
    return B;
}

// The parts as the forward's checks want them: the backward reads no bias and no out, and never accumulates.
static int lat_bwd_parts(const dmcf_lattice_conv_args* parts, int n_parts, dmcf_lattice_conv_args* own) {
    if (!parts || n_parts < 1 || n_parts > kLatMaxParts) return DMCF_EINVAL;
    for (int i = 0; i < n_parts; ++i) {
        own[i] = parts[i];
        own[i].bias = nullptr;
        own[i].out = (float*)(uintptr_t)256;  // (never dereferenced; the forward's validation asks for one)
        own[i].flags &= ~DMCF_FLAG_ACCUMULATE;
    }
    const int rc = lat_check(own, n_parts);
    if (rc != DMCF_OK) return rc;
    for (int i = 1; i < n_parts; ++i) {
        const dmcf_lattice_conv_args &a = own[i], &z = own[0];
        if (a.filters != z.filters || a.inp_volume != z.inp_volume || a.inp_step != z.inp_step || a.out_stride != z.out_stride)
            return DMCF_EINVAL;
        for (int k = 0; k < 5; ++k)
            if (a.filter_dims[k] != z.filter_dims[k]) return DMCF_EINVAL;
        for (int k = 0; k < 3; ++k)
            if (a.inp_min[k] != z.inp_min[k] || a.inp_dims[k] != z.inp_dims[k]) return DMCF_EINVAL;
    }
    const int step = own[0].inp_step, stride = own[0].out_stride;
    if (!((step == 1 && (stride == 1 || stride == 2)) || (step == 2 && stride == 1))) return DMCF_EUNSUPPORTED;
    return DMCF_OK;
}

static int lat_backward(const dmcf_lattice_conv_args* parts_, int n_parts, const float* grad_out, float* grad_volume, float* grad_filters,
                        void* workspace, size_t workspace_bytes, hipStream_t stream) {
    dmcf_lattice_conv_args parts[kLatMaxParts];
    int rc = lat_bwd_parts(parts_, n_parts, parts);
    if (rc != DMCF_OK) return rc;
    if (!grad_volume && !grad_filters) return DMCF_EINVAL;
    const dmcf_lattice_conv_args& a0 = parts[0];
    const int cin = a0.filter_dims[3], cout = a0.filter_dims[4];
    const size_t vol_floats = (size_t)a0.inp_dims[0] * a0.inp_dims[1] * a0.inp_dims[2] * cin;
    const int64_t w_floats = (int64_t)a0.filter_dims[0] * a0.filter_dims[1] * a0.filter_dims[2] * cin * cout;
    if (a0.n_out == 0) {  // no row, no gradient
        if (grad_volume && hipMemsetAsync(grad_volume, 0, vol_floats * 4, stream) != hipSuccess) return check_launch();
        if (grad_filters && hipMemsetAsync(grad_filters, 0, (size_t)w_floats * 4, stream) != hipSuccess) return check_launch();
        return DMCF_OK;
    }
    if (!grad_out) return DMCF_EINVAL;
    const LatBwdLayout B = lat_bwd_layout(parts, n_parts);
    LatBatch b;
    rc = lat_rows(parts, n_parts, workspace, workspace_bytes, B.total, stream, b, B.F);
    if (rc != DMCF_OK) return rc;
    char* ws = (char*)workspace;
    LatBwd q = {};
    q.gout = grad_out;
    q.n_out = a0.n_out;
    q.cin = cin; q.cout = cout; q.C = b.part[0].KS * 4; q.NT = b.part[0].NT; q.N16 = 16 * q.NT;
    q.Smax = B.Smax;
    q.partial = (float*)(ws + B.off_partial);
    q.red = (float*)(ws + B.off_red);
    q.tcell = (int32_t*)(ws + B.off_tcell);
    q.tw = (float*)(ws + B.off_tw);
    q.ta = (float*)(ws + B.off_ta);
    q.dw_stride = B.dw_stride;
    q.gp = (float*)(ws + B.off_gp);
    q.coutp = B.coutp;
    q.cls = (int32_t*)(ws + B.off_cls);
    q.cls_stride = B.cls_stride;
    q.wt = (float*)(ws + B.off_wt);
    q.wt_stride = B.wt_stride;
    q.step = a0.inp_step;
    q.nclass = q.step * q.step * q.step;
    q.gvol = grad_volume;
    if (grad_filters) {
        if (B.Smax > 0) {
            LatTapArgs t;
            for (int i = 0; i < n_parts; ++i) {
                t.cp[i] = lat_cconv_params(parts + i);
                for (int k = 0; k < 3; ++k) { t.voxel[i][k] = parts[i].voxel[k]; t.shift[i][k] = parts[i].rel_shift[k]; }
            }
            const int SG = (B.Smax + 15) / 16;
            // enough workgroups to fill the chip when the slabs alone do not, each wave still with several groups of 16 offsets
            const int64_t want = (1024 + B.max_slabs - 1) / B.max_slabs;
            const unsigned ny = (unsigned)std::max<int64_t>(1, std::min<int64_t>((SG + 3) / 4, want));
            const dim3 grid((unsigned)B.max_slabs, ny), block(256);
            const int KS = b.part[0].KS, NT = b.part[0].NT;
            if (KS == 1 && NT == 1) hipLaunchKernelGGL((lat_bwd_filter<1, 1>), grid, block, 0, stream, b, q);
            else if (KS == 1) hipLaunchKernelGGL((lat_bwd_filter<2, 1>), grid, block, 0, stream, b, q);
            else if (NT == 1) hipLaunchKernelGGL((lat_bwd_filter<1, 2>), grid, block, 0, stream, b, q);
            else hipLaunchKernelGGL((lat_bwd_filter<2, 2>), grid, block, 0, stream, b, q);
            hipLaunchKernelGGL(lat_bwd_reduce, dim3((unsigned)((B.dw_stride + 255) / 256), (unsigned)n_parts), block, 0, stream, b, q);
            hipLaunchKernelGGL(lat_bwd_taps, dim3((unsigned)((B.Smax + 255) / 256), (unsigned)n_parts), block, 0, stream, b, q, t);
        }
        hipLaunchKernelGGL(lat_bwd_fold, dim3((unsigned)((w_floats + 255) / 256)), dim3(256), 0, stream, b, q, grad_filters, w_floats);
    }
    if (grad_volume) {
        for (int k = 0; k < 3; ++k) {
            q.umin[k] = (int)lat_floor_div(a0.inp_min[k], q.step);
            q.udim[k] = (int)lat_floor_div((int64_t)a0.inp_min[k] + a0.inp_dims[k] - 1, q.step) - q.umin[k] + 1;
        }
        q.tiles_x2 = (q.udim[0] + 31) / 32;
        q.units = (int64_t)q.nclass * q.udim[2] * q.udim[1] * q.tiles_x2;
        if ((q.units + 3) / 4 > 0x7fffffff) return DMCF_EUNSUPPORTED;
        hipLaunchKernelGGL(lat_bwd_pad, dim3((unsigned)(((a0.n_out + 1) * q.coutp + 255) / 256)), dim3(256), 0, stream, q);
        hipLaunchKernelGGL(lat_bwd_classes, dim3((unsigned)n_parts), dim3(64), 0, stream, b, q);
        const unsigned gw = (unsigned)std::min<int64_t>(1024, (B.wt_stride + 255) / 256);
        hipLaunchKernelGGL(lat_bwd_wt, dim3(gw, (unsigned)n_parts), dim3(256), 0, stream, b, q);
        const dim3 grid((unsigned)((q.units + 3) / 4)), block(256);
        switch (q.coutp / 4) {
            case 1: hipLaunchKernelGGL((lat_bwd_input<1>), grid, block, 0, stream, b, q); break;
            case 2: hipLaunchKernelGGL((lat_bwd_input<2>), grid, block, 0, stream, b, q); break;
            case 4: hipLaunchKernelGGL((lat_bwd_input<4>), grid, block, 0, stream, b, q); break;
            case 6: hipLaunchKernelGGL((lat_bwd_input<6>), grid, block, 0, stream, b, q); break;
            default: hipLaunchKernelGGL((lat_bwd_input<8>), grid, block, 0, stream, b, q); break;
        }
    }
    return check_launch();
}
