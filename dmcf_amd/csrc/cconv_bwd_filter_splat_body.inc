// Body of cconv_bwd_filter_splat / cconv_bwd_filter_splat_ext (cconv_bwd.hip).  In scope at the include: EXT (compile-time), the
// kernels' common arguments, out_ext ([n_out], NULL unless EXT).
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x;
    const int K = geo.K, cin = geo.cin;
    float* B = smem;                            // [K][cin]
    float* ws = B + (size_t)K * cin;
    int* bs = (int*)(ws + 64 * kBwdWStride);
    int* js = bs + 64;
    const int64_t i = row0 + blockIdx.x;
    for (int e = lane; e < K * cin; e += 64) B[e] = 0.0f;
    __syncthreads();
    int64_t rb, re;
    bwd_row(p, i, rb, re);
    float inv_extent, inv_r2;
    if (!bwd_row_extent<EXT>(p, out_ext, i, inv_extent, inv_r2)) re = rb;
    const float ox = p.out_pos[3 * i], oy = p.out_pos[3 * i + 1], oz = p.out_pos[3 * i + 2];
    const float sc = bwd_scale(psi, i);
    for (int64_t b0 = rb; b0 < re; b0 += 64) {
        const int64_t pp = b0 + lane;
        bool valid = pp < re;
        int j = 0;
        if (valid) {
            j = p.idx[pp];
            valid = bwd_valid_j(p, j);
        }
        float w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        int base = 0;
        float coef = 0.0f;
        if (valid) coef = bwd_pair(p, i, j, pp, ox, oy, oz, inv_extent, inv_r2, base, w) / sc;
        bwd_stage(ws, bs, js, lane, valid, coef, base, w, j);
        __syncthreads();
        const int nq = (int)min((int64_t)64, re - b0);
        for (int c = lane; c < cin; c += 64) {
            const float fi = symmetric ? p.inp_feat[i * cin + c] : 0.0f;
            for (int q = 0; q < nq; ++q) {
                float f = p.inp_feat[(int64_t)js[q] * cin + c];
                if (symmetric) f += fi;
                float* bb = B + (size_t)bs[q] * cin + c;
#pragma unroll
                for (int t = 0; t < 8; ++t)
                    if (geo.live & (1u << t)) bb[geo.off[t] * cin] += ws[q * kBwdWStride + t] * f;
            }
        }
        __syncthreads();
    }
    float* dst = Bc + (size_t)blockIdx.x * K * cin;
    for (int e = lane; e < K * cin; e += 64) dst[e] = B[e];
