// Body of cconv_bwd_norm / cconv_bwd_norm_ext (cconv_bwd.hip).  In scope at the include: EXT (compile-time), p (CconvParams),
// out_ext ([n_out], NULL unless EXT), psi.
    const int lane = threadIdx.x & 63, h = lane >> 5, pl = lane & 31;
    const int64_t i = (int64_t)blockIdx.x * 2 + h;
    float nsum = 0.0f;
    if (i < p.n_out) {
        int64_t rb, re;
        bwd_row(p, i, rb, re);
        float inv_extent, inv_r2;
        if (!bwd_row_extent<EXT>(p, out_ext, i, inv_extent, inv_r2)) re = rb;
        const float ox = p.out_pos[3 * i], oy = p.out_pos[3 * i + 1], oz = p.out_pos[3 * i + 2];
        for (int64_t pp = rb + pl; pp < re; pp += 32) {
            const int j = p.idx[pp];
            if (bwd_valid_j(p, j)) nsum += bwd_norm_term(p, i, j, pp, ox, oy, oz, inv_r2);
        }
    }
#pragma unroll
    for (int d = 16; d >= 1; d >>= 1) nsum += __shfl_xor(nsum, d, 64);
    if (pl == 0 && i < p.n_out) psi[i] = nsum;
