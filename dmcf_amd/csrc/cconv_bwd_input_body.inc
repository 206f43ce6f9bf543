// Body of cconv_bwd_input / cconv_bwd_input_ext (cconv_bwd.hip).  In scope at the include: EXT (compile-time), the kernels' common
// arguments, out_ext ([n_out], NULL unless EXT).
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x;
    const int K = geo.K, cin = geo.cin, cout = geo.cout;
    float* T = smem;                            // [K][cout]
    float* ws = T + (size_t)K * cout;           // [64][kBwdWStride]
    int* bs = (int*)(ws + 64 * kBwdWStride);    // [64]
    int* js = bs + 64;                          // [64] output row of the staged pair
    float* red = (float*)(js + 64);             // [64] contraction partials
    const int64_t j = blockIdx.x;
    for (int e = lane; e < K * cout; e += 64) T[e] = 0.0f;
    const float jx = p.inp_pos[3 * j], jy = p.inp_pos[3 * j + 1], jz = p.inp_pos[3 * j + 2];
    __syncthreads();

    auto splat = [&](int nq) {
        for (int o = lane; o < cout; o += 64) {
            for (int q = 0; q < nq; ++q) {
                const float g = G[(int64_t)js[q] * cout + o];
                float* tb = T + (size_t)bs[q] * cout + o;
#pragma unroll
                for (int t = 0; t < 8; ++t)
                    if (geo.live & (1u << t)) tb[geo.off[t] * cout] += ws[q * kBwdWStride + t] * g;
            }
        }
    };
    // (1) the pairs that reference j: output row i = inv_index[q], forward pair inv_pair[q]
    int64_t qb = inv_rs[j], qe = inv_rs[j + 1];
    if (qb < 0) qb = 0;
    if (qe > inv_n_pairs) qe = inv_n_pairs;
    for (int64_t q0 = qb; q0 < qe; q0 += 64) {
        const int64_t q = q0 + lane;
        bool valid = q < qe;
        int64_t i = 0, pp = 0;
        if (valid) {
            i = inv_index[q];
            pp = inv_pair[q];
            valid = i >= 0 && i < p.n_out && pp >= 0 && pp < p.pair_cap;
        }
        float w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        int base = 0;
        float coef = 0.0f;
        float inv_extent = 0.0f, inv_r2 = 0.0f;  // (EXT only) of the pair's output row: a load of out_ext[i] per pair
        if (EXT && valid) valid = bwd_row_extent<EXT>(p, out_ext, i, inv_extent, inv_r2);
        if (valid) {
            const float a = bwd_pair(p, i, (int)j, pp, p.out_pos[3 * i], p.out_pos[3 * i + 1], p.out_pos[3 * i + 2],
                                     EXT ? inv_extent : p.inv_extent, EXT ? inv_r2 : p.inv_r2, base, w);
            coef = a / bwd_scale(psi, i);
        }
        bwd_stage(ws, bs, js, lane, valid, coef, base, w, (int)i);
        __syncthreads();
        splat((int)min((int64_t)64, qe - q0));
        __syncthreads();
    }
    // (2) ASCC centre term: row j of the forward list, every pair with G[j]
    if (symmetric && j < p.n_out) {
        int64_t rb, re;
        bwd_row(p, j, rb, re);
        float inv_extent = 0.0f, inv_r2 = 0.0f;  // (EXT only) of forward row j
        if (EXT && !bwd_row_extent<EXT>(p, out_ext, j, inv_extent, inv_r2)) re = rb;
        const float sc = bwd_scale(psi, j);
        for (int64_t b0 = rb; b0 < re; b0 += 64) {
            const int64_t pp = b0 + lane;
            bool valid = pp < re;
            int jj = 0;
            if (valid) {
                jj = p.idx[pp];
                valid = bwd_valid_j(p, jj);
            }
            float w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            int base = 0;
            float coef = 0.0f;
            if (valid) coef = bwd_pair(p, j, jj, pp, jx, jy, jz, EXT ? inv_extent : p.inv_extent, EXT ? inv_r2 : p.inv_r2, base, w) / sc;
            bwd_stage(ws, bs, js, lane, valid, coef, base, w, (int)j);
            __syncthreads();
            splat((int)min((int64_t)64, re - b0));
            __syncthreads();
        }
    }
    // dF_j[c] = sum_cell sum_o W[cell, c, o] T[cell, o]; lanes = (cell part, channel), parts summed in order
    float* dst = dF + j * cin;
    if (cin <= 64) {
        const int P = 64 / cin, part = lane / cin, c = lane % cin;
        float acc = 0.0f;
        if (part < P) {
            for (int cell = part; cell < K; cell += P) {
                const float* wr = Wfull + ((size_t)cell * cin + c) * cout;
                const float* tr = T + (size_t)cell * cout;
                for (int o = 0; o < cout; ++o) acc += wr[o] * tr[o];
            }
        }
        red[lane] = acc;
        __syncthreads();
        if (lane < cin) {
            float v = 0.0f;
            for (int q = 0; q < P; ++q) v += red[q * cin + lane];
            dst[lane] = accumulate ? dst[lane] + v : v;
        }
    } else {
        for (int c = lane; c < cin; c += 64) {
            float acc = 0.0f;
            for (int cell = 0; cell < K; ++cell) {
                const float* wr = Wfull + ((size_t)cell * cin + c) * cout;
                const float* tr = T + (size_t)cell * cout;
                for (int o = 0; o < cout; ++o) acc += wr[o] * tr[o];
            }
            dst[c] = accumulate ? dst[c] + acc : acc;
        }
    }
