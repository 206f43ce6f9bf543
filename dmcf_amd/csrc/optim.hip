// The optimizer update of the training loop (dmcf_adam_step): one multi-tensor Adam step over every trainable tensor of a
// model, in the order of operations of TensorFlow's ApplyAdam GPU functor (what tf.keras.optimizers.Adam runs, the
// reference's models/pbf_model.py:511-517):
//     alpha = lr sqrt(1 - beta_2^t) / (1 - beta_1^t)
//     m += (1 - beta_1)(g - m)
//     v += (1 - beta_2)(g^2 - v)
//     var -= alpha m / (eps + sqrt(v))
// With clip_norm > 0 every gradient is first clipped per tensor as tf.clip_by_norm does: g c / max(|g|, c), |g| = 0 when
// the l2 sum is 0 (the reference's grad_clip_norm, pipelines/simulator.py:405-407).
//
// Kernels (the names dmcf_adam_step_kernel_names reports):
//   adam_sumsq   with clipping only: per (tensor, block column) the double sum of g^2 over the block's chunks, one partial
//                per block (grid stride over the chunks, fixed lane order, a fixed tree over the block)
//   adam_update  per (tensor, block column): every block first combines its tensor's partials in one fixed order (so all
//                blocks of a tensor see the same norm), then updates its chunks; 16-byte accesses when all four pointers of
//                the tensor are 16-byte aligned, element-wise for the tail and for unaligned tensors
// Grid: x = block columns (the largest tensor's chunks, at most kAdamMaxCols), y = tensor.  No float atomics anywhere:
// two identical calls give identical bits.
#include <stdio.h>
#include <string.h>

#include "common.h"

namespace dmcf {

constexpr int kAdamThreads = 256;
constexpr int kAdamChunk = kAdamThreads * 4;  // floats per block and pass: one float4 per thread
constexpr int kAdamMaxCols = 256;             // block columns per tensor (partials per tensor when clipping)

typedef float adam_f32x4 __attribute__((ext_vector_type(4)));

struct AdamScalars {
    float lr, beta_1, beta_2, epsilon, beta_1_power, beta_2_power, clip_norm;
    int cols;
};

__device__ __forceinline__ double adam_block_sum(double x, double* red) {
    // fixed butterfly inside each wave, then the waves' sums in wave order
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) red[wv] = x;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < kAdamThreads / 64; ++w) s += red[w];
    return s;
}

__global__ __launch_bounds__(kAdamThreads) void adam_sumsq(const dmcf_adam_tensor* __restrict__ tabs, int cols,
                                                           double* __restrict__ partials) {
    __shared__ double red[kAdamThreads / 64];
    const dmcf_adam_tensor T = tabs[blockIdx.y];
    const int64_t n = T.n;
    double acc = 0.0;
    for (int64_t base = (int64_t)blockIdx.x * kAdamChunk; base < n; base += (int64_t)cols * kAdamChunk) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t i = base + k * kAdamThreads + threadIdx.x;
            if (i < n) {
                const double g = (double)T.grad[i];
                acc += g * g;
            }
        }
    }
    const double s = adam_block_sum(acc, red);
    if (threadIdx.x == 0) partials[(size_t)blockIdx.y * cols + blockIdx.x] = s;
}

__device__ __forceinline__ void adam_elem(float& var, float& m, float& v, float g, float alpha, float omb1, float omb2, float eps) {
    m = __fadd_rn(m, __fmul_rn(omb1, __fsub_rn(g, m)));
    v = __fadd_rn(v, __fmul_rn(omb2, __fsub_rn(__fmul_rn(g, g), v)));
    var = __fsub_rn(var, __fdiv_rn(__fmul_rn(alpha, m), __fadd_rn(eps, __fsqrt_rn(v))));
}

__global__ __launch_bounds__(kAdamThreads) void adam_update(const dmcf_adam_tensor* __restrict__ tabs, const AdamScalars s,
                                                            const double* __restrict__ partials) {
    __shared__ double red[kAdamThreads / 64];
    const dmcf_adam_tensor T = tabs[blockIdx.y];
    const int64_t n = T.n;
    if ((int64_t)blockIdx.x * kAdamChunk >= n) return;  // (uniform over the block: no barrier below is skipped by part of it)
    // clip factor: g -> (g c) / max(norm, c); the tensor's partials combined in one fixed order by every block
    const bool clip = s.clip_norm > 0.0f;
    float denom = 1.0f;
    if (clip) {
        double part = 0.0;
        for (int i = threadIdx.x; i < s.cols; i += kAdamThreads) part += partials[(size_t)blockIdx.y * s.cols + i];
        const float l2sum = (float)adam_block_sum(part, red);
        const float norm = l2sum > 0.0f ? __fsqrt_rn(l2sum) : l2sum;
        denom = fmaxf(norm, s.clip_norm);
    }
    const float alpha = __fdiv_rn(__fmul_rn(s.lr, __fsqrt_rn(__fsub_rn(1.0f, s.beta_2_power))), __fsub_rn(1.0f, s.beta_1_power));
    const float omb1 = __fsub_rn(1.0f, s.beta_1), omb2 = __fsub_rn(1.0f, s.beta_2), eps = s.epsilon, c = s.clip_norm;
    auto grad = [&](float g) { return clip ? __fdiv_rn(__fmul_rn(g, c), denom) : g; };
    const bool aligned = ((reinterpret_cast<uintptr_t>(T.param) | reinterpret_cast<uintptr_t>(T.grad) |
                           reinterpret_cast<uintptr_t>(T.m) | reinterpret_cast<uintptr_t>(T.v)) & 15) == 0;
    if (aligned) {
        const int64_t n4 = n >> 2;
        adam_f32x4* P = reinterpret_cast<adam_f32x4*>(T.param);
        adam_f32x4* M = reinterpret_cast<adam_f32x4*>(T.m);
        adam_f32x4* V = reinterpret_cast<adam_f32x4*>(T.v);
        const adam_f32x4* G = reinterpret_cast<const adam_f32x4*>(T.grad);
        for (int64_t i = (int64_t)blockIdx.x * kAdamThreads + threadIdx.x; i < n4; i += (int64_t)s.cols * kAdamThreads) {
            const adam_f32x4 p = P[i], m = M[i], v = V[i], g = G[i];
            float pk[4], mk[4], vk[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                pk[k] = p[k];
                mk[k] = m[k];
                vk[k] = v[k];
                adam_elem(pk[k], mk[k], vk[k], grad(g[k]), alpha, omb1, omb2, eps);
            }
            P[i] = (adam_f32x4){pk[0], pk[1], pk[2], pk[3]};
            M[i] = (adam_f32x4){mk[0], mk[1], mk[2], mk[3]};
            V[i] = (adam_f32x4){vk[0], vk[1], vk[2], vk[3]};
        }
        // the odd tail (n % 4 elements): block column 0
        const int64_t i = (n4 << 2) + threadIdx.x;
        if (blockIdx.x == 0 && i < n) adam_elem(T.param[i], T.m[i], T.v[i], grad(T.grad[i]), alpha, omb1, omb2, eps);
    } else {  // (the chunks of adam_sumsq)
        for (int64_t base = (int64_t)blockIdx.x * kAdamChunk; base < n; base += (int64_t)s.cols * kAdamChunk) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int64_t i = base + k * kAdamThreads + threadIdx.x;
                if (i < n) adam_elem(T.param[i], T.m[i], T.v[i], grad(T.grad[i]), alpha, omb1, omb2, eps);
            }
        }
    }
}

struct AdamPlan {
    int cols;
    bool clip;
    size_t ws_bytes;
};

static int adam_plan(const dmcf_adam_args* a, AdamPlan& pl) {
    if (!a || a->struct_size < sizeof(dmcf_adam_args)) return DMCF_EINVAL;
    if (a->n_tensors < 0 || a->n_tensors > 65535) return DMCF_EINVAL;
    if (a->n_tensors > 0 && (!a->tensors || !a->device_tensors)) return DMCF_EINVAL;
    int64_t maxn = 0;
    for (int t = 0; t < a->n_tensors; ++t) {
        const dmcf_adam_tensor& T = a->tensors[t];
        if (T.n < 0) return DMCF_EINVAL;
        if (T.n > 0 && (!T.param || !T.grad || !T.m || !T.v)) return DMCF_EINVAL;
        maxn = T.n > maxn ? T.n : maxn;
    }
    if (!(a->clip_norm == a->clip_norm)) return DMCF_EINVAL;  // NaN
    const int64_t chunks = (maxn + kAdamChunk - 1) / kAdamChunk;
    pl.cols = (int)(chunks < kAdamMaxCols ? chunks : kAdamMaxCols);
    pl.clip = a->clip_norm > 0.0f && maxn > 0;
    pl.ws_bytes = pl.clip ? sizeof(double) * (size_t)a->n_tensors * pl.cols : 0;
    return DMCF_OK;
}

}  // namespace dmcf

using namespace dmcf;

extern "C" {

size_t dmcf_adam_step_workspace_bytes(const dmcf_adam_args* a) {
    AdamPlan pl;
    if (adam_plan(a, pl) != DMCF_OK) return 0;
    return pl.ws_bytes;
}

int dmcf_adam_step(const dmcf_adam_args* a, void* workspace, size_t workspace_bytes, dmcf_stream_t stream) {
    AdamPlan pl;
    int rc = adam_plan(a, pl);
    if (rc != DMCF_OK) return rc;
    if (workspace_bytes < pl.ws_bytes || (pl.ws_bytes && !workspace)) return DMCF_EWORKSPACE;
    if (pl.cols == 0) return DMCF_OK;  // no tensor holds an element
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)pl.cols, (unsigned)a->n_tensors);
    double* partials = (double*)workspace;
    if (pl.clip) {
        hipLaunchKernelGGL(adam_sumsq, grid, dim3(kAdamThreads), 0, st, a->device_tensors, pl.cols, partials);
        rc = check_launch();
        if (rc != DMCF_OK) return rc;
    }
    AdamScalars s;
    s.lr = a->lr;
    s.beta_1 = a->beta_1;
    s.beta_2 = a->beta_2;
    s.epsilon = a->epsilon;
    s.beta_1_power = a->beta_1_power;
    s.beta_2_power = a->beta_2_power;
    s.clip_norm = pl.clip ? a->clip_norm : -1.0f;
    s.cols = pl.cols;
    hipLaunchKernelGGL(adam_update, grid, dim3(kAdamThreads), 0, st, a->device_tensors, s, (const double*)partials);
    return check_launch();
}

int dmcf_adam_step_kernel_names(const dmcf_adam_args* a, char* names, size_t name_bytes) {
    if (!names || name_bytes < 2) return DMCF_EINVAL;
    AdamPlan pl;
    const int rc = adam_plan(a, pl);
    if (rc != DMCF_OK) return rc;
    const char* s = pl.cols == 0 ? "" : (pl.clip ? "adam_sumsq;adam_update" : "adam_update");
    if (strlen(s) + 1 > name_bytes) return DMCF_EINVAL;
    memcpy(names, s, strlen(s) + 1);
    return DMCF_OK;
}

}  // extern "C"
