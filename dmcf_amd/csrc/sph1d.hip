// The 1-D SPH solver behind the column datasets (dmcf_sph1d_rollout): SPH1D.step of the reference's datasets/column_gen.py
// (:159-186) for a batch of independent scenes, advanced n_frames steps in one launch.
//
// A scene is at most 64 points and its work is strictly sequential -- a step is a viscosity pass, an advance, and up to
// max_iter (10 000) pressure iterations of two O(n^2) passes each -- so the layout is ONE 64-LANE WAVEFRONT PER SCENE,
// lane = point, every scene of the batch in flight at once (grid = scenes, block = 64).  The whole state lives in registers;
// the j loop of a pair sum is uniform over the wave and reads point j's values with v_readlane (a wave shuffle with a
// scalar source lane: the value arrives in an SGPR, no LDS, no barrier).  The convergence test max_i err_i < eps is a wave
// vote: no fluid lane may fail err_i < eps (the same predicate, NaN included: a NaN density keeps the loop running to
// max_iter, as np.max does).
//
// Precision, as the reference's numpy evaluates it (include/dmcf_hip.h has the formulas):
//   - the state (x, v, m) is float32; distances x_i - x_j, velocity differences and the spline values W, W' are float32,
//     operation by operation (un-fused: the library is built with -ffp-contract=off, and the roundings are spelled out with
//     __f*_rn); the cubes q^3 are numpy's float32 power: formed in float64 and rounded once;
//   - every product with a mass, a density or a pressure, and every sum over j, is float64;
//   - an update x += ..., v += ... is formed in float64 and rounded to float32 once -- except the advance x += dt v, which
//     numpy evaluates in float32 throughout (a Python float times a float32 array stays float32).
// Sums over j run j = 0 .. n-1 in order (numpy sums pairwise: the order is not part of the contract).  No atomics: equal
// inputs give equal bits, whatever the batch around a scene and however a rollout is cut into launches.
#include "common.h"

namespace dmcf {

constexpr int kSphMaxPoints = 64;  // one lane per point

struct SphConsts {
    double rest, stiffness, visc, gravity, dt, dt2, eps;
    float c43, soft, dt_f32;  // 4 / (3 h), 0.01 h^2 and dt as numpy rounds them when they meet a float32 array
    int bcnt, max_iter;
};

__device__ __forceinline__ float sph_lane(float v, int j) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), j));
}

__device__ __forceinline__ double sph_lane(double v, int j) {
    const uint64_t u = __builtin_bit_cast(uint64_t, v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)u, j);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(u >> 32), j);
    return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}

__device__ __forceinline__ float sph_cube(float t) { return (float)(((double)t * (double)t) * (double)t); }

// compute_val's cubic_spline: the argument is the raw distance (not distance / h), q >= 0
__device__ __forceinline__ float sph_w(float q, float c43) {
    float w = 0.0f;
    if (q <= 1.0f) {
        if (q <= 0.5f) {
            w = __fadd_rn(__fmul_rn(6.0f, __fsub_rn(sph_cube(q), __fmul_rn(q, q))), 1.0f);
        } else {
            w = __fmul_rn(2.0f, sph_cube(__fsub_rn(1.0f, q)));
        }
    }
    return __fmul_rn(c43, w);
}

// compute_grad's cubic_spline_grad: signed argument, two branches
__device__ __forceinline__ float sph_dw(float q, float c43) {
    const float a = fabsf(q);
    const float sg = q > 0.0f ? 1.0f : (q < 0.0f ? -1.0f : 0.0f);
    float g = 0.0f;
    if (a <= 1.0f) {
        if (a <= 0.5f) {
            g = __fsub_rn(__fmul_rn(__fmul_rn(18.0f, sg), __fmul_rn(q, q)), __fmul_rn(12.0f, q));
        } else {
            const float t = __fsub_rn(1.0f, a);
            g = __fmul_rn(__fmul_rn(-6.0f, sg), __fmul_rn(t, t));
        }
    }
    return __fmul_rn(c43, g);
}

// compute_val(): dens_i = sum_j m_j W(|x_i - x_j|)
__device__ __forceinline__ double sph_density(float x, float m, int n, float c43) {
    double s = 0.0;
    for (int j = 0; j < n; ++j) {
        const float q = fabsf(__fsub_rn(x, sph_lane(x, j)));
        s += (double)sph_lane(m, j) * (double)sph_w(q, c43);
    }
    return s;
}

__global__ __launch_bounds__(kSphMaxPoints) void sph1d_rollout(const float* state_in,
                                                               const int32_t* __restrict__ n_tot, int max_points,
                                                               const SphConsts c, int n_frames, int64_t n_scenes,
                                                               float* __restrict__ sequence, float* state_out,
                                                               int32_t* __restrict__ iterations) {
    const int64_t scene = blockIdx.x;
    const int lane = threadIdx.x;
    int n = n_tot[scene];
    n = n < 0 ? 0 : (n > max_points ? max_points : n);  // (the host checks max_points <= 64; n is uniform over the wave)
    const bool live = lane < n, fluid = live && lane >= c.bcnt;
    const bool slot = lane < max_points;
    const float* sp = state_in + (scene * max_points + lane) * 3;
    // every lane stays active to the end (readlane needs its source lane's registers current); idle lanes carry zeros
    float x = live ? sp[0] : 0.0f, v = live ? sp[1] : 0.0f;
    const float m = live ? sp[2] : 0.0f;
    const double md = (double)m;

    for (int t = 0; t < n_frames; ++t) {
        if (slot) {  // recorded BEFORE the step (gen_data :309-312)
            float* q = sequence + (((int64_t)t * n_scenes + scene) * max_points + lane) * 2;
            q[0] = x;
            q[1] = v;
        }
        // compute_visc: visc * 2 sum_j m_j / dens_j (v_i - v_j) d W'(d) / (d^2 + 0.01 h^2), d = x_i - x_j
        {
            const double dens = sph_density(x, m, n, c.c43);
            const double a = md / dens;
            double s = 0.0;
            for (int j = 0; j < n; ++j) {
                const float d = __fsub_rn(x, sph_lane(x, j));
                const float dv = __fsub_rn(v, sph_lane(v, j));
                const float den = __fadd_rn(__fmul_rn(d, d), c.soft);
                s += (((sph_lane(a, j) * (double)dv) * (double)d) * (double)sph_dw(d, c.c43)) / (double)den;
            }
            const double f_visc = c.visc * (2.0 * s);
            if (fluid) {
                v = (float)((double)v + c.dt * (c.gravity + f_visc));
                x = __fadd_rn(x, __fmul_rn(c.dt_f32, v));
            }
        }
        int it = 0;
        for (;;) {
            const double dens = sph_density(x, m, n, c.c43);
            const double r = dens / c.rest, r2 = r * r, r4 = r2 * r2;
            double pres = c.stiffness * (((r4 * r2) * r) - 1.0);
            pres = pres < 0.0 ? 0.0 : pres;
            const double pres_first = sph_lane(pres, c.bcnt);  // boundary points take the first fluid point's pressure
            if (lane < c.bcnt) pres = pres_first;
            double err = dens - c.rest;
            err = err < 0.0 ? 0.0 : err;
            const bool open = fluid && !(err < c.eps);
            // compute_grad: dens_i sum_j m_j (p_i / dens_i^2 + p_j / dens_j^2) W'(x_i - x_j)
            const double a = pres / (dens * dens);
            double s = 0.0;
            for (int j = 0; j < n; ++j) {
                const float d = __fsub_rn(x, sph_lane(x, j));
                s += ((double)sph_lane(m, j) * (a + sph_lane(a, j))) * (double)sph_dw(d, c.c43);
            }
            const double f = -(md / dens) * (dens * s);
            if (fluid) {  // applied BEFORE the convergence test ends the loop (:175-181)
                v = (float)((double)v + (c.dt * f) / md);
                x = (float)((double)x + (c.dt2 * f) / md);
            }
            ++it;
            if (__ballot(open) == 0 || it >= c.max_iter) break;
        }
        if (lane == 0) iterations[(int64_t)t * n_scenes + scene] = it;
    }
    if (slot) {
        float* q = state_out + (scene * max_points + lane) * 3;
        q[0] = x;
        q[1] = v;
        q[2] = m;
    }
}

}  // namespace dmcf

using namespace dmcf;

extern "C" {

int dmcf_sph1d_rollout(const float* state, const int32_t* n_tot, int64_t n_scenes, int32_t max_points,
                       const dmcf_sph1d_params* params, int32_t n_frames, float* sequence, float* state_out,
                       int32_t* iterations, dmcf_stream_t stream) {
    if (!params || params->struct_size < sizeof(dmcf_sph1d_params)) return DMCF_EINVAL;
    if (n_scenes < 0 || n_scenes > 0x7fffffffLL || n_frames < 0) return DMCF_EINVAL;
    if (max_points < 1 || max_points > kSphMaxPoints) return DMCF_EINVAL;  // one lane per point
    if (params->bcnt < 0 || params->bcnt >= max_points || params->max_iter < 1) return DMCF_EINVAL;
    if (!(params->h > 0.0) || !(params->rest_dens > 0.0) || !(params->dt == params->dt)) return DMCF_EINVAL;
    if (n_scenes == 0) return DMCF_OK;
    if (!state || !n_tot || !state_out) return DMCF_EINVAL;
    if (n_frames > 0 && (!sequence || !iterations)) return DMCF_EINVAL;
    SphConsts c;
    c.rest = params->rest_dens;
    c.stiffness = params->stiffness;
    c.visc = params->visc;
    c.gravity = params->gravity;
    c.dt = params->dt;
    c.dt2 = params->dt * params->dt;
    c.eps = params->eps;
    c.c43 = (float)(4.0 / (3.0 * params->h));
    c.soft = (float)(0.01 * (params->h * params->h));
    c.dt_f32 = (float)params->dt;
    c.bcnt = params->bcnt;
    c.max_iter = params->max_iter;
    hipLaunchKernelGGL(sph1d_rollout, dim3((unsigned)n_scenes), dim3(kSphMaxPoints), 0, (hipStream_t)stream, state, n_tot,
                       (int)max_points, c, (int)n_frames, n_scenes, sequence, state_out, iterations);
    return check_launch();
}

}  // extern "C"
