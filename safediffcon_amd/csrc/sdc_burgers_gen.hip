// Data generator of the 1D Burgers' task: 1D/data/generate_burgers.py (make_data_varying_f / make_data :302-418,
// burgers_numeric_solve / burgers_numeric_solve_free :113-299).
//
// burgers_wave_kernel is the Euler rollout of csrc/sdc_solver.hip reshaped for generation (10^5 trajectories of s = 128): one wave
// per trajectory, lane l holds the K = ceil(s / 64) cells [l K, l K + K) in registers for the whole rollout, the two values a lane
// needs from its neighbours per step come by DPP wave shifts (one VALU move each, zero in the lane without a source: the Dirichlet
// ghosts of lanes 0 and 63), the force row is read once per interval.  No LDS, no barrier.  The arithmetic is that kernel's
// expressions verbatim, contraction off, fp32 denormals kept (hipcc's default mode), so the bits are the fp32 CPU run's.
// burgers_synth_* evaluate the sums of Gaussians the reference builds on the host, in float64 in its operation order.
#include "sdc_common.h"

namespace {

// value of lane - 1 (lane 0: +0.0f) / lane + 1 (lane 63: +0.0f).  `old` = 0 with bound_ctrl off: a lane without a source keeps old.
__device__ __forceinline__ float from_lane_below(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x138 /* wave_shr:1 */, 0xf, 0xf, false));
}
__device__ __forceinline__ float from_lane_above(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x130 /* wave_shl:1 */, 0xf, 0xf, false));
}

template <int K>
__global__ void __launch_bounds__(1024) burgers_wave_kernel(const float* __restrict__ u0, const float* __restrict__ f,
                                                            float* __restrict__ traj, int N, int Nf, int s, int Nt, int rec,
                                                            int64_t f_sn, int64_t f_st, int pair_mode, float dt, float ct, float d0,
                                                            float d1, float d2) {
    // see burgers_rollout_kernel: only this pragma keeps every product and sum rounded on its own
#pragma clang fp contract(off)
    const int n = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (n >= N) return;                                  // whole waves only: every lane of a running wave stays active for the DPP moves
    const int lane = threadIdx.x & 63;
    const int ui = pair_mode ? n / Nf : n;
    const int fi = pair_mode ? n % Nf : n;
    const int c0 = lane * K;
    const float* fn = f + (int64_t)fi * f_sn + c0;
    float* tn = traj + (int64_t)n * (Nt + 1) * s + c0;
    bool live[K];
    int keep[K];                                         // all ones for a cell < s, 0 for a ghost: ANDed into the step's result, no branch
    float u[K], fv[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        live[k] = c0 + k < s;
        keep[k] = live[k] ? -1 : 0;
        u[k] = live[k] ? u0[(int64_t)ui * s + c0 + k] : 0.f;
        if (live[k]) tn[k] = u[k];
    }
    const float nct = -ct;
    for (int t = 0; t < Nt; ++t) {
#pragma unroll
        for (int k = 0; k < K; ++k) fv[k] = live[k] ? fn[(int64_t)t * f_st + k] : 0.f;
        for (int r = 0; r < rec; ++r) {
            const float lo = from_lane_below(u[K - 1]), hi = from_lane_above(u[0]);
            float un[K];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const float um = k ? u[k - 1] : lo, uc = u[k], up = k + 1 < K ? u[k + 1] : hi;
                // einsum('nsi,si->ns'): products summed in index order
                const float tr = (um * um) * nct + (up * up) * ct;
                const float df = (um * d0 + uc * d1) + up * d2;
                const float rhs = (-0.5f * tr + df) + fv[k];
                un[k] = __int_as_float(__float_as_int(uc + dt * rhs) & keep[k]);   // a ghost stays +0.0f whatever its neighbour holds
            }
#pragma unroll
            for (int k = 0; k < K; ++k) u[k] = un[k];
        }
#pragma unroll
        for (int k = 0; k < K; ++k)
            if (live[k]) tn[(int64_t)(t + 1) * s + k] = u[k];
    }
}

// e(d, sig) of the reference: np.exp(-0.5 * d**2 / sig**2)
__device__ __forceinline__ double gauss(double d, double sig) {
#pragma clang fp contract(off)
    return exp((-0.5 * (d * d)) / (sig * sig));
}

__global__ void burgers_synth_u0_kernel(const double* __restrict__ upar, const float* __restrict__ x, float* __restrict__ u0,
                                        int64_t total, int s) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const double* p = upar + (i / s) * 6;
    const double xv = (double)x[i % s];
    const double g1 = p[1] * gauss(xv - p[0], p[2]);
    const double g2 = p[4] * gauss(xv - p[3], p[5]);
    u0[i] = (float)(g1 + g2);
}

__global__ void burgers_synth_f_kernel(const double* __restrict__ fpar, const float* __restrict__ x, const float* __restrict__ ts,
                                       const float* __restrict__ mask, double comp, float alpha, float* __restrict__ f,
                                       int64_t total, int s, int Nt) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % s);
    const int t = (int)((i / s) % Nt);
    const double* p = fpar + (i / ((int64_t)s * Nt)) * 40;
    const double xv = (double)x[c];
    double acc = 0.0;
    for (int k = 0; k < 8; ++k, p += 5) {
        double es = gauss(xv - p[1], p[2]);
        double term;
        if (ts) {
            if (mask) es = es * (double)mask[c];
            term = (p[0] * es) * (comp * gauss((double)ts[t] - p[3], p[4]));
        } else {
            term = p[0] * es;
        }
        acc = k ? acc + term : term;
    }
    float v = (float)acc;
    if (alpha != 1.f) {
        v = v * alpha;
        v = v < -10.f ? -10.f : (v > 10.f ? 10.f : v);      // clamp(-10, 10): a NaN stays a NaN
    }
    f[i] = v;
}

}  // namespace

extern "C" int sdc_burgers_rollout_wave(const float* u0, const float* f, float* traj, int N, int Nu0, int Nf, int s, int Nt, int rec,
                                        int64_t f_sn, int64_t f_st, int pair_mode, float dt, float coef_transport, float d0, float d1,
                                        float d2, int waves_per_block, void* stream) {
    SDC_REQUIRE(u0 && f && traj, SDC_ENULL, "sdc_burgers_rollout_wave: null pointer");
    SDC_REQUIRE(N > 0 && Nu0 > 0 && Nf > 0 && s > 0 && Nt > 0 && rec > 0, SDC_EINVAL, "sdc_burgers_rollout_wave: bad sizes");
    SDC_REQUIRE(s <= 512, SDC_EINVAL, "sdc_burgers_rollout_wave: s = %d, a wave holds at most 512 cells", s);
    SDC_REQUIRE(f_sn >= 0 && f_st >= 0, SDC_EINVAL, "sdc_burgers_rollout_wave: negative force stride");
    SDC_REQUIRE(pair_mode == 0 || pair_mode == 1, SDC_EINVAL, "sdc_burgers_rollout_wave: pair_mode %d", pair_mode);
    if (pair_mode == 0)
        SDC_REQUIRE(Nu0 == N && Nf == N, SDC_EINVAL, "sdc_burgers_rollout_wave: pair_mode 0 needs Nu0 == Nf == N");
    else
        SDC_REQUIRE((int64_t)Nu0 * Nf == N, SDC_EINVAL, "sdc_burgers_rollout_wave: pair_mode 1 needs N == Nu0 * Nf");
    SDC_REQUIRE(waves_per_block >= 0 && waves_per_block <= 16, SDC_EINVAL, "sdc_burgers_rollout_wave: waves_per_block %d", waves_per_block);
    const int wpb = waves_per_block ? waves_per_block : 4;
    const dim3 grid((N + wpb - 1) / wpb), block(64 * wpb);
    hipStream_t st = sdc::as_stream(stream);
#define SDC_BW_LAUNCH(K)                                                                                                        \
    hipLaunchKernelGGL(burgers_wave_kernel<K>, grid, block, 0, st, u0, f, traj, N, Nf, s, Nt, rec, f_sn, f_st, pair_mode, dt, \
                       coef_transport, d0, d1, d2)
    if (s <= 64) SDC_BW_LAUNCH(1);
    else if (s <= 128) SDC_BW_LAUNCH(2);
    else if (s <= 256) SDC_BW_LAUNCH(4);
    else SDC_BW_LAUNCH(8);
#undef SDC_BW_LAUNCH
    return sdc::check_launch("sdc_burgers_rollout_wave");
}

extern "C" int sdc_burgers_synth(const double* upar, const double* fpar, const float* x, const float* ts, const float* mask,
                                 double comp, float alpha, float* u0, float* f, int Nu0, int Nf, int s, int Nt, void* stream) {
    SDC_REQUIRE(x && (u0 || f), SDC_ENULL, "sdc_burgers_synth: null pointer");
    SDC_REQUIRE((!u0 || upar) && (!f || fpar), SDC_ENULL, "sdc_burgers_synth: null parameter pointer");
    SDC_REQUIRE(s > 0 && (!u0 || Nu0 > 0) && (!f || (Nf > 0 && Nt > 0)), SDC_EINVAL, "sdc_burgers_synth: bad sizes");
    SDC_REQUIRE(!f || ts || Nt == 1, SDC_EINVAL, "sdc_burgers_synth: without a time grid Nt must be 1");
    const int64_t blocks_u = u0 ? ((int64_t)Nu0 * s + 255) / 256 : 0, blocks_f = f ? ((int64_t)Nf * Nt * s + 255) / 256 : 0;
    SDC_REQUIRE(blocks_u <= 0x7fffffff && blocks_f <= 0x7fffffff, SDC_EINVAL, "sdc_burgers_synth: too many elements");
    hipStream_t st = sdc::as_stream(stream);
    if (u0) {
        const int64_t total = (int64_t)Nu0 * s;
        hipLaunchKernelGGL(burgers_synth_u0_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, upar, x, u0, total, s);
    }
    if (f) {
        const int64_t total = (int64_t)Nf * Nt * s;
        hipLaunchKernelGGL(burgers_synth_f_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, fpar, x, ts, mask, comp,
                           alpha, f, total, s, Nt);
    }
    return sdc::check_launch("sdc_burgers_synth");
}
