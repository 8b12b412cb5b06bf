// The optimizer tail of a fine-tuning iteration -- clip_grad_norm_ + SGD / Adam / AdamW + EMA -- over every parameter of a net:
// three launches (per-chunk gradient square sums, one workgroup that reduces them and advances the step, one streaming update
// pass).  Arithmetic and table layout: include/sdc.h.  Pure HBM streaming: Adam with an EMA twin reads p, g, m, v, ema and
// writes p, m, v, ema once, plus one read of g for the norm; no LDS beyond the cross-wave sums, no atomics.
#include "sdc_common.h"
#include <cstdint>

namespace {

constexpr int NT = 256;
constexpr int CHUNK = 4096;          // elements per chunk: four 16-byte accesses per thread and array
constexpr int GRID_CAP = 2048;       // 256 CUs x 8 workgroups; the other chunks are grid-strided

// item of chunk c: the last one with chunk0 <= c (items[0].chunk0 == 0)
__device__ __forceinline__ int find_item(const SdcOptItem* __restrict__ items, const int n, const int64_t c) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (items[mid].chunk0 <= c) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// sum over the workgroup in a fixed order (wave butterflies, then the four wave sums in index order); valid in thread 0
__device__ __forceinline__ double block_sum(double s, double* red) {
    s = sdc::wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < NT / 64; ++w) t += red[w];
    __syncthreads();
    return t;
}

// partial[c] = sum of g^2 over chunk c, in fp64 (a product of two floats is exact there and cannot overflow)
__global__ __launch_bounds__(NT) void optim_norm_kernel(const SdcOptItem* __restrict__ items, const int n, const int total,
                                                        double* __restrict__ partial) {
    __shared__ double red[NT / 64];
    for (int c = blockIdx.x; c < total; c += gridDim.x) {
        const SdcOptItem& it = items[find_item(items, n, c)];
        const int64_t off = (c - it.chunk0) * (int64_t)CHUNK;
        const int cnt = (int)(it.n - off < CHUNK ? it.n - off : CHUNK);
        const float* g = it.g + off;
        double s = 0.0;
        int done = 0;
        if (aligned16(it.g)) {
            const int n4 = cnt >> 2;
            for (int e = threadIdx.x; e < n4; e += NT) {
                const float4 q = reinterpret_cast<const float4*>(g)[e];
                s += (double)q.x * q.x + (double)q.y * q.y + (double)q.z * q.z + (double)q.w * q.w;
            }
            done = n4 << 2;
        }
        for (int e = done + threadIdx.x; e < cnt; e += NT) s += (double)g[e] * g[e];
        s = block_sum(s, red);
        if (threadIdx.x == 0) partial[c] = s;
    }
}

// One workgroup: the norm from the partial sums (fixed order), the clip coefficient, the finite test, the step counter and the
// EMA decision of this step.  The update pass only reads what this launch wrote.
__global__ __launch_bounds__(NT) void optim_prepare_kernel(const double* __restrict__ partial, const int total, const double* __restrict__ hp,
                                                           SdcOptState* __restrict__ st, const int flags, const int have_norm) {
    __shared__ double red[NT / 64];
    double s = 0.0;
    if (have_norm)
        for (int c = threadIdx.x; c < total; c += NT) s += partial[c];
    s = block_sum(s, red);
    if (threadIdx.x != 0) return;
    double coef = 1.0;
    bool finite = true;
    if (have_norm) {
        const double norm = sqrt(s);
        finite = s == s && s - s == 0.0;              // neither NaN nor Inf
        st->grad_norm = (float)norm;
        if (flags & SDC_OPT_CLIP) {
            const double c = hp[SDC_OPT_HP_MAX_GRAD_NORM] / (norm + 1e-6);
            coef = c > 1.0 ? 1.0 : c;                 // a NaN stays a NaN, as torch's clamp(max=1) keeps it
        }
    }
    st->clip_coef = (float)coef;
    if ((flags & SDC_OPT_SKIP_NONFINITE) && !finite) {
        st->applied = 0;
        st->ema_mode = 0;
        return;
    }
    const int64_t t = st->step + 1;
    st->step = t;
    st->applied = 1;
    const int64_t every = (int64_t)hp[SDC_OPT_HP_EMA_UPDATE_EVERY], after = (int64_t)hp[SDC_OPT_HP_EMA_UPDATE_AFTER_STEP];
    st->ema_mode = (every >= 1 && t % every == 0) ? (t <= after ? 1 : 2) : 0;
}

// the scalars of one step, the same in every thread (read from device memory: a captured replay follows them)
struct StepScalars {
    float coef, lr, wd, decay, mu, w1, b2, w2, step_size, bc2_sqrt, eps, ema_w;
    int ema_mode;
};

// Element arithmetic: every line is one fp32 operation -- a rounded product or sum, or one fused multiply-add where the formula is
// a * b + c -- and nothing else is contracted, so the result is fixed by this text (include/sdc.h).
template <int KIND>
__device__ __forceinline__ void update_one(const StepScalars& k, float& p, const float g, float& m, float& v) {
#pragma clang fp contract(off)
    float gc = g * k.coef;                            // rounded to fp32 as clip_grad_norm_ would have stored it
    if (KIND == SDC_OPT_ADAMW) {
        p = p * k.decay;
    } else if (k.wd != 0.0f) {
        gc = fmaf(k.wd, p, gc);
    }
    if (KIND == SDC_OPT_SGD) {
        m = fmaf(k.mu, m, gc);
        p = fmaf(-k.lr, m, p);
    } else {
        m = fmaf(k.w1, gc - m, m);
        v = fmaf(k.w2, gc * gc, v * k.b2);
        const float denom = sqrtf(v) / k.bc2_sqrt + k.eps;
        p = fmaf(-k.step_size, m / denom, p);
    }
}

__device__ __forceinline__ float ema_one(const StepScalars& k, const float ema, const float p) {
#pragma clang fp contract(off)
    return k.ema_mode == 1 ? p : fmaf(k.ema_w, p - ema, ema);
}

template <int KIND>
__global__ __launch_bounds__(NT) void optim_update_kernel(const SdcOptItem* __restrict__ items, const int n, const int total,
                                                          const double* __restrict__ hp, const SdcOptState* __restrict__ st) {
    if (!st->applied) return;
    StepScalars k;
    {
        const double lr = hp[SDC_OPT_HP_LR], b1 = hp[SDC_OPT_HP_BETA1], b2 = hp[SDC_OPT_HP_BETA2], wd = hp[SDC_OPT_HP_WEIGHT_DECAY];
        const double t = (double)st->step;
        k.coef = st->clip_coef;
        k.lr = (float)lr;
        k.wd = (float)wd;
        k.decay = (float)(1.0 - lr * wd);
        k.mu = (float)b1;
        k.w1 = (float)(1.0 - b1);
        k.b2 = (float)b2;
        k.w2 = (float)(1.0 - b2);
        k.eps = (float)hp[SDC_OPT_HP_EPS];
        k.ema_w = (float)(1.0 - hp[SDC_OPT_HP_EMA_BETA]);
        k.ema_mode = st->ema_mode;
        k.step_size = 0.0f;
        k.bc2_sqrt = 1.0f;
        if (KIND != SDC_OPT_SGD) {                    // 1 - beta^t in fp64: 1 - 0.999f loses four digits at small t
            k.step_size = (float)(lr / (1.0 - pow(b1, t)));
            k.bc2_sqrt = (float)sqrt(1.0 - pow(b2, t));
        }
    }
    for (int c = blockIdx.x; c < total; c += gridDim.x) {
        const SdcOptItem& it = items[find_item(items, n, c)];
        const int64_t off = (c - it.chunk0) * (int64_t)CHUNK;
        const int cnt = (int)(it.n - off < CHUNK ? it.n - off : CHUNK);
        float* p = it.p + off;
        const float* g = it.g + off;
        float* m = it.m + off;
        float* v = KIND == SDC_OPT_SGD ? nullptr : it.v + off;
        float* ema = (it.ema && k.ema_mode) ? it.ema + off : nullptr;
        int done = 0;
        if (aligned16(it.p) && aligned16(it.g) && aligned16(it.m) && (KIND == SDC_OPT_SGD || aligned16(it.v)) && aligned16(it.ema)) {
            const int n4 = cnt >> 2;
#pragma unroll 2
            for (int e = threadIdx.x; e < n4; e += NT) {
                float4 p4 = reinterpret_cast<float4*>(p)[e];
                const float4 g4 = reinterpret_cast<const float4*>(g)[e];
                float4 m4 = reinterpret_cast<float4*>(m)[e];
                float4 v4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (KIND != SDC_OPT_SGD) v4 = reinterpret_cast<float4*>(v)[e];
                update_one<KIND>(k, p4.x, g4.x, m4.x, v4.x);
                update_one<KIND>(k, p4.y, g4.y, m4.y, v4.y);
                update_one<KIND>(k, p4.z, g4.z, m4.z, v4.z);
                update_one<KIND>(k, p4.w, g4.w, m4.w, v4.w);
                reinterpret_cast<float4*>(p)[e] = p4;
                reinterpret_cast<float4*>(m)[e] = m4;
                if (KIND != SDC_OPT_SGD) reinterpret_cast<float4*>(v)[e] = v4;
                if (ema) {
                    float4 e4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    if (k.ema_mode == 2) e4 = reinterpret_cast<float4*>(ema)[e];
                    e4.x = ema_one(k, e4.x, p4.x);
                    e4.y = ema_one(k, e4.y, p4.y);
                    e4.z = ema_one(k, e4.z, p4.z);
                    e4.w = ema_one(k, e4.w, p4.w);
                    reinterpret_cast<float4*>(ema)[e] = e4;
                }
            }
            done = n4 << 2;
        }
        for (int e = done + threadIdx.x; e < cnt; e += NT) {      // items that are only 4-byte aligned, and the n % 4 tail
            float pe = p[e], me = m[e], ve = 0.0f;
            if (KIND != SDC_OPT_SGD) ve = v[e];
            update_one<KIND>(k, pe, g[e], me, ve);
            p[e] = pe;
            m[e] = me;
            if (KIND != SDC_OPT_SGD) v[e] = ve;
            if (ema) ema[e] = ema_one(k, k.ema_mode == 2 ? ema[e] : 0.0f, pe);
        }
    }
}

bool kind_ok(int kind) { return kind == SDC_OPT_SGD || kind == SDC_OPT_ADAM || kind == SDC_OPT_ADAMW; }
bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

}  // namespace

extern "C" int sdc_optim_plan(SdcOptItem* items, int n, int kind, int* chunk, int* total_chunks, int* grid) {
    SDC_REQUIRE(items && chunk && total_chunks && grid, SDC_ENULL, "sdc_optim_plan: null pointer");
    SDC_REQUIRE(n > 0, SDC_EINVAL, "sdc_optim_plan: no items");
    SDC_REQUIRE(kind_ok(kind), SDC_EINVAL, "sdc_optim_plan: unknown kind %d (0 SGD, 1 Adam, 2 AdamW)", kind);
    int64_t chunks = 0;
    for (int i = 0; i < n; ++i) {
        SdcOptItem& it = items[i];
        SDC_REQUIRE(it.p && it.g && it.m, SDC_ENULL, "sdc_optim_plan: item %d: null p, g or m", i);
        SDC_REQUIRE(kind == SDC_OPT_SGD || it.v, SDC_ENULL, "sdc_optim_plan: item %d: null v (Adam / AdamW keep a second moment)", i);
        SDC_REQUIRE(aligned4(it.p) && aligned4(it.g) && aligned4(it.m) && aligned4(it.v) && aligned4(it.ema), SDC_EALIGN,
                    "sdc_optim_plan: item %d: pointer not 4-byte aligned", i);
        SDC_REQUIRE(it.n > 0, SDC_EINVAL, "sdc_optim_plan: item %d: n = %lld", i, (long long)it.n);
        it.chunk0 = chunks;
        chunks += (it.n + CHUNK - 1) / CHUNK;
        SDC_REQUIRE(chunks < (1ll << 30), SDC_EINVAL, "sdc_optim_plan: too many chunks");
    }
    *chunk = CHUNK;
    *total_chunks = (int)chunks;
    *grid = (int)(chunks < GRID_CAP ? chunks : GRID_CAP);
    return SDC_OK;
}

extern "C" size_t sdc_optim_bytes(int total_chunks) { return total_chunks > 0 ? (size_t)total_chunks * sizeof(double) : 0; }

extern "C" int sdc_optim_step(int kind, const SdcOptItem* items_dev, int n, int chunk, int total_chunks, int grid, const double* hp_dev,
                              SdcOptState* state_dev, void* work, int flags, void* stream) {
    SDC_REQUIRE(kind_ok(kind), SDC_EINVAL, "sdc_optim_step: unknown kind %d (0 SGD, 1 Adam, 2 AdamW)", kind);
    SDC_REQUIRE(items_dev && hp_dev && state_dev, SDC_ENULL, "sdc_optim_step: null pointer");
    SDC_REQUIRE(n > 0 && chunk == CHUNK && total_chunks >= n && grid > 0 && grid <= GRID_CAP && grid <= total_chunks, SDC_EINVAL,
                "sdc_optim_step: bad arguments (n, chunk, total_chunks and grid are those of sdc_optim_plan)");
    SDC_REQUIRE(!(flags & ~(SDC_OPT_CLIP | SDC_OPT_SKIP_NONFINITE)), SDC_EINVAL, "sdc_optim_step: unknown flags %d", flags);
    const int have_norm = flags != 0;
    SDC_REQUIRE(!have_norm || work, SDC_ENULL, "sdc_optim_step: null workspace (sdc_optim_bytes)");
    SDC_REQUIRE((reinterpret_cast<uintptr_t>(work) & 7u) == 0 && (reinterpret_cast<uintptr_t>(hp_dev) & 7u) == 0 &&
                (reinterpret_cast<uintptr_t>(state_dev) & 7u) == 0, SDC_EALIGN, "sdc_optim_step: hp, state and work must be 8-byte aligned");
    hipStream_t s = sdc::as_stream(stream);
    double* partial = static_cast<double*>(work);
    if (have_norm) hipLaunchKernelGGL(optim_norm_kernel, dim3((unsigned)grid), dim3(NT), 0, s, items_dev, n, total_chunks, partial);
    hipLaunchKernelGGL(optim_prepare_kernel, dim3(1), dim3(NT), 0, s, partial, total_chunks, hp_dev, state_dev, flags, have_norm);
    if (kind == SDC_OPT_SGD)
        hipLaunchKernelGGL(optim_update_kernel<SDC_OPT_SGD>, dim3((unsigned)grid), dim3(NT), 0, s, items_dev, n, total_chunks, hp_dev, state_dev);
    else if (kind == SDC_OPT_ADAM)
        hipLaunchKernelGGL(optim_update_kernel<SDC_OPT_ADAM>, dim3((unsigned)grid), dim3(NT), 0, s, items_dev, n, total_chunks, hp_dev, state_dev);
    else
        hipLaunchKernelGGL(optim_update_kernel<SDC_OPT_ADAMW>, dim3((unsigned)grid), dim3(NT), 0, s, items_dev, n, total_chunks, hp_dev, state_dev);
    return sdc::check_launch("sdc_optim_step");
}
