// Fine-tuning precision 6 / 7 (net.train_precision): the weight gradient of the stride-1 pad-1 3-tap convs -- Conv1d k3 (1x1x3),
// Conv2d 3x3 (1x3x3), Conv3d 3x3x3 -- on the gfx950 16-bit matrix pipe, v_mfma_f32_32x32x16_f16: fp16 operands, fp32 accumulation,
// fp32 tensors in HBM; and the per-tensor power-of-two scale of the loss gradient that keeps those operands in fp16's normal range.
//
//   dW[m][n][kd][kh][kw] = 2^-e sum_p  fp16(2^e G[m][p]) fp16(X[n][p + (kd, kh, kw) - 1])      p = (b, od, oh, ow)
//
// GEMM per (kd, 64 m x 64 n tile): C[m][n] (one per (kh, kw) tap) = sum_k A[m][k] B[k][n], k = output positions, 16 per MFMA.
// Stage = 128 consecutive output positions (R = 128 / W whole rows): the G rows [64 m][128 positions] and the X rows they reach
// through the kh taps -- the stage's rows plus a halo row above and below every run of rows inside one (sample, depth) plane,
// as in conv_f16_kernel -- are read as fp32, rounded to fp16 (RNE; G times 2^e first) and staged once into LDS:
// G as [m][position], X as [staged row][n][column] with 8 zero columns on either side.  Each staged X row serves every kh tap
// (an LDS row offset), and the kw shift is an LDS column offset: the centre tap's 8-position fragment is one 16-byte read, the
// outer taps' fragments are the same 16 bytes shifted by one half against the 4-byte words on either side (v_alignbyte).
// Wave (wm, wn) owns 32 m x 32 n x every (kh, kw) tap: 9 (3x3, 3x3x3) or 3 (1x3) accumulator blocks; per 16 positions one
// A fragment feeds 3 KH MFMAs.
//
// The positions are split over workgroups (grid.y), each writing a partial copy of the gradient that a second pass sums in split
// order: deterministic, no atomics.  Every fp16 x fp16 product is exact in fp32, so dW differs from an fp64 weight gradient of the
// ROUNDED operands by fp32 summation order only.  The bias gradient is an fp32 sum of the unscaled G (fixed order).
#include "sdc_common.h"
#include "sdc_f16frag.h"
#include <cmath>
#include <cstring>

namespace {

typedef _Float16 half4 __attribute__((ext_vector_type(4)));

constexpr int WF_NT = 256;
constexpr int WF_P = 128;                  // output positions per stage
constexpr int WF_XH = 8;                   // zero halo columns on either side of a staged X row (keeps the centre tap 16-byte aligned)
constexpr size_t WF_LDS_MAX = 80u * 1024u; // two workgroups per CU
constexpr int WF_EXP_PARTS = 1024;         // first-pass workgroups of sdc_f16_grad_exponent (SDC_F16_EXP_INTS = 1 + this)

struct WgF16Args {
    const float* g;
    const float* x;
    const int32_t* gexp;
    float* part;              // [nsplit][M][N][kD][kH][3] (one split: dw itself)
    int64_t gs[5], xs[5];
    int M, N, B, oD, oH, W, lgW, kD;
    int R, Hs, NR;            // rows per stage, rows per halo'd run, staged X rows
    int Ntot, nstages, sps, Mt, Nt;
    int gpitch, xpitch, ldsX; // bytes per staged G channel row, per staged X (row, channel), byte offset of the X image
    int gvec, xvec;           // the rows of G / X are contiguous and 16-byte aligned: float4 loads
};

__device__ __forceinline__ uint32_t shift_half(uint32_t hi, uint32_t lo) { return __builtin_amdgcn_alignbyte(hi, lo, 2); }

template <int KH>
__global__ __launch_bounds__(WF_NT, 2) void wgrad_f16_kernel(const WgF16Args a) {
    constexpr int HH = KH - 1;
    constexpr int NACC = 3 * KH;
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, l31 = lane & 31, lh = lane >> 5;
    int tb = blockIdx.x;
    const int kd = tb % a.kD; tb /= a.kD;
    const int nt = tb % a.Nt;
    const int mt = tb / a.Nt;
    const int m0 = mt * 64, n0 = nt * 64;
    const int s_lo = (int)blockIdx.y * a.sps;
    const int s_hi = min(a.nstages, s_lo + a.sps);
    const int W = a.W;
    const int dk = kd - a.kD / 2;
    const int e = *a.gexp;
    const float gsc = __builtin_ldexpf(1.0f, e), gunsc = __builtin_ldexpf(1.0f, -e);

    // zero halo columns (never overwritten: the staged columns are WF_XH .. WF_XH + W - 1)
    for (int i = tid; i < a.NR * 64 * 2; i += WF_NT) {
        const int side = i & 1, rc = i >> 1;
        *reinterpret_cast<uint4*>(lds + a.ldsX + rc * a.xpitch + (side ? (W + WF_XH) * 2 : 0)) = make_uint4(0u, 0u, 0u, 0u);
    }

    f32x16 acc[NACC];
#pragma unroll
    for (int t = 0; t < NACC; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;

    const int aoff = (wm * 32 + l31) * a.gpitch + 16 * lh;
    const int boff = a.ldsX + (wn * 32 + l31) * a.xpitch + (WF_XH + 8 * lh) * 2;
    const int xrow = 64 * a.xpitch;
    const int nrows = a.Ntot >> a.lgW;

    for (int s = s_lo; s < s_hi; ++s) {
        const int p0 = s * WF_P, r0 = p0 >> a.lgW;
        __syncthreads();                                        // the previous stage's fragments are read
        // ---- G: (m, 4 positions) items, scaled by 2^e, rounded
        for (int it = tid; it < 64 * (WF_P / 4); it += WF_NT) {
            const int q = it % (WF_P / 4), m = it / (WF_P / 4);
            const int p = p0 + 4 * q;
            float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (m0 + m < a.M && p < a.Ntot) {
                const int row = p >> a.lgW, col = p & (W - 1);
                const int oh = row % a.oH, pl = row / a.oH, od = pl % a.oD, b = pl / a.oD;
                const float* src = a.g + (int64_t)b * a.gs[0] + (int64_t)(m0 + m) * a.gs[1] + (int64_t)od * a.gs[2] +
                                   (int64_t)oh * a.gs[3] + (int64_t)col * a.gs[4];
                if (a.gvec) {
                    const float4 f = *reinterpret_cast<const float4*>(src);
                    v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i) v[i] = src[(int64_t)i * a.gs[4]];
                }
            }
            half4 h;
#pragma unroll
            for (int i = 0; i < 4; ++i) h[i] = (_Float16)(v[i] * gsc);           // exact scaling, then RNE
            *reinterpret_cast<half4*>(lds + m * a.gpitch + (4 * q) * 2) = h;
        }
        // ---- X: (staged row, n, 4 columns) items
        const int xitems = a.NR * 64 * (W / 4);
        for (int it = tid; it < xitems; it += WF_NT) {
            const int q = it % (W / 4), rest = it / (W / 4);
            const int n = rest % 64, sr = rest / 64;
            const int seg = sr / (a.Hs + HH), qq = sr - seg * (a.Hs + HH);
            const int rs = r0 + seg * a.Hs;
            int row, sh;
            if (KH == 3) { row = rs; sh = rs % a.oH + qq - 1; }
            else { row = rs + qq; sh = row % a.oH; }
            const int pl = row / a.oH;
            const int od = pl % a.oD, b = pl / a.oD, sd = od + dk;
            float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (n0 + n < a.N && row < nrows && sh >= 0 && sh < a.oH && sd >= 0 && sd < a.oD) {
                const float* src = a.x + (int64_t)b * a.xs[0] + (int64_t)(n0 + n) * a.xs[1] + (int64_t)sd * a.xs[2] +
                                   (int64_t)sh * a.xs[3] + (int64_t)(4 * q) * a.xs[4];
                if (a.xvec) {
                    const float4 f = *reinterpret_cast<const float4*>(src);
                    v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i) v[i] = src[(int64_t)i * a.xs[4]];
                }
            }
            half4 h;
#pragma unroll
            for (int i = 0; i < 4; ++i) h[i] = (_Float16)v[i];
            *reinterpret_cast<half4*>(lds + a.ldsX + (sr * 64 + n) * a.xpitch + (WF_XH + 4 * q) * 2) = h;
        }
        __syncthreads();
        // ---- MFMAs: every output row of the stage, 16 positions per k step
        const int rend = min(a.R, nrows - r0);
        for (int rl = 0; rl < rend; ++rl) {
            const int srow = KH == 3 ? (rl / a.Hs) * (a.Hs + 2) + rl % a.Hs : rl;
            for (int k0 = 0; k0 < W; k0 += 16) {
                const half8 af = *reinterpret_cast<const half8*>(lds + aoff + (rl * W + k0) * 2);
#pragma unroll
                for (int kh = 0; kh < KH; ++kh) {
                    const char* bp = lds + boff + (srow + kh) * xrow + k0 * 2;
                    const uint4 dv = *reinterpret_cast<const uint4*>(bp);
                    const uint32_t dm = *reinterpret_cast<const uint32_t*>(bp - 4);
                    const uint32_t dp = *reinterpret_cast<const uint32_t*>(bp + 16);
                    const uint4 v0 = make_uint4(shift_half(dv.x, dm), shift_half(dv.y, dv.x), shift_half(dv.z, dv.y), shift_half(dv.w, dv.z));
                    const uint4 v2 = make_uint4(shift_half(dv.y, dv.x), shift_half(dv.z, dv.y), shift_half(dv.w, dv.z), shift_half(dp, dv.w));
                    half8 b0, b1, b2;
                    __builtin_memcpy(&b0, &v0, 16);
                    __builtin_memcpy(&b1, &dv, 16);
                    __builtin_memcpy(&b2, &v2, 16);
                    acc[kh * 3 + 0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af, b0, acc[kh * 3 + 0], 0, 0, 0);
                    acc[kh * 3 + 1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af, b1, acc[kh * 3 + 1], 0, 0, 0);
                    acc[kh * 3 + 2] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af, b2, acc[kh * 3 + 2], 0, 0, 0);
                }
            }
        }
    }

    // ---- epilogue: 2^-e (exact), partial copy of this split in nn.Conv layout
    const int taps = a.kD * KH * 3;
    float* out = a.part + (int64_t)blockIdx.y * a.M * a.N * taps;
    const int n = n0 + wn * 32 + l31;
#pragma unroll
    for (int t = 0; t < NACC; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = m0 + wm * 32 + 4 * lh + (r & 3) + 8 * (r >> 2);
            if (m < a.M && n < a.N) out[((int64_t)m * a.N + n) * taps + kd * KH * 3 + t] = acc[t][r] * gunsc;
        }
}

// dw[i] = sum_s part[s][i], splits in order
__global__ __launch_bounds__(256) void wgrad_f16_sum_kernel(const float* __restrict__ part, float* __restrict__ out, int64_t n, int nsplit) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float s = 0.0f;
    for (int k = 0; k < nsplit; ++k) s += part[(int64_t)k * n + i];
    out[i] = s;
}

// dbias[m] = sum over (b, positions) of the unscaled G in fp32: thread t sums the positions t, t + 256, ... of the flattened
// (b, od, oh, ow) order, the 256 partial sums are added in a fixed tree order
__global__ __launch_bounds__(256) void wgrad_f16_bias_kernel(const float* __restrict__ g, float* __restrict__ db, int64_t g0, int64_t g1,
                                                             int64_t g2, int64_t g3, int64_t g4, int oD, int oH, int W, int Ntot) {
    __shared__ float sh[256];
    const int m = blockIdx.x;
    float s = 0.0f;
    for (int p = threadIdx.x; p < Ntot; p += 256) {
        const int col = p % W, row = p / W;
        const int oh = row % oH, pl = row / oH, od = pl % oD, b = pl / oD;
        s += g[(int64_t)b * g0 + (int64_t)m * g1 + (int64_t)od * g2 + (int64_t)oh * g3 + (int64_t)col * g4];
    }
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) sh[threadIdx.x] += sh[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) db[m] = sh[0];
}

struct WfShape { int R, Hs, NR, gpitch, xpitch; size_t lds; };

WfShape wf_shape(const SdcWgradDesc& d) {
    WfShape sh{};
    sh.R = WF_P / d.oW;
    sh.Hs = d.kH == 3 ? (d.oH < sh.R ? d.oH : sh.R) : sh.R;
    sh.NR = (sh.R / sh.Hs) * (sh.Hs + d.kH - 1);
    sh.gpitch = WF_P * 2 + 16;
    sh.xpitch = (d.oW + 2 * WF_XH) * 2 + 16;
    sh.lds = (size_t)64 * sh.gpitch + (size_t)sh.NR * 64 * sh.xpitch;
    return sh;
}

// coverage: the conv_f16_kernel tap shapes at stride 1, pad 1 along every 3-wide axis, no upsampling, same size in and out, rows
// of 16 / 32 / 64 / 128 positions, whole rows per stage (3-row taps: a plane's rows are a multiple or a divisor of the stage's)
bool wf_covered(const SdcWgradDesc& d) {
    const bool taps = d.kW == 3 && ((d.kD == 1 && d.kH == 1) || ((d.kD == 1 || d.kD == 3) && d.kH == 3));
    if (!taps) return false;
    if (!(d.sD == 1 && d.sH == 1 && d.sW == 1 && d.uD == 1 && d.uH == 1 && d.uW == 1 && d.pW == 1 && d.pH == d.kH / 2 &&
          d.pD == d.kD / 2 && d.iD == d.oD && d.iH == d.oH && d.iW == d.oW)) return false;
    if (!(d.oW == 16 || d.oW == 32 || d.oW == 64 || d.oW == 128)) return false;
    const int R = WF_P / d.oW;
    if (d.kH == 3 && !(d.oH % R == 0 || R % d.oH == 0)) return false;
    if ((int64_t)d.B * d.oD * d.oH * d.oW >= (1ll << 31)) return false;
    return wf_shape(d).lds <= WF_LDS_MAX;
}

// The dispatch table of precision 6 (tools/f16_train_step.py --shapes, fp32 sdc_conv_wgrad against this kernel on
// the fine-tuning convs of the C2 / C3 / C4 steps): the rows where this kernel is ahead.  Keyed on channel counts and row width only.
//   1x3:   rows of 16 / 32 / 64 with M N >= 512 x 256 (x1.32-1.85); rows of 128, or 256 x 256 channels, stay fp32 (x0.79-0.84).
//   3x3x3: M N >= 128 x 256 (x1.21-1.44), and 128 x 128 over rows of >= 32 (x1.23); smaller ones stay fp32 (x0.55-0.85).
//   3x3:   never (x0.21-0.64 against the merged-kh fp32 kernel).
bool wf_faster(const SdcWgradDesc& d) {
    const int64_t mn = (int64_t)d.M * d.N;
    if (d.kD == 3) return mn >= 128 * 256 || (mn >= 128 * 128 && d.oW >= 32);
    if (d.kH == 1) return d.oW <= 64 && mn >= 512 * 256;
    return false;
}

bool wf_runs(const SdcWgradDesc& d) {
    return (d.precision == 7 || (d.precision == 6 && wf_faster(d))) && wf_covered(d);
}

int wf_splits(const SdcWgradDesc& d, int nstages, int* sps) {
    const int64_t tiles = (int64_t)((d.M + 63) / 64) * ((d.N + 63) / 64) * d.kD;
    int64_t want = (512 + tiles - 1) / tiles;
    const int64_t nw = (int64_t)d.M * d.N * d.kD * d.kH * d.kW;
    const int64_t cap = (64ll << 20) / nw;
    if (want > cap) want = cap;
    if (want > nstages) want = nstages;
    if (want < 1) want = 1;
    *sps = (int)((nstages + want - 1) / want);
    return (nstages + *sps - 1) / *sps;
}

size_t wf_bytes(const SdcWgradDesc& d) {
    const int nstages = (int)(((int64_t)d.B * d.oD * d.oH * d.oW + WF_P - 1) / WF_P);
    int sps;
    const int ns = wf_splits(d, nstages, &sps);
    return ns == 1 ? 0 : (size_t)ns * d.M * d.N * d.kD * d.kH * d.kW * sizeof(float);
}

bool vec_rows(const float* p, const int64_t* st) {
    return st[4] == 1 && ((st[0] | st[1] | st[2] | st[3]) & 3) == 0 && (reinterpret_cast<uintptr_t>(p) & 15) == 0;
}

// |G| maximum of a 5-D strided tensor as float bits (NaN above inf above every finite value); pass 1: one partial per workgroup
__global__ __launch_bounds__(256) void grad_amax_kernel(const float* __restrict__ g, int C, int D, int H, int W, int64_t s0, int64_t s1,
                                                        int64_t s2, int64_t s3, int64_t s4, int64_t n, int dense, uint32_t* __restrict__ part) {
    __shared__ uint32_t sh[256];
    uint32_t mx = 0u;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        float v;
        if (dense) v = g[i];
        else {
            int64_t r = i;
            const int w = (int)(r % W); r /= W;
            const int h = (int)(r % H); r /= H;
            const int dd = (int)(r % D); r /= D;
            const int c = (int)(r % C);
            const int64_t b = r / C;
            v = g[b * s0 + (int64_t)c * s1 + (int64_t)dd * s2 + (int64_t)h * s3 + (int64_t)w * s4];
        }
        const uint32_t u = __float_as_uint(v) & 0x7fffffffu;
        mx = u > mx ? u : mx;
    }
    sh[threadIdx.x] = mx;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h && sh[threadIdx.x + h] > sh[threadIdx.x]) sh[threadIdx.x] = sh[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = sh[0];
}

// pass 2: e with max|G| 2^e in [2^14, 2^15) (0 when the maximum is 0 or not finite), clamped to [-126, 126]
__global__ __launch_bounds__(256) void grad_exp_kernel(const uint32_t* __restrict__ part, int nparts, int32_t* __restrict__ e) {
    __shared__ uint32_t sh[256];
    uint32_t mx = 0u;
    for (int i = threadIdx.x; i < nparts; i += 256) mx = part[i] > mx ? part[i] : mx;
    sh[threadIdx.x] = mx;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h && sh[threadIdx.x + h] > sh[threadIdx.x]) sh[threadIdx.x] = sh[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const uint32_t m = sh[0];
        int r = 0;
        if (m != 0u && m < 0x7f800000u) {
            r = 14 - ilogbf(__uint_as_float(m));
            r = r < -126 ? -126 : (r > 126 ? 126 : r);
        }
        e[0] = r;
    }
}

}  // namespace

extern "C" int sdc_f16_grad_exponent(const float* g, int B, int C, int D, int H, int W, const int64_t* strides, int32_t* e, void* stream) {
    SDC_REQUIRE(g && strides && e, SDC_ENULL, "sdc_f16_grad_exponent: null pointer");
    SDC_REQUIRE(B > 0 && C > 0 && D > 0 && H > 0 && W > 0, SDC_EINVAL, "sdc_f16_grad_exponent: bad sizes");
    const int64_t n = (int64_t)B * C * D * H * W;
    const bool dense = strides[4] == 1 && strides[3] == W && strides[2] == (int64_t)H * W && strides[1] == (int64_t)D * H * W &&
                       strides[0] == (int64_t)C * D * H * W;
    int64_t nb = (n + 256 * 16 - 1) / (256 * 16);
    if (nb > WF_EXP_PARTS) nb = WF_EXP_PARTS;
    uint32_t* part = reinterpret_cast<uint32_t*>(e + 1);
    hipStream_t s = sdc::as_stream(stream);
    hipLaunchKernelGGL(grad_amax_kernel, dim3((unsigned)nb), dim3(256), 0, s, g, C, D, H, W, strides[0], strides[1], strides[2], strides[3],
                       strides[4], n, dense ? 1 : 0, part);
    { const int rc = sdc::check_launch("sdc_f16_grad_exponent"); if (rc) return rc; }
    hipLaunchKernelGGL(grad_exp_kernel, dim3(1), dim3(256), 0, s, part, (int)nb, e);
    return sdc::check_launch("sdc_f16_grad_exponent[finish]");
}

extern "C" size_t sdc_conv_wgrad_f16_bytes(const SdcWgradDesc* dp) {
    if (!dp) return 0;
    const size_t b32 = sdc_conv_wgrad_bytes(dp);
    if (!wf_runs(*dp)) return b32;
    const size_t b16 = wf_bytes(*dp);
    return b16 > b32 ? b16 : b32;
}

extern "C" int sdc_conv_wgrad_describe(const SdcWgradDesc* dp, char* name, size_t cap) {
    SDC_REQUIRE(dp, SDC_ENULL, "sdc_conv_wgrad_describe: null pointer");
    const SdcWgradDesc& d = *dp;
    const char* nm;
    if (wf_runs(d)) nm = d.kD == 3 ? "wgrad_f16_kernel<3x3x3>" : (d.kH == 3 ? "wgrad_f16_kernel<3x3>" : "wgrad_f16_kernel<1x3>");
    else {
        const bool mkh = ((d.kW == 3 && d.kH == 3 && d.pH == 1 && d.pW == 1) || (d.kW == 7 && d.kH == 7 && d.pH == 3 && d.N * 7 <= 64)) &&
                         d.sW == 1 && d.sH == 1 && d.uH == 1 && d.iH == d.oH &&
                         (d.oW == 16 || d.oW == 32 || d.oW == 64 || (d.kW == 3 && d.oW > 64 && d.oW % 64 == 0 && d.oW <= 1024));
        nm = mkh ? "wgrad_mkh_kernel" : "wgrad_kernel";
    }
    if (name && cap) { std::strncpy(name, nm, cap - 1); name[cap - 1] = 0; }
    return SDC_OK;
}

extern "C" int sdc_conv_wgrad_f16(const SdcWgradDesc* dp, const float* g, const float* x, const int32_t* e, float* dw, float* dbias,
                                  void* work, size_t work_bytes, void* stream) {
    SDC_REQUIRE(dp && g && x && e && dw && work, SDC_ENULL, "sdc_conv_wgrad_f16: null pointer");
    const SdcWgradDesc& d = *dp;
    SDC_REQUIRE(d.precision == 6 || d.precision == 7, SDC_EINVAL, "sdc_conv_wgrad_f16: descriptor precision must be 6 or 7");
    SDC_REQUIRE(work_bytes >= sdc_conv_wgrad_f16_bytes(dp), SDC_EINVAL, "sdc_conv_wgrad_f16: workspace too small");
    if (!wf_runs(d)) return sdc_conv_wgrad(dp, g, x, dw, dbias, work, work_bytes, stream);
    SDC_REQUIRE(d.B > 0 && d.M > 0 && d.N > 0, SDC_EINVAL, "sdc_conv_wgrad_f16: bad sizes");
    const WfShape sh = wf_shape(d);
    WgF16Args a;
    a.g = g; a.x = x; a.gexp = e;
    for (int i = 0; i < 5; ++i) { a.gs[i] = d.gs[i]; a.xs[i] = d.xs[i]; }
    a.M = d.M; a.N = d.N; a.B = d.B; a.oD = d.oD; a.oH = d.oH; a.W = d.oW; a.kD = d.kD;
    a.lgW = d.oW == 16 ? 4 : d.oW == 32 ? 5 : d.oW == 64 ? 6 : 7;
    a.R = sh.R; a.Hs = sh.Hs; a.NR = sh.NR;
    a.Ntot = d.B * d.oD * d.oH * d.oW;
    a.nstages = (a.Ntot + WF_P - 1) / WF_P;
    const int nsplit = wf_splits(d, a.nstages, &a.sps);
    a.Mt = (d.M + 63) / 64; a.Nt = (d.N + 63) / 64;
    a.gpitch = sh.gpitch; a.xpitch = sh.xpitch; a.ldsX = 64 * sh.gpitch;
    a.gvec = vec_rows(g, d.gs); a.xvec = vec_rows(x, d.xs);
    const int64_t nw = (int64_t)d.M * d.N * d.kD * d.kH * d.kW;
    a.part = nsplit == 1 ? dw : static_cast<float*>(work);
    const int64_t tiles = (int64_t)a.Mt * a.Nt * d.kD;
    SDC_REQUIRE(tiles < (1ll << 31) && nsplit < 65536, SDC_EINVAL, "sdc_conv_wgrad_f16: grid too large");
    const dim3 grid((unsigned)tiles, (unsigned)nsplit);
    hipStream_t s = sdc::as_stream(stream);
    if (d.kH == 3) {
        static std::atomic<uint64_t> attr{0};
        SDC_LDS_OPTIN(attr, wgrad_f16_kernel<3>, 160 * 1024, "sdc_conv_wgrad_f16");
        hipLaunchKernelGGL(wgrad_f16_kernel<3>, grid, dim3(WF_NT), sh.lds, s, a);
    } else {
        static std::atomic<uint64_t> attr{0};
        SDC_LDS_OPTIN(attr, wgrad_f16_kernel<1>, 160 * 1024, "sdc_conv_wgrad_f16");
        hipLaunchKernelGGL(wgrad_f16_kernel<1>, grid, dim3(WF_NT), sh.lds, s, a);
    }
    { const int rc = sdc::check_launch("sdc_conv_wgrad_f16"); if (rc) return rc; }
    if (nsplit > 1) {
        hipLaunchKernelGGL(wgrad_f16_sum_kernel, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, s, a.part, dw, nw, nsplit);
        const int rc = sdc::check_launch("sdc_conv_wgrad_f16[reduce]");
        if (rc) return rc;
    }
    if (dbias) {
        hipLaunchKernelGGL(wgrad_f16_bias_kernel, dim3((unsigned)d.M), dim3(256), 0, s, g, dbias, d.gs[0], d.gs[1], d.gs[2], d.gs[3], d.gs[4],
                           d.oD, d.oH, d.oW, a.Ntot);
        return sdc::check_launch("sdc_conv_wgrad_f16[bias]");
    }
    return SDC_OK;
}
