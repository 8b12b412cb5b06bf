// Backward of the fused temporal-attention block (sdc_tablock.hip) for fine-tuning: given dy, the gradient of
//
//   y = x + Wo . softmax( rot(s Wq xn) rot(Wk xn)^T + relpos ) (Wv xn),   xn = channel LayerNorm(x) * gamma
//
// with respect to x, gamma, Wqkv, Wo and the relative-position bias, without any intermediate tensor in HBM: xn, q/k/v, P, O, dO,
// dq/dk/dv and dxn are recomputed from x and dy and never leave the chip.  fp32 MFMA products, fp32 accumulation; LayerNorm,
// scale-in-the-exponent, rotary and softmax as ta_block_kernel has them, the core's two orientations as tattn_bwd_kernel
// (sdc_attn_bwd.hip) has them.
//
// Persistent workgroups walk the 8-pixel groups as the forward does (ta_walk).  A group is worked in two passes of 4 pixels
// (128 tokens): the xn and dy images of 8 pixels plus the core's four [d][frame] images would need 270 KB.  Per pass:
//   A. x, dy -> registers (four threads per token, 16 channels each) -> LayerNorm statistics -> xn and dy images in LDS
//   per head (eight waves = 4 pixels x 2 roles):
//   P1. role 0: q, k = W_h xn (K = 64), rotary;  role 1: v = W_h xn, dO^T = Wo_h dy (K = 64)        -> [d][frame] images
//   P2. both roles: S^T = K'Q'^T + bias, dP^T = V dO^T, row statistics, D (lanes = queries);
//       role 0: dS^T, dq'^T = K' dS^T, O^T = V P^T;
//       role 1: S, dP with lanes = keys (statistics through the wave's own LDS words) -> dS, dk'^T = Q' dS, dv^T = dO^T P;
//       the bias gradient stays in registers over the whole walk: role 0 keeps dS^T of heads 0 and 1, role 1 dS of heads 2 and 3;
//       inverse rotary and the scale on dq', dk' in registers; the results replace the q, k, v, dO images (O over dO)
//   P3. dxn[c][f] += sum_d W[c][d] d{q,k,v}[d][f] (a wave owns one pixel and 32 channels, accumulators carried over the heads);
//       the eight waves own one 32 x 32 tile each of dWq, dWk, dWv, dWo of this head: K = the pass's 128 tokens, accumulators
//       (16 registers per head) carried over the whole walk
//   B. dxn through LDS -> LayerNorm backward + residual: dx = dy + rstd (g dxn - mean_c(g dxn) - xh mean_c(g dxn xh)), dg += dxn xh
// The weights are read from global memory (L1 / L2 resident, 128 KB): along the contraction index for the projections and in
// 16-byte runs along d / co where the transposed matrix is the operand (the contraction order of an MFMA chain is free).
// Deterministic: no atomics; a workgroup leaves one partial table (dWqkv | dWo | dbias | dg), every workgroup writes all of its
// table, and tab_sum_kernel adds the tables in a fixed order.
#define TA_WEIGHT_ARGS const float* wqkv; const float* wo; const float* dy; float* part;
#include "sdc_tablock_tile.h"

namespace {

constexpr int RP = 4 * 33 + 1;                 // row pitch of the xn / dy images [64 c][4 pixels][33]: odd, so that lanes = channels
                                               // (weight-gradient operands) are conflict-free too
constexpr int IMG = 32 * 33;                   // one [d][frame] image
constexpr int P_WQKV = 0, P_WO = 64 * 384, P_BIAS = P_WO + 128 * 64, P_G = P_BIAS + 4 * 32 * 32;
constexpr int PART = P_G + 64;                 // floats of one workgroup's partial table
constexpr int MAXWG = 256;                     // the workspace is sized for at most this many workgroups
constexpr float SCALE = 0.17677669529663687f;  // dim_head^-0.5
constexpr float SL = 0.17677669529663687f * 1.4426950408889634f;
constexpr int LDS_FLOATS = 2 * C * RP + 16 * IMG + IMG + 1024 + 8 * 96 + 256 + 1024;

#define MFMA(a_, b_, c_) __builtin_amdgcn_mfma_f32_32x32x2f32(a_, b_, c_, 0, 0, 0)

__global__ __launch_bounds__(NT) void ta_block_bwd_kernel(const TaArgs a) {
    extern __shared__ float lds[];
    float* const xs = lds;                       // [64][RP]  xn; after the heads dxn
    float* const dys = xs + C * RP;              // [64][RP]  dy
    float* const img = dys + C * RP;             // [q, k, v, dO][4 pixels][32 d][33]; after P2: dq, dk, dv, O
    float* const bs = img + 16 * IMG;            // [query][33] bias / scale of the current head
    float* const rotcs = bs + IMG;               // [16 m][32 frames][2]
    float* const stat = rotcs + 1024;            // [wave][3][32]: -max * SL, 1 / row sum, D
    float* const lnst = stat + 8 * 96;           // [2][128] mean, rstd of the pass's tokens
    float* const red = lnst + 256;               // [2][4][128] partial sums

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lh = lane >> 5;
    const int px = wave & 3, role = wave >> 2;
    const TaWalk wk = ta_walk(a.nblk);
    const int tok = tid & 127, qt = tid >> 7, pw = tok & 3, f = tok >> 2;       // LayerNorm phases: token (pixel pw, frame f), channels 16 qt ..
    const uint32_t toff = (uint32_t)(((int64_t)f * a.st + pw + (int64_t)(qt * 16) * a.sc) * 4);

    {   // tid = frame * 16 + m
        const float2 rr = a.rot ? *reinterpret_cast<const float2*>(a.rot + tid * 2) : make_float2(1.0f, 0.0f);
        *reinterpret_cast<float2*>(rotcs + (((tid & 15) * 32) + (tid >> 4)) * 2) = rr;
    }
    f32x16 dwacc[4], dbacc[2];         // dbacc: role 0 keeps dS^T of heads 0, 1, role 1 keeps dS of heads 2, 3 (each (pixel, head) once)
    float dgacc[16];
#pragma unroll
    for (int h = 0; h < 4; ++h)
#pragma unroll
        for (int r = 0; r < 16; ++r) { dwacc[h][r] = 0.f; dbacc[h >> 1][r] = 0.f; }
#pragma unroll
    for (int c = 0; c < 16; ++c) dgacc[c] = 0.f;
    float* const st_m = stat + wave * 96, * const st_l = st_m + 32, * const st_d = st_m + 64;

    // transposed rotation of a [d rows][frame lanes] accumulator (pairs d, d + 1 = registers r, r + 1), times the scale
    auto unrot = [&](f32x16& t) {
#pragma unroll
        for (int r = 0; r < 16; r += 2) {
            const int m = crow(r, lh) >> 1;
            const float2 cs = *reinterpret_cast<const float2*>(rotcs + (m * 32 + l31) * 2);
            const float y0 = t[r], y1 = t[r + 1];
            t[r] = (y0 * cs.x + y1 * cs.y) * SCALE;
            t[r + 1] = (y1 * cs.x - y0 * cs.y) * SCALE;
        }
    };

    for (int li = wk.first; li < wk.per; li += wk.stride) {
        const int64_t tp = ta_tile_ptr(a, wk, li);
#pragma unroll 1
        for (int hp = 0; hp < 2; ++hp) {
            const float* xt = a.x + tp + hp * 4;
            const float* dyt = a.dy + tp + hp * 4;
            float* dxt = a.y + tp + hp * 4;
            // ---- A. LayerNorm; xn and dy images
            {
                float v[16], gy[16];
#pragma unroll
                for (int c = 0; c < 16; ++c) { v[c] = ldu(uni(xt + (int64_t)c * a.sc), toff); gy[c] = ldu(uni(dyt + (int64_t)c * a.sc), toff); }
                float sm = 0.f;
#pragma unroll
                for (int c = 0; c < 16; ++c) sm += v[c];
                red[qt * 128 + tok] = sm;
                __syncthreads();
                const float mean = ((red[tok] + red[128 + tok]) + (red[256 + tok] + red[384 + tok])) * (1.0f / C);
                float q = 0.f;
#pragma unroll
                for (int c = 0; c < 16; ++c) { v[c] -= mean; q += v[c] * v[c]; }
                red[512 + qt * 128 + tok] = q;
                __syncthreads();
                const float rstd = rsqrtf(((red[512 + tok] + red[640 + tok]) + (red[768 + tok] + red[896 + tok])) * (1.0f / C) + a.eps);
#pragma unroll
                for (int c = 0; c < 16; ++c) {
                    xs[(qt * 16 + c) * RP + pw * 33 + f] = v[c] * rstd * a.g[qt * 16 + c];
                    dys[(qt * 16 + c) * RP + pw * 33 + f] = gy[c];
                }
                if (qt == 0) { lnst[tok] = mean; lnst[128 + tok] = rstd; }
            }
            f32x16 dxacc;
#pragma unroll
            for (int r = 0; r < 16; ++r) dxacc[r] = 0.f;
#pragma unroll 1
            for (int h = 0; h < 4; ++h) {              // (rolled: the accumulators of head h are picked by a switch)
                __syncthreads();                       // the images of the pass / the previous head's P3 is done with img and bs
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const int e = tid + i * NT;
                    bs[(e >> 5) * 33 + (e & 31)] = a.bias ? a.bias[h * 1024 + e] * 5.65685424949238f : 0.0f;
                }
                // ---- P1. projections of pixel px
                {
                    f32x16 pa, pb;
#pragma unroll
                    for (int r = 0; r < 16; ++r) { pa[r] = 0.f; pb[r] = 0.f; }
                    const float* wp = a.wqkv + h * 32 + l31 + lh * 384;          // k-step ks: c = 2 ks + lh
                    const float* xp = xs + lh * RP + px * 33 + l31;
                    if (role == 0) {
#pragma unroll 8
                        for (int ks = 0; ks < 32; ++ks) {
                            const float xv = xp[2 * ks * RP];
                            pa = MFMA(wp[2 * ks * 384], xv, pa);
                            pb = MFMA(wp[2 * ks * 384 + 128], xv, pb);
                        }
#pragma unroll
                        for (int r = 0; r < 16; r += 2) {
                            const int m = crow(r, lh) >> 1;
                            const float2 cs = *reinterpret_cast<const float2*>(rotcs + (m * 32 + l31) * 2);
                            const float q0 = pa[r], q1 = pa[r + 1], k0 = pb[r], k1 = pb[r + 1];
                            pa[r] = fmaf(-q1, cs.y, q0 * cs.x); pa[r + 1] = fmaf(q0, cs.y, q1 * cs.x);
                            pb[r] = fmaf(-k1, cs.y, k0 * cs.x); pb[r + 1] = fmaf(k0, cs.y, k1 * cs.x);
                        }
                    } else {
                        // Wo[h*32 + d = l31][co = 32 lh ..] in 16-byte runs: k-step ks: co = ks + 32 lh
                        const nfloat4* w4 = reinterpret_cast<const nfloat4*>(a.wo + (h * 32 + l31) * 64 + 32 * lh);
                        const float* gp = dys + (32 * lh) * RP + px * 33 + l31;
#pragma unroll 2
                        for (int i = 0; i < 8; ++i) {
                            const nfloat4 t = w4[i];
                            const float wv[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
                            for (int j = 0; j < 4; ++j) {
                                const int ks = 4 * i + j;
                                pa = MFMA(wp[2 * ks * 384 + 256], xp[2 * ks * RP], pa);
                                pb = MFMA(wv[j], gp[ks * RP], pb);
                            }
                        }
                    }
                    float* ia = img + ((role ? 8 : 0) + px) * IMG, * ib = img + ((role ? 12 : 4) + px) * IMG;
#pragma unroll
                    for (int r = 0; r < 16; ++r) { ia[crow(r, lh) * 33 + l31] = pa[r]; ib[crow(r, lh) * 33 + l31] = pb[r]; }
                }
                __syncthreads();
                // ---- P2. the core of (pixel px, head h)
                float* const Qi = img + px * IMG, * const Ki = Qi + 4 * IMG, * const Vi = Qi + 8 * IMG, * const Gi = Qi + 12 * IMG;
                f32x16 o1, o2;
#pragma unroll
                for (int r = 0; r < 16; ++r) { o1[r] = 0.f; o2[r] = 0.f; }
                {
                    f32x16 sT, dpT;                    // [key rows][query lanes]
#pragma unroll
                    for (int r = 0; r < 16; ++r) { sT[r] = bs[l31 * 33 + crow(r, lh)]; dpT[r] = 0.f; }
#pragma unroll
                    for (int s2 = 0; s2 < 16; ++s2) {
                        const int e = (2 * s2 + lh) * 33 + l31;
                        sT = MFMA(Ki[e], Qi[e], sT);
                        dpT = MFMA(Vi[e], Gi[e], dpT);
                    }
                    float mx = -INFINITY;
#pragma unroll
                    for (int r = 0; r < 16; ++r) mx = fmaxf(mx, sT[r]);
                    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
                    const float nmx = -mx * SL;
                    float sum = 0.f;
#pragma unroll
                    for (int r = 0; r < 16; ++r) { sT[r] = __builtin_amdgcn_exp2f(fmaf(sT[r], SL, nmx)); sum += sT[r]; }
                    sum += __shfl_xor(sum, 32, 64);
                    const float inv = 1.0f / sum;
                    float D = 0.f;
#pragma unroll
                    for (int r = 0; r < 16; ++r) { sT[r] *= inv; D += sT[r] * dpT[r]; }
                    D += __shfl_xor(D, 32, 64);
                    if (role == 0) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) dpT[r] = sT[r] * (dpT[r] - D);                                  // dS^T[key][query]
                        if (h == 0) dbacc[0] += dpT; else if (h == 1) dbacc[1] += dpT;
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int e = l31 * 33 + crow(r, lh);
                            o1 = MFMA(Ki[e], dpT[r], o1);          // dq'^T[d][query] = sum_key K'[d][key] dS^T[key][query]
                            o2 = MFMA(Vi[e], sT[r], o2);           // O^T[d][query]  = sum_key V[d][key] P^T[key][query]
                        }
                        unrot(o1);
                    } else {
                        if (lh == 0) { st_m[l31] = nmx; st_l[l31] = inv; st_d[l31] = D; }
                        f32x16 sN, dpN;                // [query rows][key lanes]
#pragma unroll
                        for (int r = 0; r < 16; ++r) { sN[r] = bs[crow(r, lh) * 33 + l31]; dpN[r] = 0.f; }
#pragma unroll
                        for (int s2 = 0; s2 < 16; ++s2) {
                            const int e = (2 * s2 + lh) * 33 + l31;
                            sN = MFMA(Qi[e], Ki[e], sN);
                            dpN = MFMA(Gi[e], Vi[e], dpN);
                        }
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int q = crow(r, lh);
                            const float p = __builtin_amdgcn_exp2f(fmaf(sN[r], SL, st_m[q])) * st_l[q];
                            sN[r] = p;
                            dpN[r] = p * (dpN[r] - st_d[q]);                                                         // dS[query][key]
                        }
                        if (h == 2) dbacc[0] += dpN; else if (h == 3) dbacc[1] += dpN;
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int e = l31 * 33 + crow(r, lh);
                            o1 = MFMA(Qi[e], dpN[r], o1);          // dk'^T[d][key] = sum_q Q'[d][q] dS[q][key]
                            o2 = MFMA(Gi[e], sN[r], o2);           // dv^T[d][key]  = sum_q dO^T[d][q] P[q][key]
                        }
                        unrot(o1);
                    }
                }
                __syncthreads();                       // every wave has read the q, k, v, dO images
                {
                    float* ia = role ? Ki : Qi, * ib = role ? Vi : Gi;     // dq | dk,  O | dv
#pragma unroll
                    for (int r = 0; r < 16; ++r) { ia[crow(r, lh) * 33 + l31] = o1[r]; ib[crow(r, lh) * 33 + l31] = o2[r]; }
                }
                __syncthreads();
                // ---- P3. dxn of (pixel px, channels 32 role ..): A = W[c][d] in 16-float runs along d (k-step ks: d = ks + 16 lh)
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const nfloat4* w4 = reinterpret_cast<const nfloat4*>(a.wqkv + (role * 32 + l31) * 384 + i * 128 + h * 32 + 16 * lh);
                    const float* bi = img + (i * 4 + px) * IMG + (16 * lh) * 33 + l31;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const nfloat4 t = w4[j];
                        dxacc = MFMA(t.x, bi[(4 * j) * 33], dxacc);
                        dxacc = MFMA(t.y, bi[(4 * j + 1) * 33], dxacc);
                        dxacc = MFMA(t.z, bi[(4 * j + 2) * 33], dxacc);
                        dxacc = MFMA(t.w, bi[(4 * j + 3) * 33], dxacc);
                    }
                }
                // the weight-gradient tile of this wave: K = 128 tokens
                {
                    const int mat = wave >> 1, hf = wave & 1;
                    const float* A = mat < 3 ? xs + (32 * hf + l31) * RP + lh : img + 12 * IMG + l31 * 33 + lh;
                    const float* B = mat < 3 ? img + (mat * 4) * IMG + l31 * 33 + lh : dys + (32 * hf + l31) * RP + lh;
                    const int sa = mat < 3 ? 33 : IMG, sb = mat < 3 ? IMG : 33;
                    f32x16 t;
#pragma unroll
                    for (int r = 0; r < 16; ++r) t[r] = 0.f;
#pragma unroll 1
                    for (int p = 0; p < 4; ++p)
#pragma unroll
                        for (int fs = 0; fs < 16; ++fs) t = MFMA(A[p * sa + 2 * fs], B[p * sb + 2 * fs], t);
                    switch (h) {
                        case 0: dwacc[0] += t; break;
                        case 1: dwacc[1] += t; break;
                        case 2: dwacc[2] += t; break;
                        default: dwacc[3] += t; break;
                    }
                }
            }
            // ---- B. dxn through LDS; LayerNorm backward, the residual, dg
            __syncthreads();                           // every wave is done with xn
#pragma unroll
            for (int r = 0; r < 16; ++r) xs[(role * 32 + crow(r, lh)) * RP + px * 33 + l31] = dxacc[r];
            __syncthreads();
            {
                const float mean = lnst[tok], rstd = lnst[128 + tok];
                float xh[16], gd[16];
                float s1 = 0.f, s2 = 0.f;
#pragma unroll
                for (int c = 0; c < 16; ++c) {
                    xh[c] = (ldu(uni(xt + (int64_t)c * a.sc), toff) - mean) * rstd;
                    const float dn = xs[(qt * 16 + c) * RP + pw * 33 + f];
                    gd[c] = dn * a.g[qt * 16 + c];
                    dgacc[c] += dn * xh[c];
                    s1 += gd[c];
                    s2 += gd[c] * xh[c];
                }
                red[qt * 128 + tok] = s1;
                red[512 + qt * 128 + tok] = s2;
                __syncthreads();
                const float m1 = ((red[tok] + red[128 + tok]) + (red[256 + tok] + red[384 + tok])) * (1.0f / C);
                const float m2 = ((red[512 + tok] + red[640 + tok]) + (red[768 + tok] + red[896 + tok])) * (1.0f / C);
#pragma unroll
                for (int c = 0; c < 16; ++c)
                    stu(uni(dxt + (int64_t)c * a.sc), toff, dys[(qt * 16 + c) * RP + pw * 33 + f] + rstd * (gd[c] - m1 - xh[c] * m2));
            }
            __syncthreads();                           // xs, dys, red and lnst are free for the next pass
        }
    }

    // ---- this workgroup's partial table: every element written, whatever the walk gave this workgroup
    float* const part = a.part + (int64_t)blockIdx.x * PART;
    {
        const int mat = wave >> 1, hf = wave & 1;
#pragma unroll
        for (int h = 0; h < 4; ++h)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                if (mat < 3) part[P_WQKV + (32 * hf + crow(r, lh)) * 384 + mat * 128 + h * 32 + l31] = dwacc[h][r];
                else part[P_WO + (h * 32 + crow(r, lh)) * 64 + 32 * hf + l31] = dwacc[h][r];
            }
    }
    // role 0: dbacc[h][r] = dS^T[key = crow][query = l31] of heads 0, 1; role 1: dS[query = crow][key = l31] of heads 2, 3 -> [pixel][head][query][key]
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            if (role == 0) img[(px * 4 + h) * 1024 + l31 * 32 + crow(r, lh)] = dbacc[h][r];
            else img[(px * 4 + 2 + h) * 1024 + crow(r, lh) * 32 + l31] = dbacc[h][r];
        }
#pragma unroll
    for (int c = 0; c < 16; ++c) xs[(qt * 16 + c) * 129 + tok] = dgacc[c];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int e = tid + i * NT;
        part[P_BIAS + e] = (img[e] + img[4096 + e]) + (img[8192 + e] + img[12288 + e]);
    }
    if (tid < C) {
        float s = 0.f;
        for (int t = 0; t < 128; ++t) s += xs[tid * 129 + t];
        part[P_G + tid] = s;
    }
}

// out[i] = sum_k part[k][i], k in a fixed order (the scheme of sum_rows_kernel, sdc_attn_bwd.hip): 16 groups x 64 elements, group g
// adds the tables k = g (mod 16), group 0 adds the sixteen sums in order.  The table's four segments go to their own arrays.
constexpr int SR_G = 16;
__global__ __launch_bounds__(64 * SR_G) void tab_sum_kernel(const float* __restrict__ part, float* __restrict__ dwqkv, float* __restrict__ dwo,
                                                           float* __restrict__ dbias, float* __restrict__ dg, int nsplit) {
    const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int i = blockIdx.x * 64 + lane;              // PART is a multiple of 64
    float s = 0.0f;
    int k = g;
    for (; k + 3 * SR_G < nsplit; k += 4 * SR_G) {
        const float v0 = part[(int64_t)k * PART + i], v1 = part[(int64_t)(k + SR_G) * PART + i];
        const float v2 = part[(int64_t)(k + 2 * SR_G) * PART + i], v3 = part[(int64_t)(k + 3 * SR_G) * PART + i];
        s += v0; s += v1; s += v2; s += v3;
    }
    for (; k < nsplit; k += SR_G) s += part[(int64_t)k * PART + i];
    __shared__ float sh[SR_G][64];
    sh[g][lane] = s;
    __syncthreads();
    if (g == 0) {
        float t = sh[0][lane];
        for (int q = 1; q < SR_G; ++q) t += sh[q][lane];
        if (i < P_WO) dwqkv[i] = t;
        else if (i < P_BIAS) dwo[i - P_WO] = t;
        else if (i < P_G) { if (dbias) dbias[i - P_BIAS] = t; }
        else dg[i - P_G] = t;
    }
}

}  // namespace

extern "C" size_t sdc_tattn_block_bwd_bytes(int outer, int inner) {
    if (outer <= 0 || inner <= 0) return 0;
    int64_t n = (int64_t)outer * inner / NS;           // pixel groups
    n = n < 1 ? 1 : (n > MAXWG ? MAXWG : n);
    return (size_t)n * PART * sizeof(float);
}

extern "C" int sdc_tattn_block_bwd(const float* x, const float* g_pre, const float* wqkv, const float* wo, const float* rot,
                                   const float* bias, const float* dy, float* dx, float* dg, float* dwqkv, float* dwo, float* dbias,
                                   void* work, int outer, int inner, int Cc, int ntok, int64_t so, int64_t sc, int64_t st, float eps,
                                   void* stream) {
    SDC_REQUIRE(x && g_pre && wqkv && wo && dy && dx && dg && dwqkv && dwo && work, SDC_ENULL, "sdc_tattn_block_bwd: null pointer");
    SDC_REQUIRE(!bias || dbias, SDC_ENULL, "sdc_tattn_block_bwd: bias given without dbias");
    TaArgs a;
    if (const int rc = ta_check_args("sdc_tattn_block_bwd", x, g_pre, rot, bias, dx, outer, inner, Cc, ntok, so, sc, st, eps, a)) return rc;
    a.wqkv = wqkv; a.wo = wo; a.dy = dy; a.part = static_cast<float*>(work);
    SDC_REQUIRE(reinterpret_cast<uintptr_t>(wqkv) % 16 == 0 && reinterpret_cast<uintptr_t>(wo) % 16 == 0 &&
                (!rot || reinterpret_cast<uintptr_t>(rot) % 8 == 0), SDC_EINVAL,
                "sdc_tattn_block_bwd: wqkv / wo must be 16-byte aligned and rot 8-byte aligned");
    static_assert(PART % 64 == 0, "tab_sum_kernel walks whole groups of 64");
    static_assert(LDS_FLOATS * sizeof(float) <= 160 * 1024, "LDS budget");
    static std::atomic<uint64_t> attr{0};
    SDC_LDS_OPTIN(attr, ta_block_bwd_kernel, 160 * 1024, "sdc_tattn_block_bwd");
    unsigned grid = 0;
    if (const int rc = sdc::ta_grid("sdc_tattn_block_bwd", a.nblk, &grid)) return rc;
    if (grid > (unsigned)MAXWG) grid = MAXWG;          // the workspace's bound (sdc_tattn_block_bwd_bytes needs no device query)
    hipStream_t s = sdc::as_stream(stream);
    hipLaunchKernelGGL(ta_block_bwd_kernel, dim3(grid), dim3(NT), LDS_FLOATS * sizeof(float), s, a);
    hipLaunchKernelGGL(tab_sum_kernel, dim3(PART / 64), dim3(64 * SR_G), 0, s, (const float*)a.part, dwqkv, dwo, bias ? dbias : nullptr, dg,
                       (int)grid);
    return sdc::check_launch("sdc_tattn_block_bwd");
}
