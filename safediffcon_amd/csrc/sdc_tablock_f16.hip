// net.attn_f16 (opt-in, samplers only): the fused temporal-attention block of sdc_tablock.hip with fp16 operands on the gfx950
// 16-bit matrix pipe, v_mfma_f32_32x32x16_f16 -- fp16 operands rounded to nearest even, fp32 accumulation:
//
//   y = x + Wo . softmax( rot(s Wq xn) rot(Wk xn)^T + relpos ) (Wv xn),   xn = channel LayerNorm(x) * gamma
//
// Same computation, tensor strides, tables and workgroup walk as ta_block_kernel (one persistent workgroup per CU, 8 adjacent
// pixels per tile, one wave per pixel, all 32 frames, all 4 heads); the arguments, the tile geometry, the wave-uniform-base accessors,
// the walk and the entry's common checks are sdc_tablock_tile.h's, the fragment type and frag() sdc_f16frag.h's.  What differs:
//   - per head and wave 12 + 2 + 2 + 4 = 20 MFMAs of K = 16 instead of 160 of K = 2;
//   - xn is kept in LDS as fp16, [pixel][frame][channel]: the 8 channels of a lane's K fragment are one 16-byte read, and the four
//     fragments of a wave's pixel are read once per tile and serve all four heads (as B operand of q and k, as A operand of V^T);
//   - the weights of all four heads sit in LDS as fp16 fragments (64 KB, sdc_pack_tattn_f16; copied once per workgroup): no weight
//     fetch and no barrier inside the head loop;
//   - the register chain of the fp32 kernel carries over: eight consecutive accumulator registers of a lane, converted to fp16,
//     are one K fragment of the next product.  Step s, half-wave lh, element j stands for accumulator row crow(8 s + j, lh) -- a
//     fixed permutation of the contraction index that both operands of a product share (the Wo fragments are packed in it);
//   - y leaves through LDS in two halves of 32 channels, in the space xn occupied.
// fp32: LayerNorm, rotary, bias, softmax (maximum, exponent, row sum, division), every accumulator, the residual add, the store.
// Rounded once to fp16 (RNE) as operands: xn, the weights (at pack time), q and k after the rotary (unscaled: the scale rides on the
// softmax exponent), v, the un-normalised probabilities exp(s - max) in (0, 1], O after the division by the fp32 row sum.
// No atomics, fixed accumulation order, a sample's arithmetic does not see the batch.
#define TA_WEIGHT_ARGS const _Float16* wpk;
#include "sdc_tablock_tile.h"
#include "sdc_f16frag.h"

namespace {

constexpr int CP = 72;                   // pitch (halves) of one token of xn: 64 channels + 16 bytes
constexpr int WQKV_H = 4 * 3 * 4 * 64 * 8;   // halves of the q / k / v fragments
constexpr int WPK_H = WQKV_H + 4 * 2 * 2 * 64 * 8;

__global__ __launch_bounds__(NT) void ta_block_f16_kernel(const TaArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_f16[];
    _Float16* const wsh = reinterpret_cast<_Float16*>(smem_f16);       // [WPK_H] the packed weights of all four heads
    _Float16* const xh = wsh + WPK_H;                                   // [8 pixels][32 frames][CP]  xn
    float* const ys = reinterpret_cast<float*>(xh);                     // [32][XP]  later half of the y image (33792 <= 36864 bytes)
    float* const biasT = reinterpret_cast<float*>(xh + NS * 32 * CP);   // [4][32][33]  [head][key][query]
    float* const rotcs = biasT + 4 * 32 * 33;                           // [16 m][32 frames][2]: (cos, sin)
    float* const red = rotcs + 2 * 32 * 16;                             // [2][2][256] LayerNorm partials

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lh = lane >> 5;
    const TaWalk wk = ta_walk(a.nblk);
    const int per = wk.per, first = wk.first, stride = wk.stride;

    const int tok = tid & 255, half = tid >> 8, pw = tok & 7, f = tok >> 3;
    const uint32_t toff = (uint32_t)(((int64_t)f * a.st + pw) * 4);     // this thread's token (byte offset inside one channel of one
                                                                        // outer index: < 2^32, host check)

    float v[32];                                   // raw x of the tile about to be normalised (this thread's token, channels half*32 ..)
    if (first < per) {
        const float* xt = a.x + ta_tile_ptr(a, wk, first) + (int64_t)(half * 32) * a.sc;
#pragma unroll
        for (int c = 0; c < 32; ++c) v[c] = ldu(uni(xt + (int64_t)c * a.sc), toff);
    }
    // ---- once per workgroup: the weights, the transposed bias table, the rotary table (the first tile's barriers publish them)
    {
        const u32x4* src = reinterpret_cast<const u32x4*>(a.wpk);
        u32x4* dst = reinterpret_cast<u32x4*>(wsh);
#pragma unroll
        for (int i = 0; i < WPK_H / 8 / NT; ++i) dst[tid + i * NT] = src[tid + i * NT];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int e = tid + i * NT, h = e >> 10, q = (e >> 5) & 31, kk = e & 31;
            // bias / scale: the q * scale of the reference is applied to the finished scores, inside the softmax's exponent
            biasT[(h * 32 + kk) * 33 + q] = (a.bias ? a.bias[e] : 0.0f) * 5.65685424949238f;
        }
        const float2 rr = a.rot ? *reinterpret_cast<const float2*>(a.rot + tid * 2) : make_float2(1.0f, 0.0f);
        *reinterpret_cast<float2*>(rotcs + (((tid & 15) * 32) + (tid >> 4)) * 2) = rr;      // tid = frame * 16 + m
    }
    const int hw = wave;                           // this wave's pixel of the tile

    for (int li = first; li < per; li += stride) {
        const int64_t tp = ta_tile_ptr(a, wk, li);
        const bool more = li + stride < per;
        // ---- 1. LayerNorm over the 64 channels of a token (pixel pw, frame f): two threads per token, 32 channels each; fp32, then
        //         one rounding to fp16
        {
            float sm = 0.f;
#pragma unroll
            for (int c = 0; c < 32; ++c) sm += v[c];
            red[half * 256 + tok] = sm;
            __syncthreads();
            const float mean = (red[tok] + red[256 + tok]) * (1.0f / C);
            float q = 0.f;
#pragma unroll
            for (int c = 0; c < 32; ++c) { v[c] -= mean; q += v[c] * v[c]; }
            red[512 + half * 256 + tok] = q;
            __syncthreads();
            const float rstd = rsqrtf((red[512 + tok] + red[768 + tok]) * (1.0f / C) + a.eps);
            half8* xo = reinterpret_cast<half8*>(xh + (pw * 32 + f) * CP + half * 32);
#pragma unroll
            for (int c8 = 0; c8 < 4; ++c8) {
                half8 h;
#pragma unroll
                for (int j = 0; j < 8; ++j) h[j] = (_Float16)(v[c8 * 8 + j] * rstd * a.g[half * 32 + c8 * 8 + j]);
                xo[c8] = h;
            }
        }
        __syncthreads();                               // xn (and, on the first tile, the weights and tables) are in LDS
        // ---- 2. heads; this wave owns pixel `wave`.  xn fragments: lane (frame l31, half-wave lh), step s holds channels
        //         16 s + 8 lh + j -- B operand of q and k, A operand of V^T, for every head
        half8 xf[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) xf[s] = *reinterpret_cast<const half8*>(xh + (hw * 32 + l31) * CP + 16 * s + 8 * lh);
        f32x16 yacc[2];                                // row tiles of y (32 channels each)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) yacc[i][r] = 0.f;
#pragma unroll 1
        for (int head = 0; head < 4; ++head) {
            const half8* wf = reinterpret_cast<const half8*>(wsh) + head * (3 * 4 * 64) + lane;
            // q, k [32 d][32 f]: A = W^T fragment, B = xn; V^T [32 f][32 d]: operands swapped, so that its accumulator registers are
            // the A fragments of O^T = V P as they stand
            f32x16 q, k, vt;
#pragma unroll
            for (int r = 0; r < 16; ++r) { q[r] = 0.f; k[r] = 0.f; vt[r] = 0.f; }
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                q = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[(0 * 4 + s) * 64], xf[s], q, 0, 0, 0);
                k = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[(1 * 4 + s) * 64], xf[s], k, 0, 0, 0);
                vt = __builtin_amdgcn_mfma_f32_32x32x16_f16(xf[s], wf[(2 * 4 + s) * 64], vt, 0, 0, 0);
            }
            // rotary on (d = 2m, 2m+1) pairs = registers (r, r+1) for even r; frame = l31 (fp32, on the accumulators)
#pragma unroll
            for (int r = 0; r < 16; r += 2) {
                const int m = crow(r, lh) >> 1;
                const float2 cs = *reinterpret_cast<const float2*>(rotcs + (m * 32 + l31) * 2);
                const float q0 = q[r], q1 = q[r + 1], k0 = k[r], k1 = k[r + 1];
                q[r] = q0 * cs.x - q1 * cs.y; q[r + 1] = q1 * cs.x + q0 * cs.y;
                k[r] = k0 * cs.x - k1 * cs.y; k[r + 1] = k1 * cs.x + k0 * cs.y;
            }
            // S^T[key][query] / scale = bias / scale + sum_d K[d][key] Q[d][query]: A = K registers, B = Q registers
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = biasT[(head * 32 + crow(r, lh)) * 33 + l31];
#pragma unroll
            for (int s = 0; s < 2; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(frag(k, 8 * s), frag(q, 8 * s), acc, 0, 0, 0);
            float mx = -INFINITY;
#pragma unroll
            for (int r = 0; r < 16; ++r) mx = fmaxf(mx, acc[r]);
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            // p = exp(scale (acc - mx)) = exp2(acc * (scale log2 e) - mx * (scale log2 e)); the row sum is of the fp32 values
            const float SL = 0.17677669529663687f * 1.4426950408889634f;
            const float nmx = -mx * SL;
            float sum = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) { acc[r] = __builtin_amdgcn_exp2f(fmaf(acc[r], SL, nmx)); sum += acc[r]; }
            sum += __shfl_xor(sum, 32, 64);
            const float inv = 1.0f / sum;
            // O^T[d][query] = sum_key V^T[key][d] P[key][query]: A = V^T registers, B = un-normalised P registers; the division by
            // the row sum (per query = per lane) follows on the fp32 accumulator
            f32x16 oacc;
#pragma unroll
            for (int r = 0; r < 16; ++r) oacc[r] = 0.f;
#pragma unroll
            for (int s = 0; s < 2; ++s) oacc = __builtin_amdgcn_mfma_f32_32x32x16_f16(frag(vt, 8 * s), frag(acc, 8 * s), oacc, 0, 0, 0);
            // y[co][f] += sum_d Wo[co][head*32 + d] O^T[d][f]:  A = Wo fragments (d in accumulator-row order), B = O^T registers
            const half8* wof = reinterpret_cast<const half8*>(wsh + WQKV_H) + head * (2 * 2 * 64) + lane;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const half8 of = frag(oacc, 8 * s, inv);
                yacc[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wof[(0 * 2 + s) * 64], of, yacc[0], 0, 0, 0);
                yacc[1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wof[(1 * 2 + s) * 64], of, yacc[1], 0, 0, 0);
            }
        }
        // ---- 3. the next tile's x is requested, then y leaves in two halves of 32 channels through the LDS space of xn: thread
        //         (token, half) adds the residual (L2-warm second read of x) to channels i*32 + half*16 .. + 16 and stores them
        {   // (unconditional: the last tile re-reads itself)
            const float* xt = a.x + ta_tile_ptr(a, wk, more ? li + stride : li) + (int64_t)(half * 32) * a.sc;
#pragma unroll
            for (int c = 0; c < 32; ++c) v[c] = ldu(uni(xt + (int64_t)c * a.sc), toff);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            float xr[16];
            const int64_t ch0 = (int64_t)(i * 32 + half * 16) * a.sc;
            const float* xt = a.x + tp + ch0;
#pragma unroll
            for (int c = 0; c < 16; ++c) xr[c] = ldu(uni(xt + (int64_t)c * a.sc), toff);
            __syncthreads();                           // every wave is done with xn / with the previous half of the y image
#pragma unroll
            for (int r = 0; r < 16; ++r) ys[crow(r, lh) * XP + hw * 33 + l31] = yacc[i][r];
            __syncthreads();
            const float* yt = a.y + tp + ch0;
#pragma unroll
            for (int c = 0; c < 16; ++c) stu(uni(yt + (int64_t)c * a.sc), toff, ys[(half * 16 + c) * XP + pw * 33 + f] + xr[c]);
        }
        __syncthreads();                               // the y image is consumed: the space is free for the next tile's xn
    }
}

// dst[e], e < WPK_H: the layout of include/sdc.h from the nn.Linear weights to_qkv (384, 64) and to_out (64, 128)
__global__ __launch_bounds__(256) void pack_tattn_f16_kernel(const float* __restrict__ wqkv, const float* __restrict__ wo,
                                                             _Float16* __restrict__ dst) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= WPK_H) return;
    const int j = e & 7, lane = (e >> 3) & 63, l31 = lane & 31, lh = lane >> 5;
    if (e < WQKV_H) {
        const int s = (e >> 9) & 3, hm = e >> 11, mat = hm % 3, head = hm / 3;
        dst[e] = (_Float16)wqkv[(mat * 128 + head * 32 + l31) * C + 16 * s + 8 * lh + j];
    } else {
        const int e2 = e - WQKV_H, s = (e2 >> 9) & 1, i = (e2 >> 10) & 1, head = e2 >> 11;
        dst[e] = (_Float16)wo[(32 * i + l31) * 128 + head * 32 + crow(8 * s + j, lh)];
    }
}

}  // namespace

extern "C" size_t sdc_pack_tattn_f16_bytes(void) { return (size_t)WPK_H * sizeof(_Float16); }

extern "C" int sdc_pack_tattn_f16(const float* wqkv, const float* wo, void* dst, void* stream) {
    SDC_REQUIRE(wqkv && wo && dst, SDC_ENULL, "sdc_pack_tattn_f16: null pointer");
    SDC_REQUIRE(reinterpret_cast<uintptr_t>(dst) % 16 == 0, SDC_EALIGN, "sdc_pack_tattn_f16: dst must be 16-byte aligned");
    hipLaunchKernelGGL(pack_tattn_f16_kernel, dim3(WPK_H / 256), dim3(256), 0, sdc::as_stream(stream), wqkv, wo,
                       reinterpret_cast<_Float16*>(dst));
    return sdc::check_launch("sdc_pack_tattn_f16");
}

extern "C" int sdc_tattn_block_f16(const float* x, const float* g_pre, const void* wpk, const float* rot, const float* bias, float* y,
                                   int outer, int inner, int Cc, int ntok, int64_t so, int64_t sc, int64_t st, float eps, void* stream) {
    SDC_REQUIRE(wpk, SDC_ENULL, "sdc_tattn_block_f16: null pointer");
    TaArgs a;
    if (const int rc = ta_check_args("sdc_tattn_block_f16", x, g_pre, rot, bias, y, outer, inner, Cc, ntok, so, sc, st, eps, a)) return rc;
    a.wpk = reinterpret_cast<const _Float16*>(wpk);
    // the prologue copies the weight buffer with 16-byte and reads the rotary table with 8-byte vector loads
    SDC_REQUIRE(reinterpret_cast<uintptr_t>(wpk) % 16 == 0, SDC_EALIGN, "sdc_tattn_block_f16: the weight buffer must be 16-byte aligned");
    SDC_REQUIRE(!rot || reinterpret_cast<uintptr_t>(rot) % 8 == 0, SDC_EINVAL, "sdc_tattn_block_f16: rot must be 8-byte aligned");
    const size_t ldsb = sizeof(_Float16) * (size_t)(WPK_H + NS * 32 * CP) + sizeof(float) * (size_t)(4 * 32 * 33 + 2 * 32 * 16 + 1024);
    static std::atomic<uint64_t> attr{0};
    SDC_LDS_OPTIN(attr, ta_block_f16_kernel, 160 * 1024, "sdc_tattn_block_f16");
    unsigned grid = 0;
    if (const int rc = sdc::ta_grid("sdc_tattn_block_f16", a.nblk, &grid)) return rc;
    hipLaunchKernelGGL(ta_block_f16_kernel, dim3(grid), dim3(NT), ldsb, sdc::as_stream(stream), a);
    return sdc::check_launch("sdc_tattn_block_f16");
}
