// net.attn_split (samplers only, precision 4 and 5): the fused temporal-attention block of sdc_tablock.hip with the products that have
// a weight operand -- the q / k / v projections and the out-projection, 128 of its 160 fp32 MFMAs per head and wave -- formed on the
// gfx950 bf16 matrix pipe, v_mfma_f32_32x32x16_bf16, from EXACT three-way bf16 operand splits (the arithmetic of conv_stem_x3_kernel):
//
//   y = x + Wo . softmax( rot(s Wq xn) rot(Wk xn)^T + relpos ) (Wv xn),   xn = channel LayerNorm(x) * gamma
//
//   a = a1 + a2 + a3 (RNE bf16 pieces, exact fp32 residuals);  a b ~ a3 b1 + a2 b2 + a1 b3 + a2 b1 + a1 b2 + a1 b1, fp32 accumulation
//
// An fp32-grade result in another rounding order, not a reduced precision.  Walk, tables and exit are ta_block_f16_kernel's (one
// persistent workgroup per CU, 8 adjacent pixels per tile, one wave per pixel, all 32 frames, all 4 heads, XCD-ordered walk, the next
// tile's x requested behind the head loop, y out through LDS in two halves); the arguments, the tile geometry, the wave-uniform-base
// accessors, the walk and the entry's common checks are sdc_tablock_tile.h's, the split and the term order sdc_split3.h's.  What is split:
//   - the weights, once, at pack time (sdc_pack_tattn_x3: three planes in sdc_pack_tattn_f16's fragment order, head by head);
//   - xn, once per value and tile: the LayerNorm leaves an fp32 image [pixel][frame][channel] in LDS, every wave reads the 32 values of
//     its lanes' fragments (frame l31, channels 16 s + 8 lh + j) and keeps their three pieces in registers (3 x 16 VGPRs) for all four
//     heads and both operand roles (B of q and k, A of V^T);
//   - O^T after the softmax normalisation: eight consecutive accumulator registers are one K fragment, in three pieces.
// A product's five small terms are issued first, smallest kind first, each over all its K steps, then the main term: one accumulator
// per output, the main sum rounded K / 16 times.  q, k and V^T are three independent chains.
// fp32, with ta_block_kernel's instructions and order: LayerNorm, rotary on the accumulators, bias as the start value of the scores, the
// 32x32x2_f32 score chain from the K and Q registers, softmax, the 32x32x2_f32 O chain from the V^T and P registers (the accumulators
// of the bf16 MFMA have the fp32 one's register layout), every accumulator, the residual add.
// LDS (141 KB): weight buffer A (one head, 3 pieces, 48 KB) | region B (68 KB: the fp32 xn image until every wave holds its fragments,
// then the second weight buffer -- heads 1 and 3 --, then the y halves) | tables.  Head h + 1's weights travel through registers while
// head h is on the matrix cores; head 3 brings head 0 of the next tile.  One barrier per head.
// No atomics, fixed accumulation order, a sample's arithmetic does not see the batch.  A non-finite x gives NaN (inf - inf in the
// residual of the split) where the fp32 kernel may give an infinity.
// Two kernels share the tile walk below (ta_x3_tiles): ta_block_x3_kernel, and ta_block_x3s_kernel, in which waves 4 - 7 run half a
// head behind waves 0 - 3 and y leaves in one pass (impl 1 of sdc_tattn_block_x3_sel; +12 KB of LDS, 152.75 KB; the same bits).  x and y
// move through buffer instructions with a scalar channel offset (ldb / stb below).
#define TA_WEIGHT_ARGS const __bf16* wpk;
#include "sdc_tablock_tile.h"
#include "sdc_split3.h"

namespace {

constexpr int XF = 68;                   // pitch (floats) of one token of the xn image: 64 channels + 16 bytes
constexpr int XPP = 32 * XF + 8;         // pitch (floats) of one pixel of the xn image (+ 32 bytes: the LayerNorm's stores spread over the banks)
constexpr int WQKV_E = 3 * 4 * 64 * 8;   // bf16 elements of one head's q / k / v fragments (one piece)
constexpr int HEAD_E = WQKV_E + 2 * 2 * 64 * 8;      // ... of one head (one piece): 8192
constexpr int WPK_E = 4 * 3 * HEAD_E;    // the whole buffer: [head][piece][HEAD_E]
constexpr int WBUF_B = 3 * HEAD_E * 2;   // bytes of one head's weights: 49152
constexpr int REGB_B = NS * XPP * 4;     // bytes of region B: 69888
static_assert(WBUF_B <= REGB_B && 64 * XP * 4 <= REGB_B, "region B holds a head's weights and the y image");
static_assert(WBUF_B % (16 * NT) == 0, "whole 16-byte words per thread");

// rotary step: x = (x0, x1), cs = (cos, sin) -> (x0 cos - x1 sin, x1 cos + x0 sin) with the roundings of ta_block_kernel's packed pair
// (a rounded product with the cosine, then one fused multiply-add with the sine), left to the compiler's instruction selection
__device__ __forceinline__ ta2 ta_rot(ta2 x, ta2 cs) {
#pragma clang fp contract(off)
    const float t0 = x.x * cs.x, t1 = x.y * cs.x;
    return ta2{__builtin_fmaf(-x.y, cs.y, t0), __builtin_fmaf(x.x, cs.y, t1)};
}

// x and y of a tile through buffer instructions: the tile's first element as a raw buffer resource (wave-uniform, four SGPRs), the
// channel as the scalar offset, the thread's token as the 32-bit vector offset -- `buffer_load_dword v, v_tok, s[rsrc], s_chan offen`,
// one scalar addition per value.  (ldu / stu of sdc_tablock_tile.h leave the compiler a 64-bit vector addition and two
// v_readfirstlane per value: 96 such accesses per thread and tile.)  Byte offsets: channel + token < 2^32 is the entry's host check.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t ta_buf(const float* p) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p), 0, 0xffffffff, 0x00020000);      // stride 0, raw, 32-bit data
}
__device__ __forceinline__ float ldb(__amdgpu_buffer_rsrc_t r, uint32_t tok_off, uint32_t chan_off) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, tok_off, chan_off, 0));
}
__device__ __forceinline__ void stb(__amdgpu_buffer_rsrc_t r, uint32_t tok_off, uint32_t chan_off, float v) {
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, v), r, tok_off, chan_off, 0);
}

// Kernel experiments of ta_block_x3_kernel (SDC_TAX3_DBG, -DSDC_KERNEL_EXPERIMENTS only; WRONG RESULTS): one part of the tile switched
// off at a time, for the phase account of DESIGN.md section 19.  The shipping library instantiates DBG = 0 alone.
constexpr int XD_LN = 1;       // no LayerNorm phase (the x loads stay)
constexpr int XD_EXIT = 2;     // no y exit (residual reads, staging through LDS, stores)
constexpr int XD_SPLIT = 4;    // no xn and O splits (the pieces are bit patterns of the values)
constexpr int XD_WFETCH = 8;   // no weight fetch and park
constexpr int XD_FRAG = 16;    // no fragment reads (the weight operands are the xn registers)
constexpr int XD_BAR = 32;     // no per-head barrier
constexpr int XD_VALU = 64;    // no rotary, bias and softmax
[[maybe_unused]] constexpr int XD_MFMA_ONLY = 127;
constexpr int XD_STORE = 128;  // the y exit without its global stores
constexpr int XD_RES = 256;    // the y exit without the residual reads
constexpr int XD_XNEXT = 512;  // no reads of the next tile's x (the first tile's registers again)

template <int DBG>
__device__ __forceinline__ void ta_split3x8(const float* v, bf16x8& h, bf16x8& m, bf16x8& l) {
    if constexpr (DBG & XD_SPLIT) {
        const nfloat4 lo = {v[0], v[1], v[2], v[3]}, hi = {v[4], v[5], v[6], v[7]};
        h = __builtin_bit_cast(bf16x8, lo); m = __builtin_bit_cast(bf16x8, hi); l = h;
    } else {
        split3x8(v, h, m, l);
    }
}

constexpr int WOS_P = 2 * 2 * 64;        // bf16x8 words of one piece of a head's out-projection fragments (4 KB)
constexpr int WOS_B = 3 * WOS_P * 16;    // bytes of the skewed kernel's third out-projection slot: 12288
constexpr int TAB_B = 4 * (4 * 32 * 33 + 2 * 32 * 16 + 1024);     // bytes of the tables: bias, rotary, LayerNorm partials

// The tile walk of both kernels.  SKEW = false is ta_block_x3_kernel: all eight waves run a head's front (q / k / v projections, weight
// park, rotary) and its tail (score chain, softmax, O chain, O split, out-projection) between the same two barriers.  SKEW = true is
// ta_block_x3s_kernel: waves 4 - 7, the second wave of every SIMD, run half a head behind -- tail(h - 1) then front(h) where waves 0 - 3
// run front(h) then tail(h) --, so that on a SIMD one wave's VALU phases face the other's MFMA phases and four waves read weight
// fragments at a time; after head 3 they drain (tail(3)) before the exit.  Same tile, LDS images, products, term order and expressions:
// a wave's arithmetic on its pixel is the same instruction sequence either way, and the results agree bit for bit.
//
// What the lag needs: Wo of head h - 1 is read (by the lagging waves) in the interval in which head h + 1 is parked, so the
// out-projection fragments have three homes -- in place in buffer A (heads 0 and 3), in place in region B (head 1) and a third slot of
// 12 KB behind the tables (head 2) -- and the q / k / v fragments keep today's two.  Head 3 brings the q / k / v fragments of the next
// tile's head 0; that head's Wo belongs in buffer A, where Wo of head 3 is read until the drain ends, so its three words per thread (all
// of them live in waves 4 - 7) are fetched and parked in the exit, behind the barrier that ends the drain.  Only __syncthreads(), which
// every thread reaches the same number of times: the branches on the wave's half are inside the intervals.
template <bool SKEW, int EXIT, int DBG>
__device__ __forceinline__ void ta_x3_tiles(const TaArgs& a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_x3[];
    unsigned char* const wA = smem_x3;                                  // [3 pieces][HEAD_E] bf16: heads 0 and 2
    unsigned char* const rB = smem_x3 + WBUF_B;                         // region B: xn image | heads 1 and 3 | y half
    float* const xim = reinterpret_cast<float*>(rB);                    // [8 pixels][32 frames][XF] fp32 xn (pixel pitch XPP)
    float* const ys = reinterpret_cast<float*>(rB);                     // [32][XP] half of the y image
    float* const biasT = reinterpret_cast<float*>(rB + REGB_B);         // [4][32][33]  [head][key][query]
    float* const rotcs = biasT + 4 * 32 * 33;                           // [16 m][32 frames][2]: (cos, sin)
    float* const red = rotcs + 2 * 32 * 16;                             // [2][2][256] LayerNorm partials
    unsigned char* const wE = rB + REGB_B + TAB_B;                      // (SKEW) [3 pieces][WOS_P] bf16x8: Wo of head 2

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lh = lane >> 5;
    const bool lag = SKEW && __builtin_amdgcn_readfirstlane(tid) >= NT / 2;     // wave-uniform: waves 4 - 7
    const TaWalk wk = ta_walk(a.nblk);
    const int per = wk.per, first = wk.first, stride = wk.stride;

    const int tok = tid & 255, half = tid >> 8, pw = tok & 7, f = tok >> 3;
    const uint32_t toff = (uint32_t)(((int64_t)f * a.st + pw) * 4);     // this thread's token (byte offset inside one channel of one
                                                                        // outer index: < 2^32, host check)

    // one head's weights (three pieces, one contiguous run of 48 KB): six 16-byte words per thread, through registers.  Word
    // i * NT + tid lies in piece i / 2; the odd words of waves 4 - 7 are the piece's out-projection fragments, every other word q / k / v.
    u32x4 wreg[6];
    // SKEW: `wo` selects among the out-projection words of waves 4 - 7 (+1 those alone, -1 all but those, 0 every word)
    auto fetch_head = [&](int head, int wo) {
        if constexpr (DBG & XD_WFETCH) return;
        const u32x4* src = reinterpret_cast<const u32x4*>(a.wpk) + head * (WBUF_B / 16) + tid;
#pragma unroll
        for (int i = 0; i < 6; ++i)
            if (!SKEW || wo == 0 || (((i & 1) && lag) == (wo > 0))) wreg[i] = src[i * NT];
    };
    // park in place: the image of the packed run in buffer `wb`
    auto park_head = [&](unsigned char* wb, int wo) {
        if constexpr (DBG & XD_WFETCH) return;
        u32x4* dst = reinterpret_cast<u32x4*>(wb) + tid;
#pragma unroll
        for (int i = 0; i < 6; ++i)
            if (!SKEW || wo == 0 || (((i & 1) && lag) == (wo > 0))) dst[i * NT] = wreg[i];
    };
    // SKEW: where the out-projection fragments of a head live (bf16x8 words: base, pitch of a piece)
    auto wo_base = [&](int head) -> unsigned char* { return head == 2 ? wE : ((head == 1) ? rB : wA) + WQKV_E * 2; };
    auto wo_pitch = [&](int head) -> int { return head == 2 ? WOS_P : HEAD_E / 8; };

    float v[32];                                   // raw x of the tile about to be normalised (this thread's token, channels half*32 ..)
    const uint32_t sc4 = (uint32_t)a.sc * 4u;                           // bytes between two channels
    const uint32_t hoff = (uint32_t)__builtin_amdgcn_readfirstlane(half) * 32u * sc4;      // this wave's half of the channels
    if (first < per) {
        const __amdgpu_buffer_rsrc_t xb = ta_buf(a.x + ta_tile_ptr(a, wk, first));
#pragma unroll
        for (int c = 0; c < 32; ++c) v[c] = ldb(xb, toff, hoff + (uint32_t)c * sc4);
    }
    // ---- once per workgroup: head 0's weights, the transposed bias table, the rotary table (the first tile's barriers publish them)
    {
        fetch_head(0, 0);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int e = tid + i * NT, h = e >> 10, q = (e >> 5) & 31, kk = e & 31;
            // bias / scale: the q * scale of the reference is applied to the finished scores, inside the softmax's exponent
            biasT[(h * 32 + kk) * 33 + q] = (a.bias ? a.bias[e] : 0.0f) * 5.65685424949238f;
        }
        const float2 rr = a.rot ? *reinterpret_cast<const float2*>(a.rot + tid * 2) : make_float2(1.0f, 0.0f);
        *reinterpret_cast<float2*>(rotcs + (((tid & 15) * 32) + (tid >> 4)) * 2) = rr;      // tid = frame * 16 + m
        park_head(wA, 0);
    }
    const int hw = wave;                           // this wave's pixel of the tile

    for (int li = first; li < per; li += stride) {
        const int64_t tp = ta_tile_ptr(a, wk, li);
        const bool more = li + stride < per;
        float xr1[EXIT >= 1 ? 32 : 1];                 // EXIT 1, 2: the residual, channels half*32 .. + 32 of this thread's token
        // ---- 1. LayerNorm over the 64 channels of a token (pixel pw, frame f): two threads per token, 32 channels each (fp32, the
        //         values of ta_block_kernel)
        if constexpr (DBG & XD_LN) {
#pragma unroll
            for (int c = 0; c < 32; ++c) asm volatile("" ::"v"(v[c]));      // (the loads stay)
        } else {
            float sm = 0.f;
            if constexpr (EXIT == 2) {                 // (the values the exit adds back: kept, not read a second time)
#pragma unroll
                for (int c = 0; c < 32; ++c) xr1[c] = v[c];
            }
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
            nfloat4* xo = reinterpret_cast<nfloat4*>(xim + pw * XPP + f * XF + half * 32);
#pragma unroll
            for (int c4 = 0; c4 < 8; ++c4) {
                nfloat4 o;
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = v[c4 * 4 + j] * rstd * a.g[half * 32 + c4 * 4 + j];
                xo[c4] = o;
            }
        }
        __syncthreads();                               // xn is in LDS
        // ---- 2. this wave owns pixel `wave`.  xn fragments: lane (frame l31, half-wave lh), step s holds channels 16 s + 8 lh + j --
        //         B operand of q and k, A operand of V^T, for every head; split once
        bf16x8 xf[3][4];
        {
            const float* xr = xim + hw * XPP + l31 * XF + 8 * lh;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const nfloat4 lo = *reinterpret_cast<const nfloat4*>(xr + 16 * s), hi = *reinterpret_cast<const nfloat4*>(xr + 16 * s + 4);
                const float xv[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                ta_split3x8<DBG>(xv, xf[0][s], xf[1][s], xf[2][s]);
            }
        }
        f32x16 yacc[2];                                // row tiles of y (32 channels each)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) yacc[i][r] = 0.f;
        // q, k [32 d][32 f]: A = W^T fragment, B = xn; V^T [32 f][32 d]: operands swapped, so that its accumulator registers are the A
        // fragments of O^T = V P as they stand.  (SKEW: they cross the head's barrier in waves 4 - 7.)
        f32x16 q, k, vt;
        // ---- a head's front: the projections from the fragments at `wh`, the next head's weights parked behind them, the rotary
        auto front = [&](const unsigned char* wh, int nh, bool next) {
            // the six terms of a product in sdc_split3.h's order: weight piece X3_PA[t] with xn / O piece X3_PB[t]
            // SKEW: head 0 of the next tile leaves its out-projection words to the exit
            if (next) fetch_head(nh, (SKEW && nh == 0) ? -1 : 0);
            const bf16x8* wf = reinterpret_cast<const bf16x8*>(wh) + lane;
#pragma unroll
            for (int r = 0; r < 16; ++r) { q[r] = 0.f; k[r] = 0.f; vt[r] = 0.f; }
#pragma unroll
            for (int t = 0; t < 6; ++t)
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const bf16x8* wp = wf + X3_PA[t] * (HEAD_E / 8);
                    const bf16x8 wq = (DBG & XD_FRAG) ? xf[X3_PA[t]][s] : wp[(0 * 4 + s) * 64];
                    const bf16x8 wkk = (DBG & XD_FRAG) ? xf[X3_PA[t]][s ^ 1] : wp[(1 * 4 + s) * 64];
                    const bf16x8 wv = (DBG & XD_FRAG) ? xf[X3_PA[t]][s ^ 2] : wp[(2 * 4 + s) * 64];
                    q = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wq, xf[X3_PB[t]][s], q, 0, 0, 0);
                    k = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wkk, xf[X3_PB[t]][s], k, 0, 0, 0);
                    vt = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xf[X3_PB[t]][s], wv, vt, 0, 0, 0);
                    if (s == 3) __builtin_amdgcn_sched_barrier(0);      // (a term's fragment reads stay with the term: no spills)
                }
            if (next) {
                if (!SKEW || nh == 1) {
                    park_head((nh & 1) ? rB : wA, 0);          // (head 1: every word in place in region B)
                } else {
                    park_head((nh & 1) ? rB : wA, -1);
                    if (nh != 0 && lag) {                      // Wo of heads 2 and 3: the third slot, buffer A
                        if constexpr (!(DBG & XD_WFETCH)) {
                            u32x4* dst = reinterpret_cast<u32x4*>(wo_base(nh)) + (tid - NT / 2);
                            const int pitch = wo_pitch(nh);
#pragma unroll
                            for (int p = 0; p < 3; ++p) dst[p * pitch] = wreg[2 * p + 1];
                        }
                    }
                }
            }
            if constexpr (DBG & XD_VALU) return;
            // rotary on (d = 2m, 2m+1) pairs = registers (r, r+1) for even r; frame = l31 (fp32, on the accumulators)
#pragma unroll
            for (int r = 0; r < 16; r += 2) {
                const int m = crow(r, lh) >> 1;
                const ta2 cs = *reinterpret_cast<const ta2*>(rotcs + (m * 32 + l31) * 2);
                ta2 q2 = {q[r], q[r + 1]}, k2 = {k[r], k[r + 1]};
                q2 = ta_rot(q2, cs);
                k2 = ta_rot(k2, cs);
                q[r] = q2.x; q[r + 1] = q2.y;
                k[r] = k2.x; k[r + 1] = k2.y;
            }
        };
        // ---- a head's tail: scores, softmax, O, out-projection from the fragments at `wof` (bf16x8 words, `wop` between two pieces)
        auto tail = [&](int head, const bf16x8* wof, int wop) {
            // S^T[key][query] / scale = bias / scale + sum_d K[d][key] Q[d][query]: A = K registers, B = Q registers (fp32 pipe, one
            // chain that starts from the bias)
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = (DBG & XD_VALU) ? 0.f : biasT[(head * 32 + crow(r, lh)) * 33 + l31];
#pragma unroll
            for (int r = 0; r < 16; ++r) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(k[r], q[r], acc, 0, 0, 0);
            if constexpr (!(DBG & XD_VALU)) {
                float mx = -INFINITY;
#pragma unroll
                for (int r = 0; r < 16; ++r) mx = fmaxf(mx, acc[r]);
                mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
                // p = exp(scale (acc - mx)) = exp2(acc * (scale log2 e) - mx * (scale log2 e)): one fma + v_exp per element
                const float SL = 0.17677669529663687f * 1.4426950408889634f;
                const float nmx = -mx * SL;
                float sum = 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) { acc[r] = __builtin_amdgcn_exp2f(fmaf(acc[r], SL, nmx)); sum += acc[r]; }
                sum += __shfl_xor(sum, 32, 64);
                const float inv = 1.0f / sum;
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[r] *= inv;
            }
            // O^T[d][query] = sum_key V^T[key][d] P[key][query]: A = V^T registers, B = P registers (fp32 pipe, one chain)
            f32x16 oacc;
#pragma unroll
            for (int r = 0; r < 16; ++r) oacc[r] = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) oacc = __builtin_amdgcn_mfma_f32_32x32x2f32(vt[r], acc[r], oacc, 0, 0, 0);
            // y[co][f] += sum_d Wo[co][head*32 + d] O^T[d][f]:  A = Wo fragments (d in accumulator-row order), B = the pieces of O^T:
            // registers 8 s .. 8 s + 7 are one K fragment
            bf16x8 of[3][2];
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                float ov[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) ov[j] = oacc[8 * s + j];
                ta_split3x8<DBG>(ov, of[0][s], of[1][s], of[2][s]);
            }
#pragma unroll
            for (int t = 0; t < 6; ++t)
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const bf16x8* wp = wof + X3_PA[t] * wop;
                    const bf16x8 w0 = (DBG & XD_FRAG) ? xf[X3_PA[t]][s] : wp[(0 * 2 + s) * 64];
                    const bf16x8 w1 = (DBG & XD_FRAG) ? xf[X3_PA[t]][s + 2] : wp[(1 * 2 + s) * 64];
                    yacc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w0, of[X3_PB[t]][s], yacc[0], 0, 0, 0);
                    yacc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w1, of[X3_PB[t]][s], yacc[1], 0, 0, 0);
                }
        };
#pragma unroll 1
        for (int head = 0; head < 4; ++head) {
            const unsigned char* const wh = (head & 1) ? rB : wA;
            if constexpr (!(DBG & XD_BAR))
                __syncthreads();                       // this head's weights are in LDS; every wave is done with the other buffer (head 0:
                                                       // with the xn image)
            const bool next = head < 3 || more;        // (head 3 brings head 0 of the next tile)
            if constexpr (SKEW) {
                if (lag && head > 0) tail(head - 1, reinterpret_cast<const bf16x8*>(wo_base(head - 1)) + lane, wo_pitch(head - 1));
                __builtin_amdgcn_sched_barrier(0);     // (the front's fetches and fragment reads stay behind the tail: registers)
                front(wh, (head + 1) & 3, next);
                if (!lag) tail(head, reinterpret_cast<const bf16x8*>(wo_base(head)) + lane, wo_pitch(head));
            } else {
                front(wh, (head + 1) & 3, next);
                tail(head, reinterpret_cast<const bf16x8*>(wh) + lane + WQKV_E / 8, HEAD_E / 8);
            }
        }
        if constexpr (SKEW) {                          // the drain: waves 0 - 3 go on to the exit's first barrier
            if (lag) tail(3, reinterpret_cast<const bf16x8*>(wo_base(3)) + lane, wo_pitch(3));
            if (more) fetch_head(0, +1);               // Wo of the next tile's head 0 (waves 4 - 7), parked behind that barrier
        }
        // ---- 3. the next tile's x is requested and y leaves through region B: thread (token, half) adds the residual (L2-warm second
        //         read of x) and stores.  EXIT 0: in two halves of 32 channels, channels i*32 + half*16 .. + 16 per thread and half.
        //         EXIT 1: the whole image [64][XP] at once, channels half*32 .. + 32 per thread, and the residual is requested in
        //         front of the next tile's x -- loads return in order, so behind it the stores wait for that tile's trip to HBM.
        //         EXIT 2: EXIT 1 without the second read -- those are the 32 values the thread read for the LayerNorm, kept in
        //         registers across the heads (32 VGPRs; the skewed walk has no room for them).
        const __amdgpu_buffer_rsrc_t xb = ta_buf(a.x + tp), yb = ta_buf(a.y + tp);
        if constexpr (EXIT == 1 && !(DBG & XD_EXIT)) {
#pragma unroll
            for (int c = 0; c < 32; ++c) xr1[c] = ldb(xb, toff, hoff + (uint32_t)c * sc4);
        }
        if constexpr (!(DBG & XD_XNEXT)) {   // (unconditional: the last tile re-reads itself)
            const __amdgpu_buffer_rsrc_t xn = ta_buf(a.x + ta_tile_ptr(a, wk, more ? li + stride : li));
#pragma unroll
            for (int c = 0; c < 32; ++c) v[c] = ldb(xn, toff, hoff + (uint32_t)c * sc4);
        }
        if constexpr (DBG & XD_EXIT) {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) asm volatile("" ::"v"(yacc[i][r]));
            __syncthreads();
        } else if constexpr (EXIT >= 1) {
            __syncthreads();                           // every wave is done with head 3's weights
            if constexpr (SKEW)
                if (more) park_head(wA, +1);           // (Wo of head 3 was read until that barrier)
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) ys[(i * 32 + crow(r, lh)) * XP + hw * 33 + l31] = yacc[i][r];
            __syncthreads();
#pragma unroll
            for (int c = 0; c < 32; ++c) stb(yb, toff, hoff + (uint32_t)c * sc4, ys[(half * 32 + c) * XP + pw * 33 + f] + xr1[c]);
        } else {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                float xr[16];
                const uint32_t ch0 = (uint32_t)i * 32u * sc4 + (hoff >> 1);           // channel i*32 + half*16
#pragma unroll
                for (int c = 0; c < 16; ++c) xr[c] = (DBG & XD_RES) ? 0.f : ldb(xb, toff, ch0 + (uint32_t)c * sc4);
                __syncthreads();                       // every wave is done with head 3's weights / with the previous half of the y image
                if constexpr (SKEW)
                    if (i == 1 && more) park_head(wA, +1);     // (Wo of head 3 was read until the first of these barriers)
#pragma unroll
                for (int r = 0; r < 16; ++r) ys[crow(r, lh) * XP + hw * 33 + l31] = yacc[i][r];
                __syncthreads();
#pragma unroll
                for (int c = 0; c < 16; ++c) {
                    const float yv = ys[(half * 16 + c) * XP + pw * 33 + f] + xr[c];
                    if constexpr (DBG & XD_STORE) asm volatile("" ::"v"(yv));
                    else stb(yb, toff, ch0 + (uint32_t)c * sc4, yv);
                }
            }
        }
        __syncthreads();                               // the y image is consumed: region B is free for the next tile's xn
    }
}

// (EXIT 2: 237 VGPRs where EXIT 0 takes 204 -- the tile's raw x stays in registers across the heads; no spills, two waves per SIMD)
__global__ __launch_bounds__(NT) void ta_block_x3_kernel(const TaArgs a) { ta_x3_tiles<false, 2, 0>(a); }

// waves 4 - 7 half a head behind, y out in one pass ("The skewed form")
__global__ __launch_bounds__(NT) void ta_block_x3s_kernel(const TaArgs a) { ta_x3_tiles<true, 1, 0>(a); }

#ifdef SDC_KERNEL_EXPERIMENTS
template <bool SKEW, int EXIT>
__global__ __launch_bounds__(NT) void ta_block_x3_form_kernel(const TaArgs a) { ta_x3_tiles<SKEW, EXIT, 0>(a); }
template <int DBG>
__global__ __launch_bounds__(NT) void ta_block_x3_dbg_kernel(const TaArgs a) { ta_x3_tiles<false, 0, DBG>(a); }     // (the parent's exit)
#endif

// dst[head][piece][e], e < HEAD_E: the three bf16 pieces of the element that sdc_pack_tattn_f16 puts at fragment position e of the head
// (include/sdc.h), from the nn.Linear weights to_qkv (384, 64) and to_out (64, 128); one thread per element of a plane
__global__ __launch_bounds__(256) void pack_tattn_x3_kernel(const float* __restrict__ wqkv, const float* __restrict__ wo,
                                                            __bf16* __restrict__ dst) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= 4 * HEAD_E) return;
    const int head = g / HEAD_E, e = g - head * HEAD_E;
    const int j = e & 7, lane = (e >> 3) & 63, l31 = lane & 31, lh = lane >> 5;
    float wv;
    if (e < WQKV_E) {
        const int s = (e >> 9) & 3, mat = e >> 11;
        wv = wqkv[(mat * 128 + head * 32 + l31) * C + 16 * s + 8 * lh + j];
    } else {
        const int e2 = e - WQKV_E, s = (e2 >> 9) & 1, i = (e2 >> 10) & 1;
        wv = wo[(32 * i + l31) * 128 + head * 32 + crow(8 * s + j, lh)];
    }
    __bf16 ph, pm, pl;
    split3(wv, ph, pm, pl);
    __bf16* d = dst + (int64_t)head * 3 * HEAD_E + e;
    d[0] = ph; d[HEAD_E] = pm; d[2 * HEAD_E] = pl;
}

// The routing table of net.attn_split: the sites where every repeat of sdc_tattn_block_x3 measured faster than
// every repeat of sdc_tattn_block on the same buffers (profiles/attn_x3_shapes.log).  Per-sample sizes only, never B.
bool sdc_tattn_x3_faster(int Cc, int ntok, int inner) {
    return Cc == 64 && ntok == 32 && inner == 4096;
}

}  // namespace

extern "C" int sdc_tattn_block_x3_ok(int Cc, int ntok, int inner) { return sdc_tattn_x3_faster(Cc, ntok, inner) ? 1 : 0; }

extern "C" size_t sdc_pack_tattn_x3_bytes(void) { return (size_t)WPK_E * sizeof(__bf16); }

extern "C" int sdc_pack_tattn_x3(const float* wqkv, const float* wo, void* dst, void* stream) {
    SDC_REQUIRE(wqkv && wo && dst, SDC_ENULL, "sdc_pack_tattn_x3: null pointer");
    SDC_REQUIRE(reinterpret_cast<uintptr_t>(dst) % 16 == 0, SDC_EALIGN, "sdc_pack_tattn_x3: dst must be 16-byte aligned");
    hipLaunchKernelGGL(pack_tattn_x3_kernel, dim3(4 * HEAD_E / 256), dim3(256), 0, sdc::as_stream(stream), wqkv, wo,
                       reinterpret_cast<__bf16*>(dst));
    return sdc::check_launch("sdc_pack_tattn_x3");
}

namespace {

// impl 0: ta_block_x3_kernel; 1: ta_block_x3s_kernel (waves 4 - 7 half a head behind; the same bits).  Checks under the entry's name,
// all before any launch.
int tattn_block_x3_impl(const char* who, const float* x, const float* g_pre, const void* wpk, const float* rot, const float* bias,
                        float* y, int outer, int inner, int Cc, int ntok, int64_t so, int64_t sc, int64_t st, float eps, int impl,
                        void* stream) {
    SDC_REQUIRE(wpk, SDC_ENULL, "%s: null pointer", who);
    SDC_REQUIRE(impl == 0 || impl == 1, SDC_EINVAL, "%s: impl must be 0 or 1 (got %d)", who, impl);
    TaArgs a;
    if (const int rc = ta_check_args(who, x, g_pre, rot, bias, y, outer, inner, Cc, ntok, so, sc, st, eps, a)) return rc;
    a.wpk = reinterpret_cast<const __bf16*>(wpk);
    // the weight buffer is fetched with 16-byte and the rotary table with 8-byte vector loads
    SDC_REQUIRE(reinterpret_cast<uintptr_t>(wpk) % 16 == 0, SDC_EALIGN, "%s: the weight buffer must be 16-byte aligned", who);
    SDC_REQUIRE(!rot || reinterpret_cast<uintptr_t>(rot) % 8 == 0, SDC_EINVAL, "%s: rot must be 8-byte aligned", who);
    const size_t ldsb = (size_t)WBUF_B + REGB_B + TAB_B;
    unsigned grid = 0;
    if (const int rc = sdc::ta_grid(who, a.nblk, &grid)) return rc;
#define TAX3_LAUNCH(KERNEL, LDS)                                                                      \
    do {                                                                                              \
        static std::atomic<uint64_t> attr{0};                                                         \
        SDC_LDS_OPTIN(attr, KERNEL, 160 * 1024, who);                                                 \
        hipLaunchKernelGGL(KERNEL, dim3(grid), dim3(NT), LDS, sdc::as_stream(stream), a);             \
        return sdc::check_launch(who);                                                                \
    } while (0)
#ifdef SDC_KERNEL_EXPERIMENTS
    // SDC_TAX3_FORM (right results): the form of the tile whatever impl says -- bit 0 the skew; 0 / 1 the two-pass exit, 2 / 3 one
    // pass, 4 / 5 one pass with the residual kept in registers
    static const int form = getenv("SDC_TAX3_FORM") ? atoi(getenv("SDC_TAX3_FORM")) : -1;
    switch (form) {
        case 0: TAX3_LAUNCH((ta_block_x3_form_kernel<false, 0>), ldsb);
        case 1: TAX3_LAUNCH((ta_block_x3_form_kernel<true, 0>), ldsb + WOS_B);
        case 2: TAX3_LAUNCH((ta_block_x3_form_kernel<false, 1>), ldsb);
        case 3: TAX3_LAUNCH((ta_block_x3_form_kernel<true, 1>), ldsb + WOS_B);
        case 4: TAX3_LAUNCH((ta_block_x3_form_kernel<false, 2>), ldsb);
        case 5: TAX3_LAUNCH((ta_block_x3_form_kernel<true, 2>), ldsb + WOS_B);
        default: break;
    }
#endif
    if (impl == 1) TAX3_LAUNCH(ta_block_x3s_kernel, ldsb + WOS_B);
#ifdef SDC_KERNEL_EXPERIMENTS
    // kernel experiments of impl 0 (WRONG RESULTS): the XD_ bits above, one part off at a time, and MFMAs only
    static const int dbg = getenv("SDC_TAX3_DBG") ? atoi(getenv("SDC_TAX3_DBG")) : 0;
    switch (dbg) {
        case 0: break;
        case XD_LN: TAX3_LAUNCH(ta_block_x3_dbg_kernel<XD_LN>, ldsb);
        case XD_EXIT: TAX3_LAUNCH(ta_block_x3_dbg_kernel<XD_EXIT>, ldsb);
        case XD_SPLIT: TAX3_LAUNCH(ta_block_x3_dbg_kernel<XD_SPLIT>, ldsb);
        case XD_WFETCH: TAX3_LAUNCH(ta_block_x3_dbg_kernel<XD_WFETCH>, ldsb);
        case XD_FRAG: TAX3_LAUNCH(ta_block_x3_dbg_kernel<XD_FRAG>, ldsb);
        case XD_BAR: TAX3_LAUNCH(ta_block_x3_dbg_kernel<XD_BAR>, ldsb);
        case XD_VALU: TAX3_LAUNCH(ta_block_x3_dbg_kernel<XD_VALU>, ldsb);
        case XD_STORE: TAX3_LAUNCH(ta_block_x3_dbg_kernel<XD_STORE>, ldsb);
        case XD_RES: TAX3_LAUNCH(ta_block_x3_dbg_kernel<XD_RES>, ldsb);
        case XD_XNEXT: TAX3_LAUNCH(ta_block_x3_dbg_kernel<XD_XNEXT>, ldsb);
        case XD_STORE | XD_RES | XD_XNEXT: TAX3_LAUNCH(ta_block_x3_dbg_kernel<XD_STORE | XD_RES | XD_XNEXT>, ldsb);
        default: TAX3_LAUNCH(ta_block_x3_dbg_kernel<XD_MFMA_ONLY>, ldsb);
    }
#endif
    TAX3_LAUNCH(ta_block_x3_kernel, ldsb);
#undef TAX3_LAUNCH
}

}  // namespace

// The measured table of the skewed kernel ("The skewed form"; profiles/attn_x3_skew_shapes.log): 1 at the
// per-sample sizes -- never B -- where every repeat of impl 1 beat every repeat of impl 0 at the bench batch.
extern "C" int sdc_tattn_block_x3_impl(int Cc, int ntok, int inner) {
    (void)Cc; (void)ntok; (void)inner;
    return 0;
}

extern "C" int sdc_tattn_block_x3_sel(const float* x, const float* g_pre, const void* wpk, const float* rot, const float* bias, float* y,
                                      int outer, int inner, int Cc, int ntok, int64_t so, int64_t sc, int64_t st, float eps, int impl,
                                      void* stream) {
    return tattn_block_x3_impl("sdc_tattn_block_x3_sel", x, g_pre, wpk, rot, bias, y, outer, inner, Cc, ntok, so, sc, st, eps, impl, stream);
}

extern "C" int sdc_tattn_block_x3(const float* x, const float* g_pre, const void* wpk, const float* rot, const float* bias, float* y,
                                  int outer, int inner, int Cc, int ntok, int64_t so, int64_t sc, int64_t st, float eps, void* stream) {
    return tattn_block_x3_impl("sdc_tattn_block_x3", x, g_pre, wpk, rot, bias, y, outer, inner, Cc, ntok, so, sc, st, eps,
                               sdc_tattn_block_x3_impl(Cc, ntok, inner), stream);
}
