// net.linattn_f16 (opt-in, samplers only): the fused LinearAttention block of sdc_lablock.hip with fp16 operands on the gfx950
// 16-bit matrix pipe, v_mfma_f32_32x32x16_f16 -- fp16 operands rounded to nearest even, fp32 accumulation:
//
//   y = x + post( Wo . LA(pre(x)) + bo ),   LA: q = softmax_d(Wq xn) * 32^-0.5, k = softmax_n(Wk xn), v = Wv xn,
//                                               ctx = k v^T (32x32 per head), out = ctx^T q
//
// Same three launches, shape domain, strides, token splits (pick_nsplit) and GroupNorm-on-load form as la_blk_ctx / la_blk_mid /
// la_blk_out.  What differs:
//   pass 1  la16_ctx : xn sits in LDS as fp16, twice: token-major (the 8 channels of a K fragment are one 16-byte read: A operand of
//                      K^T = xn^T Wk^T) and channel-major with the tokens of a tile in accumulator-row order (A operand of
//                      M^T += xn p).  Wk arrives as ready fp16 fragments.  The un-normalised probabilities p are converted to fp16 in
//                      the accumulator registers where they stand -- eight consecutive registers of a lane are one K fragment, whose
//                      contraction index runs in accumulator-row order row(r, lh).  16 MFMAs of K = 16 per tile and head at C = 64
//                      instead of 128 of K = 2.
//                      The reference maximum is an integer exponent: p = exp2(k log2e - ceil(m log2e)), m the running maximum.  Every
//                      rescale factor -- of the running accumulators, of the row sum, of the split merge -- is then an exact power
//                      of two, so the fp16 rounding of p depends neither on the tile order nor on the split count.  The row sum is of
//                      the unrounded fp32 p.
//   mid     la16_mid : fp32 on the fp32 packed weights, la_blk_mid's sums in la_blk_mid's order; T = Wo ctx is written once, rounded
//                      to fp16, in the fragment order pass 2 reads.
//   pass 2  la16_out : Q = Wq xn from fp16 fragments; softmax over d and the scale in fp32; q 32^-0.5 converted to fp16 in the
//                      registers (eight consecutive registers = one K fragment of y = T q); bias, post norm, + x, store in fp32.
// Rounded once to fp16 (RNE) as matrix operands, and nothing else: xn, Wq and Wk (at pack time), p, T, q after softmax and scale.
// fp32: both channel norms, the GroupNorm-on-load arithmetic and the stored h, maxima, exponents, row sums, the split merge, ctx,
// every accumulator, the residual add.  An operand beyond 65504 (T is the one without a bound) becomes infinite.
// No atomics, fixed accumulation order, a sample's arithmetic does not see the batch.
#include "sdc_common.h"
#include "sdc_lablock_tile.h"
#include "sdc_f16frag.h"

namespace {

constexpr int TP = TT + 8;               // pitch (halves) of one channel row of the channel-major xn: 64 tokens + 16 bytes
__host__ __device__ constexpr int cpitch(int C) { return C + 8; }      // pitch (halves) of one token of the token-major xn

struct La16Args {
    const float* x;
    const float* g_pre;
    const _Float16* wpk;    // sdc_pack_linattn_f16: Wq | Wk fragments
    const float* wqkv;      // packed fp32 [C][384] (mid: Wv)
    const float* wo;        // packed fp32 [128][C] (mid)
    const float* bo;        // [C] or null
    const float* g_post;    // [C] or null
    float* part;            // [nseq][nsplit][4][32*(C+2)]
    _Float16* tt;           // [nseq][C/32][8][64][8]  T fragments
    float* y;
    const float* gn_stats; const float* gn_gamma; const float* gn_beta; const float* gn_res;      // as LaArgs
    float* gn_hout;
    int gn_G;
    int inner, nsplit, tiles_per_split, ntiles, tiles_per_blk;
    int pre_mode, post_mode;
    float eps;
    int64_t so, sc, si;
};

// 2^d for an integer-valued d <= 0 (-inf included): exact
__device__ __forceinline__ float pow2_neg(float d) { return ldexpf(1.0f, (int)fmaxf(d, -200.0f)); }

// norm_tile_regs (the fp32 expressions of every build: xn before its rounding has la_blk's bits) storing xn as fp16:
// xt[tok][c] always; xc[c][pos(tok)], when given, with pos = tok with bits 2 and 3 swapped -- positions 16 q + 8 lh + j of a row hold
// the tokens 16 q + row(j, lh) of the tile, the order in which a lane's accumulator registers walk the tokens.
template <int C>
__device__ __forceinline__ void norm_tile16(float (&v)[C / 4], const float* __restrict__ g, int mode, float eps, _Float16* __restrict__ xt,
                                            _Float16* __restrict__ xc, float* __restrict__ xr, float* __restrict__ red, int tid) {
    constexpr int CG = C / 4, CP = cpitch(C);
    const int tok = tid & 63, grp = tid >> 6;
    float o[CG];
    norm_tile_regs<C>(v, g, mode, eps, xr, red, tid, o);
    half8* xo = reinterpret_cast<half8*>(xt + tok * CP + grp * CG);
    const int pos = (tok & ~12) | ((tok & 4) << 1) | ((tok & 8) >> 1);
#pragma unroll
    for (int c8 = 0; c8 < CG / 8; ++c8) {
        half8 h;
#pragma unroll
        for (int j = 0; j < 8; ++j) h[j] = (_Float16)o[c8 * 8 + j];
        xo[c8] = h;
        if (xc) {
#pragma unroll
            for (int j = 0; j < 8; ++j) xc[(grp * CG + c8 * 8 + j) * TP + pos] = h[j];
        }
    }
    __syncthreads();
}

// ------------------------------------------------------------------ pass 1: per (split, sequence); wave = head
// Transposed like la_blk_ctx, so that the reductions run over registers and the products chain without LDS:
//   K^T[tok][d] = xn^T Wk^T: A = xn (rows = tokens), B = the Wk fragments; register r of tile j is token j*32 + row(r, lh), d = l31
//   M^T[c][d] += sum_tok xn[c][tok] p[tok][d]: A = xn rows c from the channel-major copy, B = registers 8 q .. 8 q + 7 of p as they
//   stand; the online rescale factor is per d = per lane, a power of two.
template <int C, bool GN>
__global__ __launch_bounds__(NT, (C == 64 ? 2 : 1)) void la16_ctx(const La16Args a) {
    constexpr int NCT = C / 32, NKS = C / 16, CP = cpitch(C);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem16[];
    _Float16* const xt = reinterpret_cast<_Float16*>(smem16);          // [TT][CP]
    _Float16* const xc = xt + TT * CP;                                  // [C][TP]
    float* const red = reinterpret_cast<float*>(xc + C * TP);           // [8][TT]
    float* const gcoef = red + 8 * TT;                                  // [2][C]  (GroupNorm-on-load form only)
    const int tid = threadIdx.x, lane = tid & 63, head = tid >> 6, l31 = lane & 31, lh = lane >> 5;
    const int split = blockIdx.x, seq = blockIdx.y;
    const int o = seq / a.inner, i = seq - o * a.inner;
    const float* xseq = a.x + o * a.so + i * a.si;
    const float* rseq = (GN && a.gn_res) ? a.gn_res + o * a.so + i * a.si : nullptr;
    if (GN) gn_coef_fill<C>(a.gn_stats, a.gn_gamma, a.gn_beta, a.gn_G, o, gcoef, tid);

    half8 wk[NKS];                                  // Wk_h[d = l31][c = 16 s + 8 lh + j]
#pragma unroll
    for (int s = 0; s < NKS; ++s) wk[s] = reinterpret_cast<const half8*>(a.wpk)[((4 + head) * NKS + s) * 64 + lane];

    f32x16 macc[NCT];                               // M^T tile t: rows c = t*32 + row(r, lh), columns d = l31
#pragma unroll
    for (int t = 0; t < NCT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) macc[t][r] = 0.f;
    float erun = -INFINITY, psum = 0.f;             // per d (this lane): ceil(running max * log2e), row sum relative to 2^erun

    const int t0 = split * a.tiles_per_split;
    const int t1 = min(t0 + a.tiles_per_split, a.ntiles);
    float xv[C / 4];
    if (t0 < t1) fetch_tile<C>(xseq + (int64_t)t0 * TT, a.sc, tid, xv);
    if (GN) __syncthreads();                        // coefficient table complete
    for (int tile = t0; tile < t1; ++tile) {
        if (GN) {
            // h once, here, in fp32: pass 2 reads it back from the block's own output buffer
            gn_apply_tile<C>(xv, rseq ? rseq + (int64_t)tile * TT : nullptr, a.sc, gcoef, tid);
            gn_store_h<C>(a.gn_hout + o * a.so + i * a.si + (int64_t)tile * TT, a.sc, tid, xv);
        }
        norm_tile16<C>(xv, a.g_pre, a.pre_mode, a.eps, xt, xc, nullptr, red, tid);
        if (tile + 1 < t1) fetch_tile<C>(xseq + (int64_t)(tile + 1) * TT, a.sc, tid, xv);
        f32x16 kacc[2];
#pragma unroll
        for (int r = 0; r < 16; ++r) { kacc[0][r] = 0.f; kacc[1][r] = 0.f; }
#pragma unroll
        for (int s = 0; s < NKS; ++s) {
            const half8 a0 = *reinterpret_cast<const half8*>(xt + l31 * CP + 16 * s + 8 * lh);
            const half8 a1 = *reinterpret_cast<const half8*>(xt + (32 + l31) * CP + 16 * s + 8 * lh);
            kacc[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, wk[s], kacc[0], 0, 0, 0);
            kacc[1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, wk[s], kacc[1], 0, 0, 0);
        }
        // online softmax over tokens, per d, against an integer exponent: not la_softmax_tok -- the reference is ceil(m log2e), the
        // factor pow2_neg's exact power of two, and the first maximum has a form of its own
        // (the first maximum in plain C++, as in la16_out: it reads the accumulators the last two MFMAs have just written, and
        // behind la_max3's asm statement the compiler places no wait states -- at C = 64 the v_max3_f32 stood directly behind
        // the MFMA and read a register that was stale or not with the load of the CU: run-to-run differences in the last bits
        // once every CU was busy.  In front of the plain form it places them, and the rest of the chain depends on it.)
        float tmax = fmaxf(kacc[0][0], kacc[1][0]);
#pragma unroll
        for (int r = 1; r < 16; ++r) tmax = la_max3(tmax, kacc[0][r], kacc[1][r]);
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
        const float enew = fmaxf(erun, ceilf(tmax * LOG2E));
        const float f = pow2_neg(erun - enew);
        erun = enew;
        float ps = 0.f;
        const float nml = -enew;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            kacc[0][r] = __builtin_amdgcn_exp2f(fmaf(kacc[0][r], LOG2E, nml));
            kacc[1][r] = __builtin_amdgcn_exp2f(fmaf(kacc[1][r], LOG2E, nml));
            ps += kacc[0][r] + kacc[1][r];
        }
        psum = psum * f + ps;
        la_rescale<NCT>(macc, f);
        // step (j, q): tokens j*32 + row(8 q + jj, lh) = positions j*32 + 16 q + 8 lh + jj of the channel-major rows
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const half8 pf = frag(kacc[j], 8 * q);
#pragma unroll
                for (int t = 0; t < NCT; ++t) {
                    const half8 xa = *reinterpret_cast<const half8*>(xc + (t * 32 + l31) * TP + j * 32 + 16 * q + 8 * lh);
                    macc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(xa, pf, macc[t], 0, 0, 0);
                }
            }
        __syncthreads();                             // xt / xc are rewritten by the next tile
    }
    // the partial's m is e, the integer exponent
    la_store_partial<C>(a.part + (((int64_t)seq * a.nsplit + split) * 4 + head) * (32 * (C + 2)), macc, erun, psum, l31, lh);
}

// ------------------------------------------------------------------ mid: per (sequence, head)
template <int C>
__global__ __launch_bounds__(NT) void la16_mid(const La16Args a) {
    __shared__ float Ms[32][C + 1];
    __shared__ float cs[32][33];
    __shared__ float fsp[8][32];                    // per split: 2^(e_s - e): exact; nsplit <= 8
    __shared__ float rs[32];
    const int tid = threadIdx.x;
    const int head = blockIdx.x, seq = blockIdx.y;
    const float* pb = a.part + ((int64_t)seq * a.nsplit * 4 + head) * (32 * (C + 2));
    const int64_t sstride = (int64_t)4 * 32 * (C + 2);
    if (tid < 32) {
        float m = -INFINITY;
        for (int s = 0; s < a.nsplit; ++s) m = fmaxf(m, pb[s * sstride + 32 * C + tid]);
        float tot = 0.f;
        for (int s = 0; s < a.nsplit; ++s) {
            const float f = pow2_neg(pb[s * sstride + 32 * C + tid] - m);
            fsp[s][tid] = f;
            tot += f * pb[s * sstride + 32 * C + 32 + tid];
        }
        rs[tid] = 1.0f / tot;
    }
    __syncthreads();
    for (int e = tid; e < 32 * C; e += NT) {
        const int d = e / C, c = e - d * C;
        float v = 0.f;
        for (int s = 0; s < a.nsplit; ++s) v += fsp[s][d] * pb[s * sstride + e];
        Ms[d][c] = v;
    }
    __syncthreads();
    // ctx[d][e] = sum_c M[d][c] Wv[e][c] / rowsum[d]
    for (int q = tid; q < 32 * 32; q += NT) {
        const int d = q >> 5, e = q & 31;
        float v = 0.f;
        for (int c = 0; c < C; ++c) v += Ms[d][c] * a.wqkv[(int64_t)c * (3 * HID) + 2 * HID + head * 32 + e];
        cs[d][e] = v * rs[d];
    }
    __syncthreads();
    // T[co][head*32 + d] = sum_e Wo[head*32 + e][co] ctx[d][e], rounded once, to the K fragments of pass 2:
    // Tf[rt][s = 2 head + q][lane][j] = T[rt*32 + l31][head*32 + row(8 q + j, lh)]
    _Float16* tb = a.tt + (int64_t)seq * HID * C;
    for (int p = tid; p < 32 * C; p += NT) {
        const int j = p & 7, lane = (p >> 3) & 63, q = (p >> 9) & 1, rt = p >> 10;
        const int co = rt * 32 + (lane & 31), d = crow(8 * q + j, lane >> 5);
        float v = 0.f;
#pragma unroll 8
        for (int e = 0; e < 32; ++e) v += a.wo[(int64_t)(head * 32 + e) * C + co] * cs[d][e];
        tb[((rt * 8 + 2 * head + q) * 64 + lane) * 8 + j] = (_Float16)v;
    }
}

// ------------------------------------------------------------------ pass 2: per (tile group, sequence)
template <int C>
__global__ __launch_bounds__(NT, (C == 64 ? 2 : 1)) SDC_NO_DS_MERGE void la16_out(const La16Args a) {
    constexpr int NRT = C / 32;                     // row tiles of y (channels)
    constexpr int TPW = NRT / 2;                    // y tiles per wave (one row tile, TPW column tiles)
    constexpr int NKS = C / 16, CP = cpitch(C);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem16[];
    _Float16* const xt = reinterpret_cast<_Float16*>(smem16);          // [TT][CP]
    half8* const qs = reinterpret_cast<half8*>(xt + TT * CP);           // [8 steps][2 column tiles][64 lanes]: q as K fragments
    float* const red = reinterpret_cast<float*>(qs + 8 * 2 * 64);       // [8][TT]
    float* const xr = red + 8 * TT;                 // [C][XP] raw x tile (residual)
    float* const bg = xr + C * XP;                  // [2][C] bias | post gain
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lh = lane >> 5;
    const int seq = blockIdx.y;
    const int o = seq / a.inner, i = seq - o * a.inner;
    const float* xseq = a.x + o * a.so + i * a.si;
    float* yseq = a.y + o * a.so + i * a.si;
    const int rt = (NRT == 2) ? (wave & 1) : wave;  // this wave's row tile of y
    const int ct0 = (NRT == 2) ? (wave >> 1) : 0;   // its first column tile

    half8 wq[NKS];                                  // Wq_h[d = l31][c = 16 s + 8 lh + j], head = wave
#pragma unroll
    for (int s = 0; s < NKS; ++s) wq[s] = reinterpret_cast<const half8*>(a.wpk)[(wave * NKS + s) * 64 + lane];
    half8 tf[8];                                    // T[co = rt*32 + l31][hd = (s >> 1)*32 + row(8 (s & 1) + j, lh)]
    const half8* tb = reinterpret_cast<const half8*>(a.tt + (int64_t)seq * HID * C);
#pragma unroll
    for (int s = 0; s < 8; ++s) tf[s] = tb[(rt * 8 + s) * 64 + lane];
    for (int c = tid; c < C; c += NT) {
        bg[c] = a.bo ? a.bo[c] : 0.f;
        bg[C + c] = a.g_post ? a.g_post[c] : 1.f;
    }

    const int t0 = blockIdx.x * a.tiles_per_blk;
    const int t1 = min(t0 + a.tiles_per_blk, a.ntiles);
    float xv[C / 4];
    if (t0 < t1) fetch_tile<C>(xseq + (int64_t)t0 * TT, a.sc, tid, xv);
    for (int tile = t0; tile < t1; ++tile) {
        norm_tile16<C>(xv, a.g_pre, a.pre_mode, a.eps, xt, nullptr, xr, red, tid);
        if (tile + 1 < t1) fetch_tile<C>(xseq + (int64_t)(tile + 1) * TT, a.sc, tid, xv);
        // Q[d = row(r, lh)][tok = j*32 + l31] of head = wave
        f32x16 qacc[2];
#pragma unroll
        for (int r = 0; r < 16; ++r) { qacc[0][r] = 0.f; qacc[1][r] = 0.f; }
#pragma unroll
        for (int s = 0; s < NKS; ++s) {
            const half8 b0 = *reinterpret_cast<const half8*>(xt + l31 * CP + 16 * s + 8 * lh);
            const half8 b1 = *reinterpret_cast<const half8*>(xt + (32 + l31) * CP + 16 * s + 8 * lh);
            qacc[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wq[s], b0, qacc[0], 0, 0, 0);
            qacc[1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wq[s], b1, qacc[1], 0, 0, 0);
        }
        // softmax over d (the 32 rows of the head) per token, times dim_head^-0.5: fp32; then one rounding
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const float f = la_softmax_d<la_max3>(qacc[j]);
            // registers 8 q .. 8 q + 7: the K fragment of step 2 wave + q for column tile j, on the lane that reads it back
#pragma unroll
            for (int q = 0; q < 2; ++q) qs[((2 * wave + q) * 2 + j) * 64 + lane] = frag(qacc[j], 8 * q, f);
        }
        __syncthreads();
        // y[co][tok] = sum_hd T[co][hd] q[hd][tok]
        f32x16 yacc[TPW];
#pragma unroll
        for (int u = 0; u < TPW; ++u)
#pragma unroll
            for (int r = 0; r < 16; ++r) yacc[u][r] = bg[rt * 32 + crow(r, lh)];
#pragma unroll
        for (int s = 0; s < 8; ++s)
#pragma unroll
            for (int u = 0; u < TPW; ++u)
                yacc[u] = __builtin_amdgcn_mfma_f32_32x32x16_f16(tf[s], qs[(s * 2 + ct0 + u) * 64 + lane], yacc[u], 0, 0, 0);
        if (a.post_mode >= 0) la_post_norm<C, false>(yacc, a.post_mode, a.eps, bg, red, rt, ct0, l31, lh);
        la_store_residual<C>(yacc, yseq + (int64_t)tile * TT, a.sc, xr, rt, ct0, l31, lh);
        __syncthreads();                             // xt / qs / red / xr are rewritten by the next tile
    }
}

// dst[e], e < 256 C: the layout of include/sdc.h from the nn.Linear / 1x1 conv weight to_qkv (384, C)
__global__ __launch_bounds__(256) void pack_linattn_f16_kernel(const float* __restrict__ wqkv, _Float16* __restrict__ dst, int C) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= 256 * C) return;
    const int nks = C / 16;
    const int j = e & 7, lane = (e >> 3) & 63, s = (e >> 9) % nks, mh = (e >> 9) / nks;     // mh = mat * 4 + head = row block of 32
    dst[e] = (_Float16)wqkv[(int64_t)(mh * 32 + (lane & 31)) * C + 16 * s + 8 * (lane >> 5) + j];
}

size_t lds_ctx(int C) { return sizeof(_Float16) * (size_t)(TT * cpitch(C) + C * TP) + sizeof(float) * (size_t)(8 * TT + 2 * C); }
size_t lds_out(int C) { return sizeof(_Float16) * (size_t)(TT * cpitch(C) + 8 * 2 * 64 * 8) + sizeof(float) * (size_t)(8 * TT + C * XP + 2 * C); }

int linattn_block_f16_impl(const char* who, const float* x, const float* gn_stats, const float* gn_gamma, const float* gn_beta, int gn_G,
                           const float* gn_res, const float* g_pre, const float* wqkv, const float* wo, const void* wpk, const float* bo,
                           const float* g_post, void* work, float* y, int outer, int inner, int C, int64_t n, int64_t so, int64_t sc,
                           int64_t si, int pre_mode, int post_mode, float eps, void* stream) {
    SDC_REQUIRE(x && g_pre && wqkv && wo && wpk && work && y, SDC_ENULL, "%s: null pointer", who);
    La16Args a;
    LaGrids g;
    float* tt_at;
    const int rc0 = la_host_setup(who, a, x, gn_stats, gn_gamma, gn_beta, gn_G, gn_res, g_pre, bo, g_post, work, y, outer, inner, C, n, so, sc,
                                  si, pre_mode, post_mode, eps, g, &tt_at);
    if (rc0 != SDC_OK) return rc0;
    // the kernels read the fragments of the weights and of T (behind the partials in `work`) with 16-byte vector loads
    SDC_REQUIRE(reinterpret_cast<uintptr_t>(wpk) % 16 == 0, SDC_EALIGN, "%s: the fp16 weight buffer must be 16-byte aligned", who);
    SDC_REQUIRE(reinterpret_cast<uintptr_t>(work) % 16 == 0, SDC_EALIGN, "%s: work must be 16-byte aligned", who);
    a.wpk = reinterpret_cast<const _Float16*>(wpk); a.wqkv = wqkv; a.wo = wo;
    a.tt = reinterpret_cast<_Float16*>(tt_at);
    hipStream_t s = sdc::as_stream(stream);
    const size_t l1 = lds_ctx(C), l2 = lds_out(C);
    static std::atomic<uint64_t> attr{0};
    SDC_LDS_OPTIN(attr, la16_out<128>, 96 * 1024, who);          // 70 KB; every other instantiation stays below 64 KB
    const bool gn = gn_stats != nullptr;
    La16Args a2 = a;                                // pass 2 of the GroupNorm-on-load form: x = the h pass 1 left in y
    if (gn) { a.gn_hout = y; a2.x = y; a2.gn_stats = nullptr; }
    if (C == 64) {
        if (gn) hipLaunchKernelGGL((la16_ctx<64, true>), g.ctx, dim3(NT), l1, s, a);
        else hipLaunchKernelGGL((la16_ctx<64, false>), g.ctx, dim3(NT), l1, s, a);
        hipLaunchKernelGGL(la16_mid<64>, g.mid, dim3(NT), 0, s, a);
        hipLaunchKernelGGL(la16_out<64>, g.out, dim3(NT), l2, s, a2);
    } else {
        if (gn) hipLaunchKernelGGL((la16_ctx<128, true>), g.ctx, dim3(NT), l1, s, a);
        else hipLaunchKernelGGL((la16_ctx<128, false>), g.ctx, dim3(NT), l1, s, a);
        hipLaunchKernelGGL(la16_mid<128>, g.mid, dim3(NT), 0, s, a);
        hipLaunchKernelGGL(la16_out<128>, g.out, dim3(NT), l2, s, a2);
    }
    return sdc::check_launch(who);
}

}  // namespace

extern "C" size_t sdc_pack_linattn_f16_bytes(int C) { return (C == 64 || C == 128) ? (size_t)256 * C * sizeof(_Float16) : 0; }

extern "C" int sdc_pack_linattn_f16(const float* wqkv, const float* wo, int C, void* dst, void* stream) {
    SDC_REQUIRE(wqkv && wo && dst, SDC_ENULL, "sdc_pack_linattn_f16: null pointer");
    SDC_REQUIRE(C == 64 || C == 128, SDC_EINVAL, "sdc_pack_linattn_f16: dim must be 64 or 128 (got %d)", C);
    SDC_REQUIRE(reinterpret_cast<uintptr_t>(dst) % 16 == 0, SDC_EALIGN, "sdc_pack_linattn_f16: dst must be 16-byte aligned");
    // (to_out is not read: T = Wo ctx is formed in fp32 from the fp32 weights and rounded per sequence, by la16_mid)
    hipLaunchKernelGGL(pack_linattn_f16_kernel, dim3(C), dim3(256), 0, sdc::as_stream(stream), wqkv, reinterpret_cast<_Float16*>(dst), C);
    return sdc::check_launch("sdc_pack_linattn_f16");
}

extern "C" int sdc_linattn_block_f16_ok(int C, int64_t n) { return (C == 64 || C == 128) && n > 0 && n % TT == 0; }

extern "C" size_t sdc_linattn_block_f16_bytes(int outer, int inner, int C, int64_t n) {
    if (outer <= 0 || inner <= 0 || n <= 0 || (C != 64 && C != 128)) return 0;
    const int64_t nseq = (int64_t)outer * inner;
    return sizeof(float) * la_part_floats(nseq, C, n) + sizeof(_Float16) * (size_t)(nseq * HID * C);
}

extern "C" int sdc_linattn_block_f16(const float* x, const float* g_pre, const float* wqkv, const float* wo, const void* wpk, const float* bo,
                                     const float* g_post, void* work, float* y, int outer, int inner, int C, int64_t n, int64_t so,
                                     int64_t sc, int64_t si, int pre_mode, int post_mode, float eps, void* stream) {
    return linattn_block_f16_impl("sdc_linattn_block_f16", x, nullptr, nullptr, nullptr, 0, nullptr, g_pre, wqkv, wo, wpk, bo, g_post, work, y,
                                  outer, inner, C, n, so, sc, si, pre_mode, post_mode, eps, stream);
}

extern "C" int sdc_linattn_block_gn_f16(const float* x_raw, const float* gn_stats, const float* gn_gamma, const float* gn_beta, int gn_G,
                                        const float* gn_residual, const float* g_pre, const float* wqkv, const float* wo, const void* wpk,
                                        const float* bo, const float* g_post, void* work, float* y, int outer, int inner, int C, int64_t n,
                                        int64_t so, int64_t sc, int64_t si, int pre_mode, int post_mode, float eps, void* stream) {
    SDC_REQUIRE(gn_stats && gn_gamma && gn_beta, SDC_ENULL, "sdc_linattn_block_gn_f16: null GroupNorm pointer");
    SDC_REQUIRE(gn_G > 0 && (C == 64 || C == 128) && C % gn_G == 0, SDC_EINVAL, "sdc_linattn_block_gn_f16: groups must divide the channels");
    return linattn_block_f16_impl("sdc_linattn_block_gn_f16", x_raw, gn_stats, gn_gamma, gn_beta, gn_G, gn_residual, g_pre, wqkv, wo, wpk, bo,
                                  g_post, work, y, outer, inner, C, n, so, sc, si, pre_mode, post_mode, eps, stream);
}
