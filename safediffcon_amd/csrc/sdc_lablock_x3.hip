// The fused LinearAttention block of sdc_lablock.hip with the two products that have a weight operand -- K^T = xn^T Wk^T of pass 1 and
// Q = Wq xn of pass 2, half of the block's MFMAs -- formed on the gfx950 bf16 matrix pipe, v_mfma_f32_32x32x16_bf16, from EXACT three-way
// bf16 operand splits (the arithmetic of conv_stem_x3_kernel and ta_block_x3_kernel, DESIGN.md sections 14 and 19):
//
//   a = a1 + a2 + a3 (RNE bf16 pieces, exact fp32 residuals);  a b ~ a3 b1 + a2 b2 + a1 b3 + a2 b1 + a1 b2 + a1 b1, fp32 accumulation
//
// An fp32-grade result in another rounding order, not a reduced precision.  Launches, grids, arguments, work buffers, token splits and
// the GroupNorm-on-load form are la_blk_ctx / la_blk_mid / la_blk_out's; la_blk_mid runs as it is.  What is split:
//   - the weights, in the kernel: Wk_h (pass 1) / Wq_h (pass 2) are read from the packed fp32 wqkv before the tile loop, split there and
//     held as ready B / A fragments (3 x C/16 fragments of 8 bf16 per lane) for the workgroup's life -- no packed buffer;
//   - xn, once per value and tile, by the thread that normalises it (norm_tile's expressions: xn has la_blk's bits): three bf16 images
//     [piece][token][C + 8] in LDS, a lane's K fragment (8 consecutive channels of one token) one 16-byte read; shared by the four heads.
// A product's five small terms are issued first, smallest kind first, each over all its K steps, then the main term: one accumulator per
// output.  The bf16 MFMA's accumulators have the fp32 one's register layout, so everything behind the projections is la_blk's code, on
// the fp32 pipe, in its order: the online softmax over tokens, the rescale, M^T += xn p (pass 1 keeps the fp32 xn image for it), the
// softmax over d, y = T q, the post norm, the residual, the stores.
// No atomics, fixed accumulation order, a sequence's arithmetic does not see the batch.  A non-finite x gives NaN (inf - inf in the
// residual of the split) where the fp32 kernels may give an infinity.
#include "sdc_common.h"
#include "sdc_lablock_tile.h"
#include "sdc_split3.h"

namespace {

__host__ __device__ constexpr int cpitch(int C) { return C + 8; }      // pitch (bf16) of one token of a piece image: C channels + 16 bytes
// xn pieces whose fragments a wave keeps in registers across the six terms at C = 64 (project_x3): pass 1 has room for all three,
// pass 2 (64 registers of T) for the first
constexpr int PRE_CTX64 = 3, PRE_OUT64 = 1;
// max(a, b, c) in plain C++, not la_max3's inline v_max3_f32: behind an asm statement the compiler does not place the wait states a VALU
// read of a bf16 MFMA's fresh accumulator needs (the first maximum reads one), and the stale register showed as run-to-run differences
// in the last bits at full size (DESIGN.md section 19 met the same with a packed asm pair).  The maximum itself is exact either way.
__device__ __forceinline__ float x3_max3(float a, float b, float c) { return fmaxf(fmaxf(a, b), c); }
__host__ __device__ constexpr int piece_e(int C) { return TT * cpitch(C); }      // bf16 elements of one piece image

// norm_tile of sdc_lablock.hip (the same fp32 expressions: xn has la_blk's bits) leaving xn as fp32 xs[c][tok] (when given: the A
// operand of pass 1's M product) and as three bf16 pieces xt[piece][tok][c].
template <int C>
__device__ __forceinline__ void norm_tile_x3(float (&v)[C / 4], const float* __restrict__ g, int mode, float eps, float* __restrict__ xs,
                                             __bf16* __restrict__ xt, float* __restrict__ xr, float* __restrict__ red, int tid) {
    constexpr int CG = C / 4, CP = cpitch(C);
    const int tok = tid & 63, grp = tid >> 6;
    if (xr) {
#pragma unroll
        for (int k = 0; k < CG; ++k) xr[(grp * CG + k) * XP + tok] = v[k];
    }
    typedef float la_f2 __attribute__((ext_vector_type(2)));
    la_f2 s2 = {0.f, 0.f};
    float o[CG];
    if (mode == 0) {
#pragma unroll
        for (int k = 0; k < CG; k += 2) s2 += la_f2{v[k], v[k + 1]};
        red[grp * TT + tok] = s2.x + s2.y;
        __syncthreads();
        const float mean = (red[tok] + red[TT + tok] + red[2 * TT + tok] + red[3 * TT + tok]) * (1.0f / C);
        const la_f2 m2 = {mean, mean};
        la_f2 q2 = {0.f, 0.f};
#pragma unroll
        for (int k = 0; k < CG; k += 2) {
            const la_f2 d2 = la_f2{v[k], v[k + 1]} - m2;
            v[k] = d2.x; v[k + 1] = d2.y;
            q2 += d2 * d2;
        }
        red[(4 + grp) * TT + tok] = q2.x + q2.y;
        __syncthreads();
        const float var = (red[4 * TT + tok] + red[5 * TT + tok] + red[6 * TT + tok] + red[7 * TT + tok]) * (1.0f / C);
        const float rstd = rsqrtf(var + eps);
        const la_f2 r2 = {rstd, rstd};
#pragma unroll
        for (int k = 0; k < CG; k += 2) {
            const la_f2 o2 = la_f2{v[k], v[k + 1]} * r2 * la_f2{g[grp * CG + k], g[grp * CG + k + 1]};
            o[k] = o2.x; o[k + 1] = o2.y;
        }
    } else {
#pragma unroll
        for (int k = 0; k < CG; k += 2) { const la_f2 d2 = {v[k], v[k + 1]}; s2 += d2 * d2; }
        red[grp * TT + tok] = s2.x + s2.y;
        __syncthreads();
        const float nrm = sqrtf(red[tok] + red[TT + tok] + red[2 * TT + tok] + red[3 * TT + tok]);
        const float f = sqrtf((float)C) / fmaxf(nrm, 1e-12f);
        const la_f2 f2 = {f, f};
#pragma unroll
        for (int k = 0; k < CG; k += 2) {
            const la_f2 o2 = la_f2{v[k], v[k + 1]} * f2 * la_f2{g[grp * CG + k], g[grp * CG + k + 1]};
            o[k] = o2.x; o[k + 1] = o2.y;
        }
    }
    if (xs) {
#pragma unroll
        for (int k = 0; k < CG; ++k) xs[(grp * CG + k) * XP + tok] = o[k];
    }
    bf16x8* xo = reinterpret_cast<bf16x8*>(xt + tok * CP + grp * CG);
#pragma unroll
    for (int c8 = 0; c8 < CG / 8; ++c8) {
        bf16x8 ph, pm, pl;
        split3x8(o + c8 * 8, ph, pm, pl);
        xo[c8] = ph;
        xo[piece_e(C) / 8 + c8] = pm;
        xo[2 * (piece_e(C) / 8) + c8] = pl;
    }
    __syncthreads();
}

// this lane's row of head `hrow`'s weight (wqkv column hrow + l31), channels 16 s + 8 lh + j, in three pieces: the B fragments of
// K^T = xn^T Wk^T / the A fragments of Q = Wq xn
template <int C>
__device__ __forceinline__ void split_weight(const float* __restrict__ wqkv, int col, int lh, bf16x8 (&w)[3][C / 16]) {
#pragma unroll
    for (int s = 0; s < C / 16; ++s)
#pragma unroll
        for (int j = 0; j < 8; ++j) {       // (open-coded: through split3x8 and a staging array la_x3_out<128> compiles to other instructions)
            __bf16 h, m, l;
            split3(wqkv[(int64_t)(16 * s + 8 * lh + j) * (3 * HID) + col], h, m, l);
            w[0][s][j] = h; w[1][s][j] = m; w[2][s][j] = l;
        }
}

// 64 tokens x 32 rows of one head's projection in six terms, one accumulator per output.  XA: xn is the A operand (pass 1:
// acc[j][r] = K^T[tok = j*32 + row(r, lh)][d = l31]); otherwise the B operand (pass 2: acc[j][r] = Q[d = row(r, lh)][tok = j*32 + l31]).
// Either way the lane reads token j*32 + l31, channels 16 s + 8 lh .. + 8, of a piece image.
template <int C, bool XA, int NPRE>
__device__ __forceinline__ void project_x3(const bf16x8 (&w)[3][C / 16], const __bf16* __restrict__ xt, int l31, int lh, f32x16 (&acc)[2]) {
    constexpr int NKS = C / 16, CP8 = cpitch(C) / 8, PE8 = piece_e(C) / 8;
    // the six terms in sdc_split3.h's order: weight piece X3_PA[t] with xn piece X3_PB[t]
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc[0][r] = 0.f; acc[1][r] = 0.f; }
    const bf16x8* xp = reinterpret_cast<const bf16x8*>(xt) + l31 * CP8 + lh;
    // the fragments of the first NPRE pieces are read once into registers (piece 0 enters three terms, piece 1 two); the others are
    // read with their term -- as many as the kernel's registers allow without a spill
    bf16x8 xf[NPRE > 0 ? NPRE : 1][2][NKS];
#pragma unroll
    for (int p = 0; p < NPRE; ++p)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int s = 0; s < NKS; ++s) xf[p][j][s] = xp[p * PE8 + j * 32 * CP8 + 2 * s];
#pragma unroll
    for (int t = 0; t < 6; ++t) {
#pragma unroll
        for (int s = 0; s < NKS; ++s)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const bf16x8 xv = X3_PB[t] < NPRE ? xf[X3_PB[t] < NPRE ? X3_PB[t] : 0][j][s] : xp[X3_PB[t] * PE8 + j * 32 * CP8 + 2 * s];
                acc[j] = XA ? __builtin_amdgcn_mfma_f32_32x32x16_bf16(xv, w[X3_PA[t]][s], acc[j], 0, 0, 0)
                            : __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[X3_PA[t]][s], xv, acc[j], 0, 0, 0);
            }
        // (C = 64, two waves per SIMD: a term's fragment reads stay with the term -- hoisted, they spill; C = 128 has the registers)
        if (C == 64 && NPRE < 3) __builtin_amdgcn_sched_barrier(0);
    }
}

// ------------------------------------------------------------------ pass 1: la_blk_ctx with K^T from the split operands
template <int C, bool GN>
__global__ __launch_bounds__(NT, (C == 64 ? 2 : 1)) SDC_NO_DS_MERGE void la_x3_ctx(const LaArgs a) {
    constexpr int NCT = C / 32;                     // row tiles of M^T (channels)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_x3[];
    __bf16* const xt = reinterpret_cast<__bf16*>(smem_x3);             // [3][TT][C + 8]
    float* const xs = reinterpret_cast<float*>(xt + 3 * piece_e(C));    // [C][XP]
    float* const red = xs + C * XP;                 // [8][TT]
    float* const gcoef = red + 8 * TT;              // [2][C]  (GroupNorm-on-load form only)
    const int tid = threadIdx.x, lane = tid & 63, head = tid >> 6, l31 = lane & 31, lh = lane >> 5;
    const int split = blockIdx.x, seq = blockIdx.y;
    const int o = seq / a.inner, i = seq - o * a.inner;
    const float* xseq = a.x + o * a.so + i * a.si;
    const float* rseq = (GN && a.gn_res) ? a.gn_res + o * a.so + i * a.si : nullptr;
    if (GN) gn_coef_fill<C>(a.gn_stats, a.gn_gamma, a.gn_beta, a.gn_G, o, gcoef, tid);

    bf16x8 wk[3][C / 16];                           // Wk_h[d = l31][c = 16 s + 8 lh + j], three pieces
    split_weight<C>(a.wqkv, HID + head * 32 + l31, lh, wk);

    f32x16 macc[NCT];                               // M^T tile t: rows c = t*32 + crow, columns d = l31
#pragma unroll
    for (int t = 0; t < NCT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) macc[t][r] = 0.f;
    float mrun = -INFINITY, psum = 0.f;             // per d (this lane; the two half-waves hold different token rows)

    const int t0 = split * a.tiles_per_split;
    const int t1 = min(t0 + a.tiles_per_split, a.ntiles);
    float xv[C / 4];
    if (t0 < t1) fetch_tile<C>(xseq + (int64_t)t0 * TT, a.sc, tid, xv);
    if (GN) __syncthreads();                        // coefficient table complete
    for (int tile = t0; tile < t1; ++tile) {
        if (GN) {
            // h once, here: pass 2 reads it back from the block's own output buffer (la_blk_ctx)
            gn_apply_tile<C>(xv, rseq ? rseq + (int64_t)tile * TT : nullptr, a.sc, gcoef, tid);
            float* hb = a.gn_hout + o * a.so + i * a.si + (int64_t)tile * TT;
            constexpr int CG = C / 4;
            la_gptr hp = la_uni(hb + (int64_t)(__builtin_amdgcn_readfirstlane(tid >> 6) * CG) * a.sc);
            uint32_t hoff = (uint32_t)(tid & 63) * 4u;
#pragma unroll
            for (int k = 0; k < CG; ++k) {
                asm volatile("" : "+v"(hoff));
                la_st(hp, hoff, xv[k]);
                hp += a.sc;
                asm volatile("" : "+s"(hp));
            }
        }
        norm_tile_x3<C>(xv, a.g_pre, a.pre_mode, a.eps, xs, xt, nullptr, red, tid);
        if (tile + 1 < t1) fetch_tile<C>(xseq + (int64_t)(tile + 1) * TT, a.sc, tid, xv);
        // K^T tiles j = 0, 1: rows tok = j*32 + crow(r, lh), columns d = l31
        f32x16 kacc[2];
        project_x3<C, true, (C == 64 ? PRE_CTX64 : 0)>(wk, xt, l31, lh, kacc);
        // online softmax over tokens, per d (la_blk_ctx's)
        float tmax = kacc[0][0];
#pragma unroll
        for (int r = 0; r < 16; ++r) tmax = x3_max3(tmax, kacc[0][r], kacc[1][r]);
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
        const float mnew = fmaxf(mrun, tmax);
        const float f = __expf(mrun - mnew);
        mrun = mnew;
        float ps = 0.f;
        const float nml = -mnew * LOG2E;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            kacc[0][r] = __builtin_amdgcn_exp2f(fmaf(kacc[0][r], LOG2E, nml));
            kacc[1][r] = __builtin_amdgcn_exp2f(fmaf(kacc[1][r], LOG2E, nml));
            ps += kacc[0][r] + kacc[1][r];
        }
        psum = psum * f + ps;
        if (__builtin_amdgcn_ballot_w64(f != 1.0f)) {           // (wave-uniform: a multiplication by 1 is skipped)
#pragma unroll
            for (int t = 0; t < NCT; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) macc[t][r] *= f;
        }
        // M^T[c][d] += sum_tok xn[c][tok] p[tok][d] on the fp32 pipe; step (j, r) covers tokens j*32 + crow(r, 0) | crow(r, 1)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int tok = j * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
#pragma unroll
                for (int t = 0; t < NCT; ++t)
                    macc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(xs[(t * 32 + l31) * XP + tok], kacc[j][r], macc[t], 0, 0, 0);
            }
        __syncthreads();                             // xs / xt are rewritten by the next tile
    }
    // partial result of this split: M[32][C], m[32], s[32]
    float* pp = a.part + (((int64_t)seq * a.nsplit + split) * 4 + head) * (32 * (C + 2));
#pragma unroll
    for (int t = 0; t < NCT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) pp[l31 * C + t * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh] = macc[t][r];
    const float stot = psum + __shfl_xor(psum, 32, 64);
    if (lh == 0) { pp[32 * C + l31] = mrun; pp[32 * C + 32 + l31] = stot; }
}

// ------------------------------------------------------------------ pass 2: la_blk_out with Q from the split operands
template <int C>
__global__ __launch_bounds__(NT, (C == 64 ? 2 : 1)) SDC_NO_DS_MERGE void la_x3_out(const LaArgs a) {
    constexpr int NRT = C / 32;                     // row tiles of y (channels)
    constexpr int TPW = NRT / 2;                    // y tiles per wave (one row tile, TPW column tiles)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_x3[];
    __bf16* const xt = reinterpret_cast<__bf16*>(smem_x3);             // [3][TT][C + 8]
    float* const qs = reinterpret_cast<float*>(xt + 3 * piece_e(C));    // [128][XP]
    float* const red = qs + HID * XP;               // [8][TT]
    float* const xr = red + 8 * TT;                 // [C][XP] raw x tile (residual)
    float* const bg = xr + C * XP;                  // [2][C] bias | post gain
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lh = lane >> 5;
    const int seq = blockIdx.y;
    const int o = seq / a.inner, i = seq - o * a.inner;
    const float* xseq = a.x + o * a.so + i * a.si;
    float* yseq = a.y + o * a.so + i * a.si;
    const int rt = (NRT == 2) ? (wave & 1) : wave;  // this wave's row tile of y
    const int ct0 = (NRT == 2) ? (wave >> 1) : 0;   // its first column tile

    bf16x8 wq[3][C / 16];                           // Wq_h[d = l31][c = 16 s + 8 lh + j], head = wave, three pieces
    split_weight<C>(a.wqkv, wave * 32 + l31, lh, wq);
    float treg[HID / 2];                            // T[co = rt*32 + l31][hd = 2ks + lh]
    const float* tb = a.tt + (int64_t)seq * HID * C;
#pragma unroll
    for (int ks = 0; ks < HID / 2; ++ks) treg[ks] = tb[(2 * ks + lh) * C + rt * 32 + l31];
    for (int c = tid; c < C; c += NT) {
        bg[c] = a.bo ? a.bo[c] : 0.f;
        bg[C + c] = a.g_post ? a.g_post[c] : 1.f;
    }

    const int t0 = blockIdx.x * a.tiles_per_blk;
    const int t1 = min(t0 + a.tiles_per_blk, a.ntiles);
    float xv[C / 4];
    if (t0 < t1) fetch_tile<C>(xseq + (int64_t)t0 * TT, a.sc, tid, xv);
    for (int tile = t0; tile < t1; ++tile) {
        norm_tile_x3<C>(xv, a.g_pre, a.pre_mode, a.eps, nullptr, xt, xr, red, tid);
        if (tile + 1 < t1) fetch_tile<C>(xseq + (int64_t)(tile + 1) * TT, a.sc, tid, xv);
        f32x16 qacc[2];
        project_x3<C, false, (C == 64 ? PRE_OUT64 : 0)>(wq, xt, l31, lh, qacc);
        // softmax over d (the 32 rows of the head) per token, times dim_head^-0.5 (la_blk_out's)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            float m = fmaxf(qacc[j][0], qacc[j][1]);
#pragma unroll
            for (int r = 2; r < 16; r += 2) m = x3_max3(m, qacc[j][r], qacc[j][r + 1]);
            m = fmaxf(m, __shfl_xor(m, 32, 64));
            typedef float la_f2 __attribute__((ext_vector_type(2)));
            const float nml = -m * LOG2E;
            const la_f2 l2 = {LOG2E, LOG2E}, n2 = {nml, nml};
            la_f2 s2 = {0.f, 0.f};
#pragma unroll
            for (int r = 0; r < 16; r += 2) {
                const la_f2 e2 = la_f2{qacc[j][r], qacc[j][r + 1]} * l2 + n2;
                const la_f2 p2 = {__builtin_amdgcn_exp2f(e2.x), __builtin_amdgcn_exp2f(e2.y)};
                qacc[j][r] = p2.x; qacc[j][r + 1] = p2.y;
                s2 += p2;
            }
            float s = s2.x + s2.y;
            s += __shfl_xor(s, 32, 64);
            const float f = 0.17677669529663687f * __builtin_amdgcn_rcpf(s);
            const la_f2 f2 = {f, f};
#pragma unroll
            for (int r = 0; r < 16; r += 2) {
                const la_f2 o2 = la_f2{qacc[j][r], qacc[j][r + 1]} * f2;
                qs[(wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh) * XP + j * 32 + l31] = o2.x;
                qs[(wave * 32 + ((r + 1) & 3) + 8 * ((r + 1) >> 2) + 4 * lh) * XP + j * 32 + l31] = o2.y;
            }
        }
        __syncthreads();
        // y[co][tok] = sum_hd T[co][hd] q[hd][tok] on the fp32 pipe
        f32x16 yacc[TPW];
#pragma unroll
        for (int u = 0; u < TPW; ++u)
#pragma unroll
            for (int r = 0; r < 16; ++r) yacc[u][r] = bg[rt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh];
#pragma unroll
        for (int ks = 0; ks < HID / 2; ++ks)
#pragma unroll
            for (int u = 0; u < TPW; ++u)
                yacc[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(treg[ks], qs[(2 * ks + lh) * XP + (ct0 + u) * 32 + l31], yacc[u], 0, 0, 0);
        // channel norm over the C rows of each token column: 16 registers x 2 half-waves x NRT row tiles (waves)
        if (a.post_mode >= 0) {
            float st[TPW];
#pragma unroll
            for (int u = 0; u < TPW; ++u) {
                float s = 0.f;
                if (a.post_mode == 0) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) s += yacc[u][r];
                } else {
#pragma unroll
                    for (int r = 0; r < 16; ++r) s += yacc[u][r] * yacc[u][r];
                }
                s += __shfl_xor(s, 32, 64);
                if (lh == 0) red[rt * TT + (ct0 + u) * 32 + l31] = s;
            }
            __syncthreads();
#pragma unroll
            for (int u = 0; u < TPW; ++u) {
                float s = 0.f;
#pragma unroll
                for (int q = 0; q < NRT; ++q) s += red[q * TT + (ct0 + u) * 32 + l31];
                st[u] = s;
            }
            if (a.post_mode == 0) {
#pragma unroll
                for (int u = 0; u < TPW; ++u) {
                    typedef float la_f2 __attribute__((ext_vector_type(2)));
                    const float mean = st[u] * (1.0f / C);
                    const la_f2 m2 = {mean, mean};
                    la_f2 q2 = {0.f, 0.f};
#pragma unroll
                    for (int r = 0; r < 16; r += 2) {
                        const la_f2 d2 = la_f2{yacc[u][r], yacc[u][r + 1]} - m2;
                        yacc[u][r] = d2.x; yacc[u][r + 1] = d2.y;
                        q2 += d2 * d2;
                    }
                    float q = q2.x + q2.y;
                    q += __shfl_xor(q, 32, 64);
                    if (lh == 0) red[(4 + rt) * TT + (ct0 + u) * 32 + l31] = q;
                }
                __syncthreads();
#pragma unroll
                for (int u = 0; u < TPW; ++u) {
                    float q = 0.f;
#pragma unroll
                    for (int w = 0; w < NRT; ++w) q += red[(4 + w) * TT + (ct0 + u) * 32 + l31];
                    const float rstd = rsqrtf(q * (1.0f / C) + a.eps);
                    typedef float la_f2 __attribute__((ext_vector_type(2)));
                    const la_f2 r2 = {rstd, rstd};
#pragma unroll
                    for (int r = 0; r < 16; r += 2) {
                        const la_f2 o2 = la_f2{yacc[u][r], yacc[u][r + 1]} * r2 *
                                         la_f2{bg[C + rt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh], bg[C + rt * 32 + ((r + 1) & 3) + 8 * ((r + 1) >> 2) + 4 * lh]};
                        yacc[u][r] = o2.x; yacc[u][r + 1] = o2.y;
                    }
                }
            } else {
#pragma unroll
                for (int u = 0; u < TPW; ++u) {
                    const float f = sqrtf((float)C) / fmaxf(sqrtf(st[u]), 1e-12f);
#pragma unroll
                    for (int r = 0; r < 16; ++r) yacc[u][r] = yacc[u][r] * f * bg[C + rt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh];
                }
            }
        }
        // + x, store (tokens on lanes: coalesced rows; scalar row base + one lane offset, host check `4 sc` elements < 2^30)
#pragma unroll
        for (int u = 0; u < TPW; ++u) {
            const int col = (ct0 + u) * 32 + l31;
            uint32_t loff = (uint32_t)((int64_t)(4 * lh) * a.sc + col) * 4u;
            la_gptr yrow = la_uni(yseq + (int64_t)(rt * 32) * a.sc + (int64_t)tile * TT);
            const float* xrow = xr + (rt * 32 + 4 * lh) * XP + col;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                asm volatile("" : "+v"(loff));
                la_st(yrow, loff, yacc[u][r] + xrow[((r & 3) + 8 * (r >> 2)) * XP]);
                yrow += ((r & 3) == 3 ? 5 : 1) * a.sc;
                asm volatile("" : "+s"(yrow));
            }
        }
        __syncthreads();                             // xt / qs / red / xr are rewritten by the next tile
    }
}

size_t lds_ctx(int C) { return sizeof(__bf16) * (size_t)(3 * piece_e(C)) + sizeof(float) * (size_t)(C * XP + 8 * TT + 2 * C); }
size_t lds_out(int C) { return sizeof(__bf16) * (size_t)(3 * piece_e(C)) + sizeof(float) * (size_t)(HID * XP + 8 * TT + C * XP + 2 * C); }
static_assert((sizeof(__bf16) * 3 * piece_e(64)) % 16 == 0 && (sizeof(__bf16) * 3 * piece_e(128)) % 16 == 0, "the fp32 images start on 16 bytes");
// two workgroups of la_x3_out<64> share a CU's 160 KB
static_assert(2 * (sizeof(__bf16) * 3 * piece_e(64) + sizeof(float) * (HID * XP + 8 * TT + 64 * XP + 2 * 64)) <= 160 * 1024, "la_x3_out<64>: two per CU");

}  // namespace

namespace sdc {

int la_x3_launch_ctx(const LaArgs& a, int C, bool gn, dim3 grid, hipStream_t stream) {
    static std::atomic<uint64_t> attr0{0}, attr1{0};
    SDC_LDS_OPTIN(attr0, (la_x3_ctx<128, false>), 96 * 1024, "sdc_linattn_block");        // 87 KB; C = 64 stays below 64 KB
    SDC_LDS_OPTIN(attr1, (la_x3_ctx<128, true>), 96 * 1024, "sdc_linattn_block");
    const size_t ldsb = lds_ctx(C);
    if (C == 64) {
        if (gn) hipLaunchKernelGGL((la_x3_ctx<64, true>), grid, dim3(NT), ldsb, stream, a);
        else hipLaunchKernelGGL((la_x3_ctx<64, false>), grid, dim3(NT), ldsb, stream, a);
    } else {
        if (gn) hipLaunchKernelGGL((la_x3_ctx<128, true>), grid, dim3(NT), ldsb, stream, a);
        else hipLaunchKernelGGL((la_x3_ctx<128, false>), grid, dim3(NT), ldsb, stream, a);
    }
    return SDC_OK;
}

int la_x3_launch_out(const LaArgs& a, int C, dim3 grid, hipStream_t stream) {
    static std::atomic<uint64_t> attr0{0}, attr1{0};
    SDC_LDS_OPTIN(attr0, la_x3_out<64>, 96 * 1024, "sdc_linattn_block");                  // 78 KB
    SDC_LDS_OPTIN(attr1, la_x3_out<128>, 128 * 1024, "sdc_linattn_block");                // 119 KB
    const size_t ldsb = lds_out(C);
    if (C == 64) hipLaunchKernelGGL(la_x3_out<64>, grid, dim3(NT), ldsb, stream, a);
    else hipLaunchKernelGGL(la_x3_out<128>, grid, dim3(NT), ldsb, stream, a);
    return SDC_OK;
}

}  // namespace sdc

// The routing table of sdc_linattn_block / sdc_linattn_block_gn: the (C, tokens per sequence) at which every repeat
// of the split kernels measured faster than every repeat of the fp32 kernels on the same buffers, at the bench batch and at B = 2
// (profiles/linattn_x3_shapes.log): four of the five fused sites of the default C4 plan (width 64 at 64 x 64 and 32 x 32 pixels, width
// 128 at 32 x 32) and the C2 plan's 16 x 128 and 8 x 64 levels.  Per-sequence sizes only, never the batch; a size that was not measured
// is not listed, and (128, 256) -- x1.02 at the bench batch -- is left on the fp32 kernels.
extern "C" int sdc_linattn_block_x3_ok(int C, int64_t n) {
    return (C == 64 && (n == 4096 || n == 2048 || n == 1024)) || (C == 128 && (n == 1024 || n == 512));
}
