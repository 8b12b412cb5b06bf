// One body per pass for the two builds of the fused LinearAttention block whose M and y products are fp32 MFMAs: sdc_lablock.hip (every
// product on the fp32 pipe) and sdc_lablock_x3.hip (the q / k projections as bf16 splits).  A build is a policy struct P holding only
// what differs:
//   P::Ctx<C>, P::Out<C>    the LDS carve-up of pass 1 / pass 2 as byte offsets (XS, RED, GCOEF / XS, QS, RED, XR, BG; XS < 0: no fp32 xn
//                           image) and its byte count (BYTES: the launches' dynamic LDS comes from here)
//   P::W<C>                 one head's weight fragments, filled before the tile loop by
//   P::load_w<C>(wqkv, col, lh, w)             this lane's row `col` of the packed wqkv
//   P::norm<C>(v, a, L, xr, tid)               the channel norm of a tile, left in L as the build's projection (and pass 1's M
//                                              product, from the fp32 image L.xs) reads it; ends with the barrier
//   P::project<C, XA>(w, L, l31, lh, acc)      the 64 tokens x 32 rows of one head: XA, xn is the A operand (pass 1: K^T, rows =
//                                              tokens); otherwise the B operand (pass 2: Q, columns = tokens)
//   P::max3(a, b, c)        the three-way maximum that first reads the projection's accumulators
// Everything else -- the order of the steps, the products behind the projections, the stores -- is written here once.
#pragma once
#include "sdc_lablock_tile.h"

namespace {

// the LDS of a pass as the policies' norm / project see it: base = the start of the dynamic LDS (the bf16-split build's piece images)
struct LaCtxLds { unsigned char* base; float *xs, *red, *gcoef; };           // [C][XP] | [8][TT] | [2][C] (GroupNorm-on-load form only)
struct LaOutLds { unsigned char* base; float *xs, *qs, *red, *xr, *bg; };    // [C][XP] or none | [128][XP] | [8][TT] | [C][XP] raw x tile | [2][C] bias, post gain

// ------------------------------------------------------------------ pass 1: per (split, sequence); wave = head
// Everything is kept transposed so that the reductions run over registers and the products chain without LDS:
//   K^T[tok][d] = xn^T Wk^T        (operands swapped: rows = tokens on registers, columns = d on lanes)
//   softmax statistics per d       = per lane: max / sum over the 32 accumulator registers + one cross-half shuffle
//   M^T[c][d] += sum_tok xn[c][tok] p[tok][d]:  A = xn from LDS, B = the P registers as they stand (the contraction
//   index tok is walked in accumulator-row order); the online rescale factor is per d = per lane, one multiply per register.
template <int C, bool GN, class P>
__device__ __forceinline__ void la_ctx_body(const LaArgs& a) {
    constexpr int NCT = C / 32;                     // row tiles of M^T (channels)
    typedef typename P::template Ctx<C> Lds;
    static_assert(C != 64 || 2 * Lds::BYTES <= 160 * 1024, "pass 1 at C = 64: two workgroups share a CU's 160 KB");
    extern __shared__ __attribute__((aligned(16))) unsigned char la_smem[];
    // (brace-initialised here with the casts written out, and xs kept as a local: shapes the width-128 bf16-split kernels' speed
    // depends on; the same in pass 2)
    const LaCtxLds L = {la_smem, reinterpret_cast<float*>(la_smem + Lds::XS), reinterpret_cast<float*>(la_smem + Lds::RED), reinterpret_cast<float*>(la_smem + Lds::GCOEF)};
    float* const xs = L.xs;
    const int tid = threadIdx.x, lane = tid & 63, head = tid >> 6, l31 = lane & 31, lh = lane >> 5;
    const int split = blockIdx.x, seq = blockIdx.y;
    const int o = seq / a.inner, i = seq - o * a.inner;
    const float* xseq = a.x + o * a.so + i * a.si;
    const float* rseq = (GN && a.gn_res) ? a.gn_res + o * a.so + i * a.si : nullptr;
    if (GN) gn_coef_fill<C>(a.gn_stats, a.gn_gamma, a.gn_beta, a.gn_G, o, L.gcoef, tid);

    typename P::template W<C> wk;                   // Wk_h[d = l31][c]
    P::template load_w<C>(a.wqkv, HID + head * 32 + l31, lh, wk);

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
            gn_apply_tile<C>(xv, rseq ? rseq + (int64_t)tile * TT : nullptr, a.sc, L.gcoef, tid);
            gn_store_h<C>(a.gn_hout + o * a.so + i * a.si + (int64_t)tile * TT, a.sc, tid, xv);
        }
        P::template norm<C>(xv, a, L, nullptr, tid);
        if (tile + 1 < t1) fetch_tile<C>(xseq + (int64_t)(tile + 1) * TT, a.sc, tid, xv);
        // K^T tiles j = 0, 1: rows tok = j*32 + crow(r, lh), columns d = l31
        f32x16 kacc[2];
        P::template project<C, true>(wk, L, l31, lh, kacc);
        const float f = la_softmax_tok<P::max3>(kacc, mrun, psum);
        la_rescale<NCT>(macc, f);
        // M^T[c][d] += sum_tok xn[c][tok] p[tok][d] on the fp32 pipe; step (j, r) covers tokens j*32 + crow(r, 0) | crow(r, 1)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int tok = j * 32 + crow(r, lh);
#pragma unroll
                for (int t = 0; t < NCT; ++t)
                    macc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(xs[(t * 32 + l31) * XP + tok], kacc[j][r], macc[t], 0, 0, 0);
            }
        __syncthreads();                             // the xn images are rewritten by the next tile
    }
    la_store_partial<C>(a.part + (((int64_t)seq * a.nsplit + split) * 4 + head) * (32 * (C + 2)), macc, mrun, psum, l31, lh);
}

// ------------------------------------------------------------------ pass 2: per (tile group, sequence); wave = head for Q
template <int C, class P>
__device__ __forceinline__ void la_out_body(const LaArgs& a) {
    constexpr int NRT = C / 32;                     // row tiles of y (channels)
    constexpr int TPW = NRT / 2;                    // y tiles per wave (one row tile, TPW column tiles)
    typedef typename P::template Out<C> Lds;
    static_assert(C != 64 || 2 * Lds::BYTES <= 160 * 1024, "pass 2 at C = 64: two workgroups share a CU's 160 KB");
    extern __shared__ __attribute__((aligned(16))) unsigned char la_smem[];
    const LaOutLds L = {la_smem, Lds::XS < 0 ? nullptr : reinterpret_cast<float*>(la_smem + (Lds::XS < 0 ? 0 : Lds::XS)), reinterpret_cast<float*>(la_smem + Lds::QS),
                        reinterpret_cast<float*>(la_smem + Lds::RED), reinterpret_cast<float*>(la_smem + Lds::XR), reinterpret_cast<float*>(la_smem + Lds::BG)};
    float* const qs = L.qs; float* const red = L.red; float* const xr = L.xr; float* const bg = L.bg;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lh = lane >> 5;
    const int seq = blockIdx.y;
    const int o = seq / a.inner, i = seq - o * a.inner;
    const float* xseq = a.x + o * a.so + i * a.si;
    float* yseq = a.y + o * a.so + i * a.si;
    const int rt = (NRT == 2) ? (wave & 1) : wave;  // this wave's row tile of y
    const int ct0 = (NRT == 2) ? (wave >> 1) : 0;   // its first column tile

    typename P::template W<C> wq;                   // Wq_h[d = l31][c], head = wave
    P::template load_w<C>(a.wqkv, wave * 32 + l31, lh, wq);
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
        P::template norm<C>(xv, a, L, xr, tid);
        if (tile + 1 < t1) fetch_tile<C>(xseq + (int64_t)(tile + 1) * TT, a.sc, tid, xv);
        f32x16 qacc[2];
        P::template project<C, false>(wq, L, l31, lh, qacc);
        // softmax over d (the 32 rows of the head) per token, times dim_head^-0.5
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            typedef float la_f2 __attribute__((ext_vector_type(2)));
            const float f = la_softmax_d<P::max3>(qacc[j]);
            const la_f2 f2 = {f, f};
#pragma unroll
            for (int r = 0; r < 16; r += 2) {
                const la_f2 o2 = la_f2{qacc[j][r], qacc[j][r + 1]} * f2;
                qs[(wave * 32 + crow(r, lh)) * XP + j * 32 + l31] = o2.x;
                qs[(wave * 32 + crow(r + 1, lh)) * XP + j * 32 + l31] = o2.y;
            }
        }
        __syncthreads();
        // y[co][tok] = sum_hd T[co][hd] q[hd][tok] on the fp32 pipe
        f32x16 yacc[TPW];
#pragma unroll
        for (int u = 0; u < TPW; ++u)
#pragma unroll
            for (int r = 0; r < 16; ++r) yacc[u][r] = bg[rt * 32 + crow(r, lh)];
#pragma unroll
        for (int ks = 0; ks < HID / 2; ++ks)
#pragma unroll
            for (int u = 0; u < TPW; ++u)
                yacc[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(treg[ks], qs[(2 * ks + lh) * XP + (ct0 + u) * 32 + l31], yacc[u], 0, 0, 0);
        if (a.post_mode >= 0) la_post_norm<C, true>(yacc, a.post_mode, a.eps, bg, red, rt, ct0, l31, lh);
        la_store_residual<C>(yacc, yseq + (int64_t)tile * TT, a.sc, xr, rt, ct0, l31, lh);
        __syncthreads();                             // the xn images / qs / red / xr are rewritten by the next tile
    }
}

// dynamic LDS of a pass at a runtime width
template <class P> size_t la_ctx_bytes(int C) { return C == 64 ? P::template Ctx<64>::BYTES : P::template Ctx<128>::BYTES; }
template <class P> size_t la_out_bytes(int C) { return C == 64 ? P::template Out<64>::BYTES : P::template Out<128>::BYTES; }

}  // namespace
