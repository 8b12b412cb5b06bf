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
//   - xn, once per value and tile, by the thread that normalises it (norm_tile_regs' expressions: xn has la_blk's bits): three bf16 images
//     [piece][token][C + 8] in LDS, a lane's K fragment (8 consecutive channels of one token) one 16-byte read; shared by the four heads.
// A product's five small terms are issued first, smallest kind first, each over all its K steps, then the main term: one accumulator per
// output.  The bf16 MFMA's accumulators have the fp32 one's register layout, so everything behind the projections is la_blk's code, on
// the fp32 pipe, in its order: the online softmax over tokens, the rescale, M^T += xn p (pass 1 keeps the fp32 xn image for it), the
// softmax over d, y = T q, the post norm, the residual, the stores.
// No atomics, fixed accumulation order, a sequence's arithmetic does not see the batch.  A non-finite x gives NaN (inf - inf in the
// residual of the split) where the fp32 kernels may give an infinity.
#include "sdc_common.h"
#include "sdc_lablock_pass.h"
#include "sdc_split3.h"

namespace {

__host__ __device__ constexpr int cpitch(int C) { return C + 8; }      // pitch (bf16) of one token of a piece image: C channels + 16 bytes
// xn pieces whose fragments a wave keeps in registers across the six terms at C = 64 (project_x3): pass 1 has room for all three,
// pass 2 (64 registers of T) for the first
constexpr int PRE_CTX64 = 3, PRE_OUT64 = 1;
__host__ __device__ constexpr int piece_e(int C) { return TT * cpitch(C); }      // bf16 elements of one piece image

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

// The bf16-split build of the pass bodies (sdc_lablock_pass.h): xn as three bf16 piece images xt[piece][tok][c] in front of the fp32
// images (pass 1 keeps the fp32 xs for its M product, pass 2 has none), weight fragments as three pieces.
struct LaX3 {
    template <int C> static constexpr size_t xt_bytes() { return sizeof(__bf16) * 3 * piece_e(C); }
    // byte offsets into the dynamic LDS: xt [3][TT][C + 8] bf16 first; pass 1 then has xs, pass 2 has none (XS < 0) and has qs there
    template <int C> struct Ctx {
        static_assert(xt_bytes<C>() % 16 == 0, "the fp32 images start on 16 bytes");
        static constexpr int XS = (int)xt_bytes<C>(), RED = XS + 4 * C * XP, GCOEF = RED + 4 * 8 * TT;
        static constexpr size_t BYTES = GCOEF + 4 * 2 * C;
    };
    template <int C> struct Out {
        static constexpr int XS = -1, QS = (int)xt_bytes<C>(), RED = QS + 4 * HID * XP, XR = RED + 4 * 8 * TT, BG = XR + 4 * C * XP;
        static constexpr size_t BYTES = BG + 4 * 2 * C;
    };
    // W_h[d = l31][c = 16 s + 8 lh + j], three pieces (a plain array, not a struct: DESIGN.md 22.1)
    template <int C> using W = bf16x8[3][C / 16];
    // this lane's row `col` of the packed wqkv, channels 16 s + 8 lh + j, split: the B fragments of K^T = xn^T Wk^T / the A fragments of
    // Q = Wq xn.  (The loop itself, not a call of a helper that holds it: DESIGN.md 22.1.)
    template <int C>
    static __device__ __forceinline__ void load_w(const float* __restrict__ wqkv, int col, int lh, bf16x8 (&w)[3][C / 16]) {
#pragma unroll
        for (int s = 0; s < C / 16; ++s)
#pragma unroll
            for (int j = 0; j < 8; ++j) {       // (open-coded: through split3x8 and a staging array la_x3_out<128> compiles to other instructions)
                __bf16 h, m, l;
                split3(wqkv[(int64_t)(16 * s + 8 * lh + j) * (3 * HID) + col], h, m, l);
                w[0][s][j] = h; w[1][s][j] = m; w[2][s][j] = l;
            }
    }
    // xn (norm_tile_regs' fp32 expressions: la_blk's bits) as fp32 xs[c][tok] where the pass has one, and as three bf16 pieces
    template <int C, class L>
    static __device__ __forceinline__ void norm(float (&v)[C / 4], const LaArgs& a, const L& l, float* __restrict__ xr, int tid) {
        constexpr int CG = C / 4, CP = cpitch(C);
        const int tok = tid & 63, grp = tid >> 6;
        float o[CG];
        norm_tile_regs<C>(v, a.g_pre, a.pre_mode, a.eps, xr, l.red, tid, o);
        if (l.xs) {
#pragma unroll
            for (int k = 0; k < CG; ++k) l.xs[(grp * CG + k) * XP + tok] = o[k];
        }
        bf16x8* xo = reinterpret_cast<bf16x8*>(reinterpret_cast<__bf16*>(l.base) + tok * CP + grp * CG);
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
    template <int C, bool XA, class L>
    static __device__ __forceinline__ void project(const W<C>& w, const L& l, int l31, int lh, f32x16 (&acc)[2]) {
        project_x3<C, XA, (C == 64 ? (XA ? PRE_CTX64 : PRE_OUT64) : 0)>(w, reinterpret_cast<const __bf16*>(l.base), l31, lh, acc);
    }
    // max(a, b, c) in plain C++, not la_max3's inline v_max3_f32: behind an asm statement the compiler does not place the wait states a VALU
    // read of a bf16 MFMA's fresh accumulator needs (the first maximum reads one), and the stale register showed as run-to-run differences
    // in the last bits at full size (DESIGN.md section 19 met the same with a packed asm pair).  The maximum itself is exact either way.
    static __device__ __forceinline__ float max3(float a, float b, float c) { return fmaxf(fmaxf(a, b), c); }
};

// pass 1: la_blk_ctx with K^T from the split operands
template <int C, bool GN>
__global__ __launch_bounds__(NT, (C == 64 ? 2 : 1)) SDC_NO_DS_MERGE void la_x3_ctx(const LaArgs a) { la_ctx_body<C, GN, LaX3>(a); }
// pass 2: la_blk_out with Q from the split operands
template <int C>
__global__ __launch_bounds__(NT, (C == 64 ? 2 : 1)) SDC_NO_DS_MERGE void la_x3_out(const LaArgs a) { la_out_body<C, LaX3>(a); }

}  // namespace

namespace sdc {

int la_x3_launch_ctx(const LaArgs& a, int C, bool gn, dim3 grid, hipStream_t stream) {
    static std::atomic<uint64_t> attr0{0}, attr1{0};
    SDC_LDS_OPTIN(attr0, (la_x3_ctx<128, false>), 96 * 1024, "sdc_linattn_block");        // 87 KB; C = 64 stays below 64 KB
    SDC_LDS_OPTIN(attr1, (la_x3_ctx<128, true>), 96 * 1024, "sdc_linattn_block");
    const size_t ldsb = la_ctx_bytes<LaX3>(C);
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
    const size_t ldsb = la_out_bytes<LaX3>(C);
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
