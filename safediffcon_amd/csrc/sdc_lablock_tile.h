// Tile helpers shared by the fused LinearAttention block kernels (sdc_lablock.hip: fp32 operands; sdc_lablock_f16.hip: fp16
// operands; sdc_lablock_x3.hip: bf16-split q / k projections): the kernel arguments, the tile geometry, the wave-uniform-base global
// accesses, the tile fetch and the GroupNorm-on-load arithmetic.
#pragma once
#include "sdc_common.h"

namespace sdc {

struct LaArgs {
    const float* x;
    const float* g_pre;
    const float* wqkv;      // packed [C][384]  (q | k | v, each heads*32)
    const float* wo;        // packed [128][C]
    const float* bo;        // [C] or null
    const float* g_post;    // [C] or null
    float* part;            // [nseq][nsplit][4][32*(C+2)]
    float* tt;              // [nseq][128][C]
    float* y;
    // GroupNorm + SiLU (+ residual) of the producing ResnetBlock applied on load (sdc_linattn_block_gn): x is then the RAW conv
    // output, gn_stats (mean, rstd) per (outer index, group), gn_res the residual branch (same strides as x) or null
    const float* gn_stats; const float* gn_gamma; const float* gn_beta; const float* gn_res;
    float* gn_hout;         // pass 1 stores h here (x's strides); pass 2 then reads it as its x
    int gn_G;
    int inner, nsplit, tiles_per_split, ntiles, tiles_per_blk;
    int pre_mode, post_mode;
    float eps;
    int64_t so, sc, si;
};

// passes 1 and 3 of the block with the q / k projections as three-way bf16 splits (sdc_lablock_x3.hip), launched by
// sdc_linattn_block_sel / sdc_linattn_block_gn_sel (sdc_lablock.hip) around la_blk_mid: the grids and arguments of la_blk_ctx / la_blk_out
int la_x3_launch_ctx(const LaArgs& a, int C, bool gn, dim3 grid, hipStream_t stream);
int la_x3_launch_out(const LaArgs& a, int C, dim3 grid, hipStream_t stream);
// pass 1 in fp32 (la_blk_ctx of sdc_lablock.hip, no GroupNorm on load) for the block's backward (sdc_lablock_bwd.hip), which re-runs
// it into its own workspace: grid = (a.nsplit, sequences)
int la_launch_ctx(const LaArgs& a, int C, dim3 grid, hipStream_t stream);

}  // namespace sdc

namespace {

using sdc::LaArgs;

constexpr int NT = 256;
constexpr int TT = 64;            // tokens per tile
constexpr int XP = TT + 1;        // LDS pitch of a token row (odd: conflict-free when lanes walk channels)
constexpr int HID = 128;
constexpr float LOG2E = 1.4426950408889634f;
typedef float f32x16 __attribute__((ext_vector_type(16)));

// wave-uniform base (SGPR pair) + one 32-bit per-lane byte offset: the channel row of an access is wave-uniform (a wave owns whole
// rows: grp = tid >> 6), only the token is per lane -- left to the compiler every access formed a 64-bit address per lane
// (17 v_lshl_add_u64 + 20-66 v_add_u32 per tile in these kernels, where a VALU instruction costs matrix-pipe time)
typedef __attribute__((address_space(1))) float* la_gptr;
typedef __attribute__((address_space(1))) char* la_gcptr;
__device__ __forceinline__ la_gptr la_uni(const float* p) {
    const uint64_t u = reinterpret_cast<uint64_t>(p);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)u), hi = __builtin_amdgcn_readfirstlane((uint32_t)(u >> 32));
    return (la_gptr)(((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ float la_ld(la_gptr base, uint32_t byte_off) { return *(la_gptr)((la_gcptr)base + byte_off); }
__device__ __forceinline__ void la_st(la_gptr base, uint32_t byte_off, float v) { *(la_gptr)((la_gcptr)base + byte_off) = v; }

// max(a, b, c) in one instruction (fmaxf(fmaxf()) came out as v_max_f32 pairs plus a canonicalising v_max x, x per input: 45 for 32)
__device__ __forceinline__ float la_max3(float a, float b, float c) { float r; asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }

template <int C>
__device__ __forceinline__ void fetch_tile(const float* __restrict__ xb, int64_t sc, int tid, float (&v)[C / 4]) {
    constexpr int CG = C / 4;
    const int tok = tid & 63, grp = __builtin_amdgcn_readfirstlane(tid >> 6);
    la_gptr rp = la_uni(xb + (int64_t)(grp * CG) * sc);
    // (the lane offset passes through an empty asm before every access: left alone its zero-extension is hoisted out of the loop as a
    // 64-bit register pair and every load forms its address with a v_lshl_add_u64 -- 16 per tile here -- instead of taking the
    // scalar base + 32-bit offset form)
    uint32_t off = (uint32_t)tok * 4u;
#pragma unroll
    for (int k = 0; k < CG; ++k) {
        asm volatile("" : "+v"(off));
        v[k] = la_ld(rp, off);
        rp += sc;
        asm volatile("" : "+s"(rp));
    }
}

// GroupNorm-on-load form (template GN; the producing ResnetBlock's second GroupNorm + SiLU + residual add, conv3d.py:189-230,
// never written to HBM): gn_apply_tile turns the raw conv tile into the block input h = SiLU(x * mul[c] + add[c]) + r with the
// same expressions as gn_apply_kernel (sdc_norm.hip), coefficients from LDS.
template <int C>
__device__ __forceinline__ void gn_apply_tile(float (&v)[C / 4], const float* __restrict__ rb, int64_t sc, const float* __restrict__ gcoef,
                                              int tid) {
    constexpr int CG = C / 4;
    const int tok = tid & 63, grp = tid >> 6;
    float rv[CG];                                   // the residual tile is requested first: it travels under the SiLUs
    if (rb) {
        la_gptr rp = la_uni(rb + (int64_t)(__builtin_amdgcn_readfirstlane(grp) * CG) * sc);
        uint32_t off = (uint32_t)tok * 4u;
#pragma unroll
        for (int k = 0; k < CG; ++k) {
            asm volatile("" : "+v"(off));
            rv[k] = la_ld(rp, off);
            rp += sc;
            asm volatile("" : "+s"(rp));
        }
    } else {
#pragma unroll
        for (int k = 0; k < CG; ++k) rv[k] = 0.f;
    }
#pragma unroll
    for (int k = 0; k < CG; ++k) {
        const float mul = gcoef[grp * CG + k], add = gcoef[C + grp * CG + k];
        v[k] = sdc::silu_f(v[k] * mul + add) + rv[k];
    }
}
// (mul, add) per channel of outer index o into LDS: mul = rstd * gamma, add = beta - mean * mul
template <int C>
__device__ __forceinline__ void gn_coef_fill(const float* __restrict__ stats, const float* __restrict__ gamma,
                                             const float* __restrict__ beta, int G, int o, float* __restrict__ gcoef, int tid) {
    for (int c = tid; c < C; c += NT) {
        const int g = c / (C / G);
        const float mean = stats[(o * G + g) * 2], rstd = stats[(o * G + g) * 2 + 1];
        const float mul = rstd * gamma[c];
        gcoef[c] = mul;
        gcoef[C + c] = beta[c] - mean * mul;
    }
}

// token splits of pass 1: a function of the sequence length only, so a trajectory's result does not depend on how
// many others share the launch (batch-invariant summation order)
inline int pick_nsplit(int64_t /*nseq*/, int ntiles) {
    int ns = ntiles / 8;
    if (ns > 8) ns = 8;
    return ns < 1 ? 1 : ns;
}

}  // namespace
