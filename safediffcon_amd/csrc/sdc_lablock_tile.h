// What the three builds of the fused LinearAttention block share (sdc_lablock.hip: fp32 operands; sdc_lablock_f16.hip: fp16 operands;
// sdc_lablock_x3.hip: bf16-split q / k projections): the kernel arguments, the tile geometry, the wave-uniform-base global accesses, the
// tile fetch, the GroupNorm-on-load arithmetic, the steps of the two passes that touch no matrix operand (the channel norm into
// registers, the online softmax over tokens, the softmax over d, the post norm, the residual store) and the host set-up.  The pass
// bodies of the fp32 and bf16-split builds are in sdc_lablock_pass.h.
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

// pass 1 of the GroupNorm-on-load form stores h once (pass 2 reads it back from the block's own output buffer, tile by tile in place,
// instead of paying the SiLUs a second time -- measured with both passes normalising on load: +4.4 ms in these kernels for 3.5 ms of
// sdc_gn_apply saved at C4): hb = this tile's first token of channel 0
template <int C>
__device__ __forceinline__ void gn_store_h(float* hb, int64_t sc, int tid, const float (&v)[C / 4]) {
    constexpr int CG = C / 4;
    la_gptr hp = la_uni(hb + (int64_t)(__builtin_amdgcn_readfirstlane(tid >> 6) * CG) * sc);
    uint32_t hoff = (uint32_t)(tid & 63) * 4u;
#pragma unroll
    for (int k = 0; k < CG; ++k) {
        asm volatile("" : "+v"(hoff));
        la_st(hp, hoff, v[k]);
        hp += sc;
        asm volatile("" : "+s"(hp));
    }
}

// accumulator register r of half-wave lh -> row of a 32 x 32 MFMA result tile
__host__ __device__ __forceinline__ int crow(int r, int lh) { return (r & 3) + 8 * (r >> 2) + 4 * lh; }

// Channel norm over C per token of a tile (C channels x 64 tokens), into registers.  Thread (tok = tid & 63, group = tid >> 6) owns C/4
// channels of one token; the per-token statistics are combined across the 4 groups through `red` (two barriers for mode 0, one for
// mode 1).  mode 0: (x - mean) * rsqrt(var + eps) * g (two-pass variance); mode 1: x / max(||x||, 1e-12) * g * sqrt(C).
// fetch_tile only issues the loads (the next tile's are issued while the current one is on the matrix cores); this consumes them (v is
// left centred); `xr`, when given, keeps the raw tile for the residual add.  How o is left in LDS, and the barrier behind that, is the
// build's (fp32 xs; xs + three bf16 pieces; fp16 xt / xc).
template <int C>
__device__ __forceinline__ void norm_tile_regs(float (&v)[C / 4], const float* __restrict__ g, int mode, float eps, float* __restrict__ xr,
                                               float* __restrict__ red, int tid, float (&o)[C / 4]) {
    constexpr int CG = C / 4;
    const int tok = tid & 63, grp = tid >> 6;
    if (xr) {
#pragma unroll
        for (int k = 0; k < CG; ++k) xr[(grp * CG + k) * XP + tok] = v[k];
    }
    // the element-wise chains run on register pairs (v_pk_add / v_pk_fma / v_pk_mul: half the instructions; CG is even)
    typedef float la_f2 __attribute__((ext_vector_type(2)));
    la_f2 s2 = {0.f, 0.f};
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
}

// One online-softmax step over tokens of pass 1, per d = per lane (the two half-waves hold different token rows): the two K^T
// accumulators (rows tok = j*32 + crow(r, lh), columns d = l31) become the un-normalised probabilities exp(k - m) in place, m the new
// running maximum; returns the factor exp(m_old - m) that the running sum has taken and the running accumulators are to take.
// MAX3 is the build's three-way maximum: it is the first VALU read of the accumulators the last two MFMAs have written.
// (la16_ctx keeps a step of its own: its reference is the integer exponent ceil(m log2e) and its factor an exact power of two.)
template <float (*MAX3)(float, float, float)>
__device__ __forceinline__ float la_softmax_tok(f32x16 (&kacc)[2], float& mrun, float& psum) {
    float tmax = kacc[0][0];
#pragma unroll
    for (int r = 0; r < 16; ++r) tmax = MAX3(tmax, kacc[0][r], kacc[1][r]);
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
    const float mnew = fmaxf(mrun, tmax);
    const float f = __expf(mrun - mnew);
    mrun = mnew;
    float ps = 0.f;
    // exp(k - m) as exp2(k log2e - m log2e): one multiply-add in front of the v_exp instead of a subtraction and a multiplication
    const float nml = -mnew * LOG2E;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        kacc[0][r] = __builtin_amdgcn_exp2f(fmaf(kacc[0][r], LOG2E, nml));
        kacc[1][r] = __builtin_amdgcn_exp2f(fmaf(kacc[1][r], LOG2E, nml));
        ps += kacc[0][r] + kacc[1][r];
    }
    psum = psum * f + ps;
    return f;
}

// the running maximum settles after a few tiles: when no lane's moved, f is exactly 1 everywhere and the rescaling of the NCT x 16
// accumulator registers (a multiplication by 1: the same bits) is skipped -- a wave-uniform branch
template <int NCT>
__device__ __forceinline__ void la_rescale(f32x16 (&macc)[NCT], float f) {
    if (__builtin_amdgcn_ballot_w64(f != 1.0f)) {
#pragma unroll
        for (int t = 0; t < NCT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) macc[t][r] *= f;
    }
}

// partial result of a split and head of pass 1: M[32][C] (M^T tile t: rows c = t*32 + crow, columns d = l31), m[32], s[32]
template <int C>
__device__ __forceinline__ void la_store_partial(float* pp, const f32x16 (&macc)[C / 32], float mrun, float psum, int l31, int lh) {
#pragma unroll
    for (int t = 0; t < C / 32; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) pp[l31 * C + t * 32 + crow(r, lh)] = macc[t][r];
    const float stot = psum + __shfl_xor(psum, 32, 64);
    if (lh == 0) { pp[32 * C + l31] = mrun; pp[32 * C + 32 + l31] = stot; }
}

// Softmax over d (the 32 rows of the head: 16 registers x 2 half-waves) of pass 2, per token = per lane: leaves the un-normalised
// probabilities in q and returns f = dim_head^-0.5 / sum.  MAX3 as above; the first maximum is a plain fmaxf in every build.
template <float (*MAX3)(float, float, float)>
__device__ __forceinline__ float la_softmax_d(f32x16& q) {
    float m = fmaxf(q[0], q[1]);
#pragma unroll
    for (int r = 2; r < 16; r += 2) m = MAX3(m, q[r], q[r + 1]);
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    typedef float la_f2 __attribute__((ext_vector_type(2)));
    const float nml = -m * LOG2E;
    const la_f2 l2 = {LOG2E, LOG2E}, n2 = {nml, nml};
    la_f2 s2 = {0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 16; r += 2) {              // (register pairs: packed multiply-add in front of the two v_exp, packed sum)
        const la_f2 e2 = la_f2{q[r], q[r + 1]} * l2 + n2;
        const la_f2 p2 = {__builtin_amdgcn_exp2f(e2.x), __builtin_amdgcn_exp2f(e2.y)};
        q[r] = p2.x; q[r + 1] = p2.y;
        s2 += p2;
    }
    float s = s2.x + s2.y;
    s += __shfl_xor(s, 32, 64);
    return 0.17677669529663687f * __builtin_amdgcn_rcpf(s);      // (reciprocal instruction: the IEEE division is ten more)
}

// Post norm of pass 2 (post_mode 0 LayerNorm, 1 RMSNorm; both barriers are taken by the whole workgroup: post_mode is uniform) over the
// C rows of each token column of y: 16 registers x 2 half-waves x NRT row tiles (waves), combined through `red`.  yacc[u]: rows
// rt*32 + crow(r, lh), column (ct0 + u)*32 + l31; bg[C ..] the gain.  PACKED: LayerNorm's centring and its sum of squares on register
// pairs (even | odd registers summed apart); the scalar form sums the registers in order -- the fp16 build's bits.
template <int C, bool PACKED>
__device__ __forceinline__ void la_post_norm(f32x16 (&yacc)[C / 64], int post_mode, float eps, const float* __restrict__ bg,
                                             float* __restrict__ red, int rt, int ct0, int l31, int lh) {
    constexpr int NRT = C / 32, TPW = NRT / 2;
    typedef float la_f2 __attribute__((ext_vector_type(2)));
    float st[TPW];
#pragma unroll
    for (int u = 0; u < TPW; ++u) {
        float s = 0.f;
        if (post_mode == 0) {                       // (uniform branch: a per-element select computed both forms, 16 v_cndmask per tile)
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
    if (post_mode == 0) {
#pragma unroll
        for (int u = 0; u < TPW; ++u) {
            const float mean = st[u] * (1.0f / C);
            float q;
            if (PACKED) {
                const la_f2 m2 = {mean, mean};
                la_f2 q2 = {0.f, 0.f};
#pragma unroll
                for (int r = 0; r < 16; r += 2) {
                    const la_f2 d2 = la_f2{yacc[u][r], yacc[u][r + 1]} - m2;
                    yacc[u][r] = d2.x; yacc[u][r + 1] = d2.y;
                    q2 += d2 * d2;
                }
                q = q2.x + q2.y;
            } else {
                // (contraction off: every difference and every square is rounded, and the squares are added in register order --
                // what the fp16 build's kernels have always computed; left to the compiler, how many of the 16 steps become fused
                // multiply-adds changes with the code around them, and with it the last bits)
#pragma clang fp contract(off)
                q = 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) { yacc[u][r] -= mean; q += yacc[u][r] * yacc[u][r]; }
            }
            q += __shfl_xor(q, 32, 64);
            if (lh == 0) red[(4 + rt) * TT + (ct0 + u) * 32 + l31] = q;
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < TPW; ++u) {
            float q = 0.f;
#pragma unroll
            for (int w = 0; w < NRT; ++w) q += red[(4 + w) * TT + (ct0 + u) * 32 + l31];
            const float rstd = rsqrtf(q * (1.0f / C) + eps);
            if (PACKED) {
                const la_f2 r2 = {rstd, rstd};
#pragma unroll
                for (int r = 0; r < 16; r += 2) {
                    const la_f2 o2 = la_f2{yacc[u][r], yacc[u][r + 1]} * r2 * la_f2{bg[C + rt * 32 + crow(r, lh)], bg[C + rt * 32 + crow(r + 1, lh)]};
                    yacc[u][r] = o2.x; yacc[u][r + 1] = o2.y;
                }
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) yacc[u][r] = yacc[u][r] * rstd * bg[C + rt * 32 + crow(r, lh)];
            }
        }
    } else {
#pragma unroll
        for (int u = 0; u < TPW; ++u) {
            const float f = sqrtf((float)C) / fmaxf(sqrtf(st[u]), 1e-12f);
#pragma unroll
            for (int r = 0; r < 16; ++r) yacc[u][r] = yacc[u][r] * f * bg[C + rt * 32 + crow(r, lh)];
        }
    }
}

// y + x, stored (tokens on lanes: coalesced rows).  Rows co = rt*32 + crow(r, 0) from a scalar base, the half-wave's 4 rows and the
// column as one lane offset (host check `4 sc` elements < 2^30).  The scalar row base runs: rows crow(r, 0) are +1, +1, +1, +5 channel
// strides apart (formed per row from (cob, tile) the base cost ~6 scalar instructions per store, 190 per tile at width 64 -- a wave
// issues one instruction per four cycles whatever its kind).  ytile = this tile's first token of channel 0; xr the raw x tile.
template <int C>
__device__ __forceinline__ void la_store_residual(const f32x16 (&yacc)[C / 64], float* ytile, int64_t sc, const float* __restrict__ xr,
                                                  int rt, int ct0, int l31, int lh) {
#pragma unroll
    for (int u = 0; u < C / 64; ++u) {
        const int col = (ct0 + u) * 32 + l31;
        uint32_t loff = (uint32_t)((int64_t)(4 * lh) * sc + col) * 4u;
        la_gptr yrow = la_uni(ytile + (int64_t)(rt * 32) * sc);
        const float* xrow = xr + (rt * 32 + 4 * lh) * XP + col;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            asm volatile("" : "+v"(loff));
            la_st(yrow, loff, yacc[u][r] + xrow[crow(r, 0) * XP]);
            yrow += ((r & 3) == 3 ? 5 : 1) * sc;
            asm volatile("" : "+s"(yrow));
        }
    }
}

// token splits of pass 1: a function of the sequence length only, so a trajectory's result does not depend on how
// many others share the launch (batch-invariant summation order)
inline int pick_nsplit(int64_t /*nseq*/, int ntiles) {
    int ns = ntiles / 8;
    if (ns > 8) ns = 8;
    return ns < 1 ? 1 : ns;
}

// floats of the pass-1 partials at the head of the work buffer, as the *_bytes entry points promise them: sized for pick_nsplit's
// split count before the "no empty splits" clamp (a multiple of 16 bytes); T follows
inline size_t la_part_floats(int64_t nseq, int C, int64_t n) { return (size_t)(nseq * pick_nsplit(nseq, (int)(n / TT)) * 4 * 32 * (C + 2)); }

struct LaGrids { dim3 ctx, mid, out; };

// The host set-up of every build (A = LaArgs, or the fp16 build's argument struct with the same fields): the argument checks behind the
// caller's own null-pointer check, the split geometry, the partials at the head of `work` (*tt_at = where T goes) and the three grids.
// a.wqkv / a.wo, the packed weights and a.tt are the caller's.
template <class A>
inline int la_host_setup(const char* who, A& a, const float* x, const float* gn_stats, const float* gn_gamma, const float* gn_beta, int gn_G,
                         const float* gn_res, const float* g_pre, const float* bo, const float* g_post, void* work, float* y, int outer,
                         int inner, int C, int64_t n, int64_t so, int64_t sc, int64_t si, int pre_mode, int post_mode, float eps,
                         LaGrids& g, float** tt_at) {
    SDC_REQUIRE(C == 64 || C == 128, SDC_EINVAL, "%s: dim must be 64 or 128 (got %d)", who, C);
    SDC_REQUIRE(outer > 0 && inner > 0 && n > 0 && n % TT == 0, SDC_EINVAL, "%s: tokens must be a multiple of 64", who);
    SDC_REQUIRE((pre_mode == 0 || pre_mode == 1) && post_mode >= -1 && post_mode <= 1, SDC_EINVAL, "%s: bad norm mode", who);
    SDC_REQUIRE(post_mode < 0 || g_post, SDC_ENULL, "%s: post norm needs its gain", who);
    const int64_t nseq = (int64_t)outer * inner;
    SDC_REQUIRE(nseq < 65536, SDC_EINVAL, "%s: outer*inner must be < 65536", who);
    SDC_REQUIRE(sc > 0 && sc < (1ll << 27), SDC_EINVAL, "%s: channel stride must stay below 2^27 elements (32-bit lane offsets)", who);
    a.x = x; a.g_pre = g_pre; a.bo = bo; a.g_post = g_post; a.y = y;
    a.gn_stats = gn_stats; a.gn_gamma = gn_gamma; a.gn_beta = gn_beta; a.gn_res = gn_res; a.gn_G = gn_G; a.gn_hout = nullptr;
    a.inner = inner; a.ntiles = (int)(n / TT);
    const int ns0 = pick_nsplit(nseq, a.ntiles);
    a.tiles_per_split = (a.ntiles + ns0 - 1) / ns0;
    a.nsplit = (a.ntiles + a.tiles_per_split - 1) / a.tiles_per_split;     // no empty splits
    a.part = reinterpret_cast<float*>(work);
    *tt_at = a.part + la_part_floats(nseq, C, n);
    const int tpb = (int)((nseq * a.ntiles + 1023) / 1024);
    a.tiles_per_blk = tpb < 1 ? 1 : (tpb > 8 ? 8 : tpb);
    a.pre_mode = pre_mode; a.post_mode = post_mode; a.eps = eps;
    a.so = so; a.sc = sc; a.si = si;
    g.ctx = dim3((unsigned)a.nsplit, (unsigned)nseq);
    g.mid = dim3(4, (unsigned)nseq);
    g.out = dim3((unsigned)((a.ntiles + a.tiles_per_blk - 1) / a.tiles_per_blk), (unsigned)nseq);
    return SDC_OK;
}

}  // namespace
