// net.wino_split: the 3x3x3 stride-1 convs over rows of 16 as Winograd F(2x2x2,3x3x3) -- conv_wg3_kernel's algorithm (sdc_conv_wino.hip) --
// with the Cin products on v_mfma_f32_32x32x16_bf16 from EXACT three-way bf16 operand splits: the arithmetic of conv_stem_x3_kernel and
// conv_gemm_x3_kernel.  fp32 inputs, fp32 accumulation, fp32 outputs; x = h + m + l with h = bf16(x), m = bf16(x - h), l = bf16(x - h - m)
// (RNE, contraction off); six MFMAs per product, smallest terms first -- a3 b1, a2 b2, a1 b3, a2 b1, a1 b2, a1 b1 -- into ONE accumulator
// per tile (accumulators of their own for the five small terms, as in the stem kernel, would need 512 registers beside the 256 here).
// The operand that is split is the transformed one: V = B^T d B is formed in fp32 with conv_wg3_kernel's operations (the same bits) and
// split when it is parked; U is the conv's U3[jd][ci][co][j*4+xi] (formed in fp64, rounded once), split at pack time.
//
// Taken from conv_wg3_kernel as it stands: workgroup = 64 Cout x 64 tiles x one plane pair, 4 waves of 32 Cout x 32 tiles x 16 (j, xi)
// components in 256 accumulator registers (the 32x32 accumulator layout is the same for the fp32 and the bf16 instruction); the four
// depth passes in the order m1, m2, m0, m3 with the depth combination on load; the folds into the plane pair (y is scratch while the
// kernel runs: m1 is parked in plane 1); the bias as start value of component (1, 1) of the first pass; the GroupNorm partial sums from
// the finished values (fp64 from 16-element fp32 partials, fixed order; sdc_conv_gn's contract); the second, channel-concatenated input;
// stores through the descriptor's strides; xcd_tile.
//
// Staging: a K stage is 16 input channels, cut by transformed row j into four sub-stages of 4 components: 24 KB of U and 24 KB of V,
// double-buffered (96 KB), one barrier and 24 MFMAs per wave and sub-stage.
//   V image [piece][xi][tile][16 ci] bf16, 32 bytes per row: the 64 lanes of a ds_read_b128 fragment read walk 1 KB.  A thread owns the
//     four channels 4 wave .. 4 wave + 3 of one tile (the lane <-> tile map of conv_wg3_kernel<16>: the neighbour columns of the W
//     transform come through DPP row shifts) and parks with 8-byte writes, three per component.
//   U image [piece][xi][co][16 ci]: the packed buffer Wb[piece][co / 64][jd][stage][j][xi][co % 64][ci % 16] makes a sub-stage one
//     contiguous run of 8 KB per piece; six 16-byte loads per thread, parked as they are (the packer swaps the two channel octets
//     of rows 8-15 of every 16, as the V park does: conflict-free fragment reads).
//   While sub-stage q computes, sub-stage q + 1 is transformed, split and parked in the other buffer, the weight runs of q + 2 and q + 3 and the raw
//   rows of the next stage are in flight.
// Every stage runs for every tile, fixed k order, no K split, no atomics; clipped planes and rows enter with a factor 0 (exact zeros): a
// sample's bits do not depend on its batch or its tile mates.  A non-finite input gives NaN where the fp32 kernel gives +-inf (inf - inf
// in the split residuals, 0 * inf in a clipped plane).
#include "sdc_conv.h"
#include "sdc_split3.h"

using namespace sdcconv;

namespace {

typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef float w2f2 __attribute__((ext_vector_type(2)));
typedef float nfloat4 __attribute__((ext_vector_type(4)));
typedef float nfloat2 __attribute__((ext_vector_type(2)));

// the packed / DPP forms of conv_wg3_kernel's transforms (copied: V must come out with that kernel's bits)
__device__ __forceinline__ w2f2 pk_add2(w2f2 a, w2f2 b) { w2f2 r; asm("v_pk_add_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ w2f2 pk_sub2(w2f2 a, w2f2 b) { w2f2 r; asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ w2f2 pk_fma2(w2f2 a, w2f2 b, w2f2 c) { w2f2 r; asm("v_pk_fma_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }
__device__ __forceinline__ w2f2 pk_fms2(w2f2 a, w2f2 b, w2f2 c) { w2f2 r; asm("v_pk_fma_f32 %0, %1, %2, %3 neg_lo:[0,0,1] neg_hi:[0,0,1]" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }
__device__ __forceinline__ w2f2 pk_fnma2(w2f2 a, w2f2 b, w2f2 c) { w2f2 r; asm("v_pk_fma_f32 %0, %1, %2, %3 neg_lo:[0,1,0] neg_hi:[0,1,0]" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }
__device__ __forceinline__ w2f2 pk_sumdiff(w2f2 c) {          // (c1, c2) -> (c1 + c2, c2 - c1)
    w2f2 r;
    asm("v_pk_add_f32 %0, %1, %1 op_sel:[0,1] op_sel_hi:[1,0] neg_hi:[0,1]" : "=v"(r) : "v"(c));
    return r;
}
__device__ __forceinline__ w2f2 pk_sumdiff_fwd(w2f2 c) {      // (c1, c2) -> (c1 + c2, c1 - c2)
    w2f2 r;
    asm("v_pk_add_f32 %0, %1, %1 op_sel:[0,1] op_sel_hi:[0,1] neg_hi:[0,1]" : "=v"(r) : "v"(c));
    return r;
}
__device__ __forceinline__ w2f2 pk_addsub(w2f2 s, w2f2 a) { w2f2 r; asm("v_pk_add_f32 %0, %1, %2 neg_hi:[0,1]" : "=v"(r) : "v"(s), "v"(a)); return r; }
__device__ __forceinline__ w2f2 pk_sqacc(w2f2 a, w2f2 c) { w2f2 r; asm("v_pk_fma_f32 %0, %1, %1, %2" : "=v"(r) : "v"(a), "v"(c)); return r; }
__device__ __forceinline__ uint64_t lo64(float k) { return (uint64_t)__builtin_bit_cast(uint32_t, k); }
__device__ __forceinline__ w2f2 pks_mul(w2f2 a, float k) { w2f2 r; asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[1,0]" : "=v"(r) : "v"(a), "s"(lo64(k))); return r; }
__device__ __forceinline__ w2f2 pks_fma(w2f2 a, float k, w2f2 c) { w2f2 r; asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[1,0,1]" : "=v"(r) : "v"(a), "s"(lo64(k)), "v"(c)); return r; }
// value of lane - 2 of the same 16-lane row (0 past the row end) minus b;  a minus the value of lane + 2
__device__ __forceinline__ float sub_prev2(float x, float b) {
    float r;
    asm("v_sub_f32_dpp %0, %1, %2 row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:0" : "=v"(r) : "v"(x), "v"(b));
    return r;
}
__device__ __forceinline__ float sub_next2(float a, float x) {
    float r;
    asm("v_subrev_f32_dpp %0, %1, %2 row_shl:2 row_mask:0xf bank_mask:0xf bound_ctrl:0" : "=v"(r) : "v"(x), "v"(a));
    return r;
}
// sums over the 64 lanes of eight fp64 values per lane (conv_wg3_kernel's: fixed order)
__device__ __forceinline__ double wave_sum8(const double (&v)[8], int lane) {
    double w[4], u[2];
    const bool b5 = lane & 32, b4 = lane & 16, b3 = lane & 8;
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] = (b5 ? v[4 + i] : v[i]) + __shfl_xor(b5 ? v[i] : v[4 + i], 32, 64);
#pragma unroll
    for (int i = 0; i < 2; ++i) u[i] = (b4 ? w[2 + i] : w[i]) + __shfl_xor(b4 ? w[i] : w[2 + i], 16, 64);
    double t = (b3 ? u[1] : u[0]) + __shfl_xor(b3 ? u[0] : u[1], 8, 64);
    t += __shfl_xor(t, 4, 64);
    t += __shfl_xor(t, 2, 64);
    t += __shfl_xor(t, 1, 64);
    return t;
}

// x = h + m + l exactly (finite x): hardware RNE conversions, exact fp32 residuals
// two values to one packed bf16 pair (RNE; lo = a) and the pair's halves back as fp32
__device__ __forceinline__ uint32_t cvt_pk_bf16(float a, float b) {
    typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(w2f2{a, b}, bf16x2));
}
__device__ __forceinline__ float bf16_lo(uint32_t p) { return __builtin_bit_cast(float, p << 16); }
__device__ __forceinline__ float bf16_hi(uint32_t p) { return __builtin_bit_cast(float, p & 0xFFFF0000u); }

constexpr int X3_BM = 64, X3_TILES = 64, X3_SK = 16;
constexpr int X3_PC = 4 * 64 * X3_SK * 2;        // bytes of one piece of a sub-stage image: [4 xi][64 rows][16 ci] bf16
constexpr int X3_IMG = 3 * X3_PC;                // 24 KB
constexpr int X3_U = 0, X3_V = 2 * X3_IMG;       // U[2][IMG], V[2][IMG]
constexpr int X3_SCR = 4 * X3_IMG;               // GroupNorm reduction scratch (4 waves x 8 doubles), then the plane-0 partial sums
constexpr int X3_STASH = X3_SCR + 4 * 8 * 8;
constexpr int X3_LDS = X3_STASH + 256 * 8 * 4;
constexpr int X3_RUN = 4 * 64 * X3_SK;           // bf16 elements of one sub-stage run of one piece

struct WinoX3Args {
    SdcConvDesc d;
    const float* x0;
    const float* x1;
    const __bf16* wb;
    const float* bias;
    float* y;
    int Cin;
    uint32_t plane_bytes;        // bytes of one weight piece
    double* gn_part;
    int gn_G, gn_cpg, gn_nparts;
};

// DBG: parts of the loop switched off (WRONG RESULTS; experiment builds only, see the launch)
template <int OW, int DBG = 0>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1))) void conv_wg3_x3_kernel(const WinoX3Args a) {
    static_assert(OW == 16, "rows of 16: one lane per tile and stage channel quad");
    constexpr int BM = X3_BM, TW = OW / 2, LGW = 4;
    typedef const __attribute__((address_space(1))) char* gchar_p;
    typedef const __attribute__((address_space(1))) nfloat2* gfloat2_p;
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    typedef const __attribute__((address_space(1))) u32x4* guint4_p;
    typedef __attribute__((address_space(1))) char* gwchar_p;
    typedef __attribute__((address_space(1))) nfloat2* gwfloat2_p;
    extern __shared__ __attribute__((aligned(16))) char lds[];

    const SdcConvDesc& d = a.d;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = SDC_UNIFORM(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int l31 = lane & 31, lh = lane >> 5;
    const int MT = d.Cout / BM;
    const int lb = xcd_tile(blockIdx.x, gridDim.x);
    const int mt = lb % MT;
    const int m0 = mt * BM;
    const int tile0 = (lb / MT) * X3_TILES;
    const int H2 = d.oH >> 1, D2 = d.oD >> 1;
    // the workgroup's 8 row pairs lie in one plane pair (host check: H2 % 8 == 0): (sample ob, planes od, od + 1, first row pair hp0)
    int ob, od, hp0;
    {
        const int rp0 = tile0 >> (LGW - 1);          // < 2^20 (host check): the float quotients are exact
        const int q = (int)(((float)rp0 + 0.5f) * (1.0f / (float)H2));
        const int b = (int)(((float)q + 0.5f) * (1.0f / (float)D2));
        hp0 = SDC_UNIFORM(rp0 - q * H2);
        ob = SDC_UNIFORM(b);
        od = SDC_UNIFORM(2 * (q - b * D2));
    }
    const bool two = d.Cin1 > 0;

    // ---- park geometry (conv_wg3_kernel<16>): a 16-lane DPP row is two image row pairs interleaved; the lane owns columns pc0, pc0 + 1
    // of row pair pr, i.e. tile (pr, pc0 / 2), for the four channels 4 wave .. 4 wave + 3 of the stage
    const int pr = 2 * (lane >> 4) + (lane & 1), pc0 = 2 * ((lane & 15) >> 1);
    const int hp = hp0 + pr;
    const bool up_ok = hp > 0, dn_ok = 2 * hp + 2 < d.iH;
    const w2f2 m0p = {up_ok ? 1.0f : 0.0f, up_ok ? 1.0f : 0.0f}, m3p = {dn_ok ? 1.0f : 0.0f, dn_ok ? 1.0f : 0.0f};
    const uint32_t rsel0 = up_ok ? OW * 4 : 0, rsel3 = dn_ok ? 2 * OW * 4 : 0;
    const uint32_t vp = (uint32_t)((2 * hp) * OW + pc0) * 4u;                    // bytes inside a plane (both inputs: rows contiguous)
    // (the 16-byte halves of a row -- channel octets -- swap places in rows 8-15 of every 16: a fragment read's 16-lane groups then
    // cover all 64 banks, and the 8-byte stores of a 16-lane group are two-way instead of four-way)
    const int ptile = pr * TW + (pc0 >> 1);
    const int vpark = X3_V + ptile * 32 + (((wave >> 1) ^ ((ptile >> 3) & 1)) * 16) + (wave & 1) * 8;      // + buf * IMG + piece * PC + xi * 2048
    // fragments: row (wm / wn) * 32 + l31, channel octet lh
    const int afrag = X3_U + (wm * 32 + l31) * 32 + (lh ^ ((l31 >> 3) & 1)) * 16;
    const int bfrag = X3_V + (wn * 32 + l31) * 32 + (lh ^ ((l31 >> 3) & 1)) * 16;
    // weight run items: 16-byte item it = tid + 256 k of the sub-stage's [piece][512] items
    uint32_t uoff[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const int it = tid + 256 * k;
        uoff[k] = (uint32_t)(it >> 9) * a.plane_bytes + (uint32_t)(it & 511) * 16u;
    }

    const int64_t xs1_0 = d.x0s[1], xs1_1 = d.x1s[1];
    const int cin0 = d.Cin0, cin = a.Cin;
    const int S1 = cin / X3_SK;                      // stages per depth component
    const float* const x0p = a.x0 + (int64_t)ob * d.x0s[0] + (int64_t)od * d.x0s[2];
    const float* const x1p = two ? a.x1 + (int64_t)ob * d.x1s[0] + (int64_t)od * d.x1s[2] : x0p;
    const int64_t xs2_0 = d.x0s[2], xs2_1 = two ? d.x1s[2] : d.x0s[2];
    const uint32_t lo_u = (uint32_t)(-od) >> 31, hi_u = (uint32_t)(od + 2 - d.iD) >> 31;     // planes od - 1 / od + 2 exist

    // ---- raw rows of a stage: [channel][depth slice a / b][source row], two columns each
    w2f2 raw[4][2][4];
    int s_jd = 0, s_ci = 0;
    float mka = 0.f, mkb = 0.f;
    const float *f_xa = x0p, *f_xb = x0p;
    int64_t f_sc = 0;
    uint32_t voff = vp, voff0 = vp - rsel0, voff3 = vp + rsel3;
    // scalar part of a stage's fetch: input, planes and signs of depth component s_jd
    auto fetch_raw_begin = [&]() __attribute__((always_inline)) {
        const bool first = s_ci < cin0;
        f_sc = first ? xs1_0 : xs1_1;
        const int64_t xs2 = first ? xs2_0 : xs2_1;
        const int cbase = (first ? s_ci : s_ci - cin0) + wave * 4;
        const float* bsel = (first ? x0p : x1p) + (int64_t)cbase * f_sc;
        // pass s_jd (0..3) works on depth component 1, 2, 0, 3; planes (relative to od) and signs as in conv_wg3_kernel: a plane outside
        // the volume is plane od with factor 0 (integer arithmetic on the float bits: no branch in the loop)
        const int jd_u = SDC_UNIFORM(s_jd);
        const uint32_t j0 = (uint32_t)((jd_u ^ 2) - 1) >> 31, j2 = (uint32_t)((jd_u ^ 1) - 1) >> 31, j3 = (uint32_t)((jd_u ^ 3) - 1) >> 31;
        const int da = -(int)(j0 & lo_u);
        const int db = 1 + (int)j3 * (2 * (int)hi_u - 1);
        mka = __builtin_bit_cast(float, (0x3F800000u & ((j0 & (lo_u ^ 1u)) - 1u)) | (j2 << 31));
        mkb = __builtin_bit_cast(float, (0x3F800000u & ((j3 & (hi_u ^ 1u)) - 1u)) | ((j0 | (j3 & hi_u)) << 31));
        f_xa = bsel + da * xs2;
        f_xb = bsel + db * xs2;
        // (past the last stage the walk wraps to the first one: the extra fetches of the pipeline tail stay in bounds and are never
        // consumed; selects, not branches)
        const int nci = s_ci + X3_SK;
        const bool wrap = nci >= cin;
        s_ci = wrap ? 0 : nci;
        s_jd = wrap ? ((s_jd + 1) & 3) : s_jd;
    };
    // the four rows of (channel ch, depth slice sl): scalar base + 32-bit lane offset (the offsets pass through an empty asm so that
    // their zero-extension is not hoisted out of the loop as 64-bit register pairs)
    auto fetch_raw_rows = [&](int ch, int sl) __attribute__((always_inline)) {
        const gchar_p rb = (gchar_p)uniform_ptr((sl ? f_xb : f_xa) + ch * f_sc);
        asm volatile("" : "+v"(voff), "+v"(voff0), "+v"(voff3));
        const nfloat2 v0 = *(gfloat2_p)(rb + voff0), v1 = *(gfloat2_p)(rb + voff), v2 = *(gfloat2_p)(rb + voff + OW * 4), v3 = *(gfloat2_p)(rb + voff3);
        raw[ch][sl][0] = w2f2{v0.x, v0.y}; raw[ch][sl][1] = w2f2{v1.x, v1.y};
        raw[ch][sl][2] = w2f2{v2.x, v2.y}; raw[ch][sl][3] = w2f2{v3.x, v3.y};
    };
    // depth combination e_j = ca a_j + cb b_j fused with the H transform, per channel (conv_wg3_kernel's operations)
    w2f2 hrow[4][4];              // [channel][transformed row j]
    w2f2 ka0, kb0, ka3, kb3;
    auto h_begin = [&](float ca, float cb) __attribute__((always_inline)) {
        ka0 = pks_mul(m0p, ca); kb0 = pks_mul(m0p, cb); ka3 = pks_mul(m3p, ca); kb3 = pks_mul(m3p, cb);
    };
    auto h_transform = [&](int ch, float ca, float cb) __attribute__((always_inline)) {
        const w2f2 e1 = pks_fma(raw[ch][1][1], cb, pks_mul(raw[ch][0][1], ca));
        const w2f2 e2 = pks_fma(raw[ch][1][2], cb, pks_mul(raw[ch][0][2], ca));
        hrow[ch][0] = pk_fma2(raw[ch][1][0], kb0, pk_fms2(raw[ch][0][0], ka0, e2));       // e0 - e2
        hrow[ch][1] = pk_add2(e1, e2);
        hrow[ch][2] = pk_sub2(e2, e1);
        hrow[ch][3] = pk_fnma2(raw[ch][1][3], kb3, pk_fnma2(raw[ch][0][3], ka3, e1));     // e1 - e3
    };
    // Parking component (j, xi) of the thread's four channels, in five steps that each fit behind one MFMA and hold four independent
    // chains (a dependent VALU instruction waits for its predecessor; the next one of another channel does not):
    //   0  the W transform of the component -- V0 = c0 - c2, (V1, V2) = (c1 + c2, c2 - c1), V3 = c1 - c3, the neighbour columns through
    //      DPP -- and h of the four channels       1  x - h       2  m and its fp32 form       3  x - h - m and l
    //   4  three 8-byte stores (h, m, l of the four channels)
    float px[4], pf[4];
    uint32_t ph[2], pm[2], pl[2];
    w2f2 sdv[4];
    auto park_step = [&](int buf, int j, int xi, int k) __attribute__((always_inline)) {
#pragma clang fp contract(off)
        if (k == 0) {
#pragma unroll
            for (int ch = 0; ch < 4; ++ch) {
                const w2f2 cc = hrow[ch][j];
                if (xi == 0) px[ch] = sub_prev2(cc.y, cc.y);
                else if (xi == 1) { sdv[ch] = pk_sumdiff(cc); px[ch] = sdv[ch].x; }
                else if (xi == 2) px[ch] = sdv[ch].y;
                else px[ch] = sub_next2(cc.x, cc.x);
            }
            ph[0] = cvt_pk_bf16(px[0], px[1]);
            ph[1] = cvt_pk_bf16(px[2], px[3]);
        } else if (k == 1) {
            pf[0] = bf16_lo(ph[0]); pf[1] = bf16_hi(ph[0]); pf[2] = bf16_lo(ph[1]); pf[3] = bf16_hi(ph[1]);
#pragma unroll
            for (int i = 0; i < 4; ++i) px[i] = px[i] - pf[i];
        } else if (k == 2) {
            pm[0] = cvt_pk_bf16(px[0], px[1]);
            pm[1] = cvt_pk_bf16(px[2], px[3]);
            pf[0] = bf16_lo(pm[0]); pf[1] = bf16_hi(pm[0]); pf[2] = bf16_lo(pm[1]); pf[3] = bf16_hi(pm[1]);
        } else if (k == 3) {
#pragma unroll
            for (int i = 0; i < 4; ++i) px[i] = px[i] - pf[i];
            pl[0] = cvt_pk_bf16(px[0], px[1]);
            pl[1] = cvt_pk_bf16(px[2], px[3]);
        } else {
            char* dst = lds + vpark + buf * X3_IMG + xi * 2048;
            *reinterpret_cast<uint2*>(dst) = make_uint2(ph[0], ph[1]);
            *reinterpret_cast<uint2*>(dst + X3_PC) = make_uint2(pm[0], pm[1]);
            *reinterpret_cast<uint2*>(dst + 2 * X3_PC) = make_uint2(pl[0], pl[1]);
        }
    };
    // ---- weight runs: sub-stage walk (pass, stage, j) in pass order
    u32x4 ureg[2][6];            // [set]: runs of sub-stages of equal parity; two runs are in flight
    int u_p = 0, u_st = 0, u_j = 0;
    gchar_p u_base = (gchar_p)uniform_ptr(reinterpret_cast<const float*>(a.wb));
    auto fetch_u_begin = [&]() __attribute__((always_inline)) {
        const int jdc = (0xC9 >> (2 * u_p)) & 3;                 // pass 0..3 -> depth component 1, 2, 0, 3
        const int run = ((mt * 4 + jdc) * S1 + u_st) * 4 + u_j;
        u_base = (gchar_p)uniform_ptr(reinterpret_cast<const float*>(a.wb + (int64_t)run * X3_RUN));
        // (the walk wraps like the rows': selects, not branches)
        const bool wj = u_j == 3, ws = wj && u_st + 1 == S1;
        u_j = (u_j + 1) & 3;
        u_st = ws ? 0 : (wj ? u_st + 1 : u_st);
        u_p = ws ? ((u_p + 1) & 3) : u_p;
    };
    auto fetch_u_item = [&](int set, int k) __attribute__((always_inline)) {
        asm volatile("" : "+v"(uoff[k]));
        ureg[set][k] = *(guint4_p)(u_base + uoff[k]);
    };
    auto park_u_item = [&](int buf, int k) __attribute__((always_inline)) {
        *reinterpret_cast<u32x4*>(lds + X3_U + buf * X3_IMG + (tid + 256 * k) * 16) = ureg[buf][k];
    };
    // fragments of component xi of a buffer: piece p of U (p < 3) or of V (p - 3)
    bf16x8 fr[2][6];
    auto read_frag = [&](int buf, int xi, int set, int p) __attribute__((always_inline)) {
        fr[set][p] = *reinterpret_cast<const bf16x8*>(lds + (p < 3 ? afrag : bfrag) + buf * X3_IMG + (p % 3) * X3_PC + xi * 2048);
    };

    f32x16 acc[16];
    // the bias rides on component (j, xi) = (1, 1) of depth component 1 (coefficient +1 in all 8 outputs): the start value of that
    // accumulator in the first pass.  Register r of a lane is channel m0 + 32 wm + 8 (r >> 2) + 4 lh + (r & 3).
    f32x16 zero16, biasv;
#pragma unroll
    for (int r = 0; r < 16; ++r) { zero16[r] = 0.0f; biasv[r] = a.bias ? a.bias[m0 + wm * 32 + 8 * (r >> 2) + 4 * lh + (r & 3)] : 0.0f; }

    float pka, pkb;               // factors of the raw rows in registers
    {   // prologue: stage 0 is transformed and its row 0 parked in buffer 0; the weight runs of sub-stages 1 and 2 travel
        fetch_raw_begin();
        pka = mka; pkb = mkb;
#pragma unroll
        for (int g = 0; g < 8; ++g) fetch_raw_rows(g >> 1, g & 1);
        fetch_u_begin();
#pragma unroll
        for (int k = 0; k < 6; ++k) fetch_u_item(0, k);
        fetch_u_begin();
#pragma unroll
        for (int k = 0; k < 6; ++k) fetch_u_item(1, k);
        h_begin(pka, pkb);
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) h_transform(ch, pka, pkb);
#pragma unroll
        for (int k = 0; k < 6; ++k) park_u_item(0, k);
#pragma unroll
        for (int st = 0; st < 20; ++st) park_step(0, 0, st / 5, st % 5);
        fetch_u_begin();
#pragma unroll
        for (int k = 0; k < 6; ++k) fetch_u_item(0, k);
    }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < 6; ++p) read_frag(0, 0, 0, p);

    // ---- output geometry (conv_wg3_kernel's)
    const int cob = m0 + wm * 32;
    const int nloc = wn * 32 + l31;
    const int ohp = hp0 + (nloc >> (LGW - 1)), otw = nloc & (TW - 1);
    const uint32_t yoff = (uint32_t)((2 * ohp) * d.ys[3] + (2 * otw) * d.ys[4] + (4 * lh) * d.ys[1]) * 4u;
    const uint32_t yoff1 = yoff + (uint32_t)d.ys[3] * 4u;
    const bool gn = a.gn_part != nullptr;
    float gp[8];
    float* const gstash = reinterpret_cast<float*>(lds + X3_STASH) + tid * 8;

    // fold of pass p into the plane pair (conv_wg3_kernel's, as it stands).  Pass order: depth components 1, 2, 0, 3 --
    //   p 0 (m1): plane 1 <- m1;  p 1 (m2): plane 0 <- m1 + m2, plane 1 <- m1 - m2;  p 2 (m0): plane 0 finished;  p 3 (m3): plane 1 finished
    auto fold = [&](const int p) __attribute__((always_inline)) {
        const bool t0 = p == 1 || p == 2, t1 = p != 2;
        const bool ld0 = p == 2, ld1 = p == 1 || p == 3;
        const bool fin0 = p == 2, fin1 = p == 3;
        const bool always = d.Cout > 0;
        const int LEAD = 2;
        const int64_t ycs4 = d.ys[1] * 4;
        float* const y0p = a.y + (int64_t)ob * d.ys[0] + (int64_t)od * d.ys[2] + (int64_t)cob * d.ys[1];
        gwchar_p s0 = (gwchar_p)(__attribute__((address_space(1))) void*)uniform_ptr(y0p);
        gwchar_p s1 = (gwchar_p)(__attribute__((address_space(1))) void*)uniform_ptr(y0p + d.ys[2]);
        gchar_p l0 = (gchar_p)s0, l1 = (gchar_p)s1;
        w2f2 P0[4][4][2], P1[4][4][2];
        auto load_block = [&](int g4) __attribute__((always_inline)) {
#pragma unroll
            for (int r3 = 0; r3 < 4; ++r3) {
                if (ld0) { P0[g4][r3][0] = *(gfloat2_p)(l0 + yoff); P0[g4][r3][1] = *(gfloat2_p)(l0 + yoff1); l0 += r3 < 3 ? ycs4 : 5 * ycs4; }
                if (ld1) { P1[g4][r3][0] = *(gfloat2_p)(l1 + yoff); P1[g4][r3][1] = *(gfloat2_p)(l1 + yoff1); l1 += r3 < 3 ? ycs4 : 5 * ycs4; }
            }
        };
        if (ld0 || ld1) {
#pragma unroll
            for (int g = 0; g < LEAD; ++g) load_block(g);
        }
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            if (g4 + LEAD < 4 && (ld0 || ld1)) load_block(g4 + LEAD);
            // (each 8-row block its own basic block: see conv_wg3_kernel)
            if (!always) continue;
            w2f2 bs2 = {0.f, 0.f}, bq2 = {0.f, 0.f};
#pragma unroll
            for (int r3 = 0; r3 < 4; ++r3) {
                const int rr = g4 * 4 + r3;
                w2f2 pa[4], pb[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    pa[j] = w2f2{acc[4 * j][rr], acc[4 * j + 3][rr]};
                    pb[j] = w2f2{acc[4 * j + 1][rr], acc[4 * j + 2][rr]};
                }
                const w2f2 t0a = pk_add2(pk_add2(pa[0], pa[1]), pa[2]), t1a = pk_sub2(pk_sub2(pa[1], pa[2]), pa[3]);
                const w2f2 t0b = pk_add2(pk_add2(pb[0], pb[1]), pb[2]), t1b = pk_sub2(pk_sub2(pb[1], pb[2]), pb[3]);
                const w2f2 z0 = pk_addsub(pk_sumdiff_fwd(t0b), t0a);
                const w2f2 z1 = pk_addsub(pk_sumdiff_fwd(t1b), t1a);
                if (t0) {
                    const bool have = p == 1 ? ld1 : ld0;
                    const w2f2 b0 = p == 1 ? P1[g4][r3][0] : P0[g4][r3][0], b1 = p == 1 ? P1[g4][r3][1] : P0[g4][r3][1];
                    const w2f2 u0 = have ? pk_add2(b0, z0) : z0, u1 = have ? pk_add2(b1, z1) : z1;
                    *(gwfloat2_p)(s0 + yoff) = nfloat2{u0.x, u0.y};
                    *(gwfloat2_p)(s0 + yoff1) = nfloat2{u1.x, u1.y};
                    s0 += r3 < 3 ? ycs4 : 5 * ycs4;
                    if (fin0) { bs2 = pk_add2(bs2, pk_add2(u0, u1)); bq2 = pk_sqacc(u1, pk_sqacc(u0, bq2)); }
                }
                if (t1) {
                    const w2f2 u0 = ld1 ? pk_sub2(P1[g4][r3][0], z0) : z0, u1 = ld1 ? pk_sub2(P1[g4][r3][1], z1) : z1;
                    *(gwfloat2_p)(s1 + yoff) = nfloat2{u0.x, u0.y};
                    *(gwfloat2_p)(s1 + yoff1) = nfloat2{u1.x, u1.y};
                    s1 += r3 < 3 ? ycs4 : 5 * ycs4;
                    if (fin1) { bs2 = pk_add2(bs2, pk_add2(u0, u1)); bq2 = pk_sqacc(u1, pk_sqacc(u0, bq2)); }
                }
            }
            if (fin0 || fin1) { gp[2 * g4] = bs2.x + bs2.y; gp[2 * g4 + 1] = bq2.x + bq2.y; }
        }
        if (fin0 && gn) {
            *reinterpret_cast<nfloat4*>(gstash) = nfloat4{gp[0], gp[1], gp[2], gp[3]};
            *reinterpret_cast<nfloat4*>(gstash + 4) = nfloat4{gp[4], gp[5], gp[6], gp[7]};
        }
    };

    // ---- sub-stage (stage, j): 24 MFMAs from buffer j & 1 -- component by component, the six terms of a component smallest first --
    // while row j + 1 (row 0 of the next stage) is parked in the other buffer.  The other work sits in 24 slots, one behind each MFMA, in
    // source order (a VALU instruction between two MFMAs is hidden only while the matrix pipe is busy, so it is dealt out evenly):
    //   every slot of components 0-2   one fragment read of the next component
    //   slots 0-5     the weight run of sub-stage q + 1 (in registers) into the other buffer
    //   slots 6-11    the run of sub-stage q + 3 into flight, in the registers just parked (the run of q + 2 is on its way in the other set:
    //                 a run has a sub-stage and three quarters to arrive)
    //   slots 0-19    the 4 x 5 park steps of the row
    //   slots 12-19   (j = 0) the raw rows of the next stage into flight, one (channel, depth slice) each
    //   slot 20       the barrier: every park of q + 1 is done and every fragment read of this buffer has returned
    //   slots 20-23   (j = 2) depth combination and H transform of the next stage, a channel each (row 3 of this one is parked)
    //   slots 21-23   the fragments of component 0 of sub-stage q + 1
    // FIRST: the first stage of a pass starts its accumulators from zero (from the bias for component (1, 1) of the first pass) in the MFMA.
    auto substage = [&](auto FIRST, auto J, const int pass) __attribute__((always_inline)) {
        constexpr bool first = decltype(FIRST)::value;
        constexpr int j = decltype(J)::value;
        constexpr int rbuf = j & 1, wbuf = rbuf ^ 1, jn = (j + 1) & 3;
#pragma unroll
        for (int sl = 0; sl < 24; ++sl) {
            const int xi = sl / 6, t = sl % 6, c = 4 * j + xi, set = xi & 1;
            const f32x16 cstart = (first && t == 0) ? ((c == 5 && pass == 0) ? biasv : zero16) : acc[c];
            if (!(DBG & 64) || t == 0) acc[c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fr[set][X3_PA[t]], fr[set][3 + X3_PB[t]], cstart, 0, 0, 0);
            if (DBG & 16) {}
            else if (xi < 3) read_frag(rbuf, xi + 1, set ^ 1, t);
            else if (t >= 3) { read_frag(wbuf, 0, 0, 2 * (t - 3)); read_frag(wbuf, 0, 0, 2 * (t - 3) + 1); }
            if (sl < 6) { if (!(DBG & 4)) park_u_item(wbuf, sl); }
            else if (sl < 12) { if (sl == 6) fetch_u_begin(); if (!(DBG & 2)) fetch_u_item(wbuf, sl - 6); }
            if (sl < 20 && !(DBG & 1)) park_step(wbuf, jn, sl / 5, sl % 5);
            if (j == 0 && sl >= 12 && sl < 20 && !(DBG & 8)) {
                if (sl == 12) { fetch_raw_begin(); pka = mka; pkb = mkb; }
                fetch_raw_rows((sl - 12) >> 1, (sl - 12) & 1);
            }
            if (j == 2 && sl >= 20) {
                if (sl == 20) h_begin(pka, pkb);
                h_transform(sl - 20, pka, pkb);
            }
            __builtin_amdgcn_sched_barrier(0);
            if (sl == 20 && !(DBG & 32)) __syncthreads();
        }
    };
    auto stage = [&](auto FIRST, const int pass) __attribute__((always_inline)) {
        substage(FIRST, std::integral_constant<int, 0>{}, pass);
        substage(FIRST, std::integral_constant<int, 1>{}, pass);
        substage(FIRST, std::integral_constant<int, 2>{}, pass);
        substage(FIRST, std::integral_constant<int, 3>{}, pass);
    };
    auto run_pass = [&](auto P) __attribute__((always_inline)) {
        constexpr int p = decltype(P)::value;
        stage(std::true_type{}, p);
        for (int st = 1; st < S1; ++st) stage(std::false_type{}, p);
        fold(p);
        // (the first fragments of the next pass, read again: carried across the fold they cost 24 registers there)
#pragma unroll
        for (int q = 0; q < 6; ++q) read_frag(0, 0, 0, q);
    };
    run_pass(std::integral_constant<int, 0>{});
    run_pass(std::integral_constant<int, 1>{});
    run_pass(std::integral_constant<int, 2>{});
    run_pass(std::integral_constant<int, 3>{});

    if (gn) {
        // (the thread index taken again behind an empty asm: values derived from the first copy would stay live through the whole kernel)
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
        const int lane = tid & 63;
        double* scr = reinterpret_cast<double*>(lds + X3_SCR);
        double gv[8];                                // fp64 from here on
        {
            const nfloat4 s0 = *reinterpret_cast<const nfloat4*>(gstash), s1 = *reinterpret_cast<const nfloat4*>(gstash + 4);
            const float g0[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
#pragma unroll
            for (int i = 0; i < 8; ++i) gv[i] = (double)g0[i] + (double)gp[i];
        }
        const double tot = wave_sum8(gv, lane);
        if ((lane & 7) == 0) scr[wave * 8 + (lane >> 3)] = tot;
        __syncthreads();
        const int ngl = a.gn_cpg >= BM ? 1 : BM / a.gn_cpg;       // groups inside this workgroup's rows
        if (tid < ngl) {
            const int r0 = a.gn_cpg >= BM ? 0 : tid * a.gn_cpg, r1 = a.gn_cpg >= BM ? BM : r0 + a.gn_cpg;   // local rows
            double sum = 0.0, sq = 0.0;
            for (int blk = r0 / 8; blk < r1 / 8; ++blk) {
                const int wmi = blk >> 2, k = blk & 3;
                for (int wni = 0; wni < 2; ++wni) {
                    sum += scr[((wmi * 2 + wni) * 4 + k) * 2];
                    sq += scr[((wmi * 2 + wni) * 4 + k) * 2 + 1];
                }
            }
            const int g = (m0 + r0) / a.gn_cpg;
            const int ntl = tile0 / X3_TILES - ob * (D2 * H2 * TW / X3_TILES);      // part of the sample (512 positions each)
            const int idx = a.gn_cpg >= BM ? ntl * (a.gn_cpg / BM) + (m0 - g * a.gn_cpg) / BM : ntl;
            double* pp = a.gn_part + (((int64_t)ob * a.gn_G + g) * a.gn_nparts + idx) * 2;
            pp[0] = sum; pp[1] = sq;
        }
    }
}

// Wb[piece][co / 64][jd][stage][j][xi][co % 64][(ci % 16) ^ 8 ((co >> 3) & 1)]: the three bf16 pieces of U3[jd][ci][co][j * 4 + xi];
// one thread per element of a plane
__global__ __launch_bounds__(256) void pack_wino3_x3_kernel(const float* __restrict__ u3, __bf16* __restrict__ out, int Cout, int Cin, int64_t n) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const int c16 = (int)(e & 15), col = (int)((e >> 4) & 63), xi = (int)((e >> 10) & 3), j = (int)((e >> 12) & 3);
    int64_t r = e >> 14;
    const int S1 = Cin / 16;
    const int st = (int)(r % S1); r /= S1;
    const int jd = (int)(r & 3);
    const int mt = (int)(r >> 2);
    const int ci = st * 16 + (c16 ^ (((col >> 3) & 1) << 3)), co = mt * 64 + col;     // (rows 8-15 of every 16: the channel octets swapped)
    __bf16 ph, pm, pl;
    split3(u3[(((int64_t)jd * Cin + ci) * Cout + co) * 16 + j * 4 + xi], ph, pm, pl);
    out[e] = ph; out[n + e] = pm; out[2 * n + e] = pl;
}

bool x3_small(const SdcConvDesc& d) {
    auto span = [](const int64_t* st, int b, int dd, int h, int w) {
        return (int64_t)(b - 1) * st[0] + (int64_t)(dd - 1) * st[2] + (int64_t)(h - 1) * st[3] + (int64_t)(w - 1) * st[4];
    };
    return span(d.x0s, d.B, d.iD, d.iH, d.iW) < (1ll << 30) && (d.Cin1 == 0 || span(d.x1s, d.B, d.iD, d.iH, d.iW) < (1ll << 30));
}

// coverage of conv_wg3_x3_kernel: what conv_wg3_kernel takes (wg3_ok at precision 4: 3x3x3 taps, stride 1, 'same' padding, an even depth,
// whole 64-channel blocks, the row pairs of a workgroup inside one plane, 8-byte aligned rows of y, no fused residual), rows of 16, whole
// 16-channel stages in each input.  Descriptor only; d.precision is not looked at.
bool wino3_x3_covers(const SdcConvDesc& d) {
    if (!(d.B > 0 && d.Cin0 > 0 && d.Cin1 >= 0 && d.Cout > 0 && d.oW == 16)) return false;
    if (d.Cin0 % X3_SK != 0 || d.Cin1 % X3_SK != 0) return false;
    SdcConvDesc e = d;
    e.precision = 4;
    if (!wg3_ok(e, x3_small(e))) return false;
    // one weight piece below 2^30 bytes (32-bit lane offsets over the three pieces)
    return (int64_t)64 * (d.Cin0 + d.Cin1) * d.Cout * 2 < (1ll << 30);
}

// partial sums per (sample, group) of the GroupNorm epilogue: conv_wg3_kernel's (sdc_conv_gnparts of the same conv at precision 4)
int wino3_x3_gnparts(const SdcConvDesc& d, int G) {
    if (G <= 0 || d.Cout % G) return 0;
    const int cpg = d.Cout / G;
    const int64_t S = (int64_t)d.oD * d.oH * d.oW;
    const int bn = X3_TILES * 8;
    if (cpg % 8 || S % bn || !(cpg % X3_BM == 0 || X3_BM % cpg == 0)) return 0;
    return (int)(S / bn) * (cpg >= X3_BM ? cpg / X3_BM : 1);
}

// The routing table of net.wino_split: the shapes where every repeat of sdc_conv_wino3_x3 measured faster than every
// repeat of sdc_conv at precision 4 on the same buffers (profiles/wino_x3_shapes.log).  Per-sample sizes only, never B.
//   at 32 x 16 x 16 (the 16 x 16 level of the C4 net):  128 -> 256 (x1.05),  256 -> 256 (x1.05-1.06),  256 + 256 -> 128 (x1.06)
//   128 -> 128 at 32 x 16 x 16 stays fp32: x1.04-1.07, but one repeat of one of its three launches did not beat every fp32 repeat
//   (the rows of 32 and of 64 are not covered)
bool wino3_x3_faster(const SdcConvDesc& d) {
    if (!(d.oD == 32 && d.oH == 16 && d.oW == 16)) return false;
    const int c0 = d.Cin0, c1 = d.Cin1, co = d.Cout;
    return (c0 == 128 && c1 == 0 && co == 256) || (c0 == 256 && c1 == 0 && co == 256) || (c0 == 256 && c1 == 256 && co == 128);
}

}  // namespace

extern "C" int sdc_conv_wino3_x3_ok(const SdcConvDesc* dp) {
    return dp && wino3_x3_covers(*dp) && wino3_x3_faster(*dp) ? 1 : 0;
}

extern "C" size_t sdc_pack_wino3_x3_bytes(int Cout, int Cin) {
    if (Cout <= 0 || Cout % 64 != 0 || Cin <= 0 || Cin % 16 != 0) return 0;
    return (size_t)3 * 64 * Cin * Cout * sizeof(__bf16);
}

extern "C" int sdc_pack_wino3_x3(const float* wp, void* out, int Cout, int Cin, void* stream) {
    SDC_REQUIRE(wp && out, SDC_ENULL, "sdc_pack_wino3_x3: null pointer");
    SDC_REQUIRE(sdc_pack_wino3_x3_bytes(Cout, Cin) > 0, SDC_EINVAL, "sdc_pack_wino3_x3: Cout a multiple of 64, Cin a multiple of 16 (got Cin %d, Cout %d)", Cin, Cout);
    const int64_t n = (int64_t)64 * Cin * Cout;
    SDC_REQUIRE(n / 256 + 1 < (1ll << 31), SDC_EINVAL, "sdc_pack_wino3_x3: weight too large");
    // U3 behind Wp, the F(2,3) taps and the F(2x2,3x3) taps of the precision-4 buffer (include/sdc.h)
    const int64_t K = (int64_t)27 * Cin;
    const float* u3 = wp + K * Cout + (K / 3 * 4) * Cout + (K / 9 * 16) * Cout;
    hipLaunchKernelGGL(pack_wino3_x3_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, sdc::as_stream(stream), u3,
                       reinterpret_cast<__bf16*>(out), Cout, Cin, n);
    return sdc::check_launch("sdc_pack_wino3_x3");
}

extern "C" int sdc_conv_wino3_x3(const SdcConvDesc* dp, const float* x, const float* x1, const void* wb, const float* bias, float* y,
                                 double* gn_parts, int gn_groups, void* stream) {
    SDC_REQUIRE(dp && x && wb && y, SDC_ENULL, "sdc_conv_wino3_x3: null pointer");
    const SdcConvDesc& d = *dp;
    SDC_REQUIRE(d.Cin1 <= 0 || x1, SDC_ENULL, "sdc_conv_wino3_x3: Cin1 > 0 but x1 is null");
    SDC_REQUIRE(wino3_x3_covers(d), SDC_EINVAL, "sdc_conv_wino3_x3: descriptor not covered: %dx%dx%d taps, stride %dx%dx%d, Cin %d+%d, Cout %d, "
                "residual %d, output %dx%dx%d", d.kD, d.kH, d.kW, d.sD, d.sH, d.sW, d.Cin0, d.Cin1, d.Cout, (int)(d.rs[1] != 0), d.oD, d.oH, d.oW);
    auto al = [](const void* p, int b) { return reinterpret_cast<uintptr_t>(p) % b == 0; };
    SDC_REQUIRE(al(wb, 16) && al(x, 8) && (d.Cin1 == 0 || al(x1, 8)) && al(y, 8), SDC_EALIGN,
                "sdc_conv_wino3_x3: the packed weight buffer must be 16-byte aligned, x, x1 and y 8-byte aligned");
    WinoX3Args a;
    a.d = d;
    a.x0 = x; a.x1 = x1; a.wb = reinterpret_cast<const __bf16*>(wb); a.bias = bias; a.y = y;
    a.Cin = d.Cin0 + d.Cin1;
    a.plane_bytes = (uint32_t)((int64_t)64 * a.Cin * d.Cout * 2);
    a.gn_part = nullptr; a.gn_G = a.gn_cpg = a.gn_nparts = 0;
    if (gn_parts) {
        const int np = wino3_x3_gnparts(d, gn_groups);
        SDC_REQUIRE(np > 0, SDC_EINVAL, "sdc_conv_wino3_x3: shape not covered by the fused statistics (%d groups over %d channels)", gn_groups, d.Cout);
        a.gn_part = gn_parts; a.gn_G = gn_groups; a.gn_cpg = d.Cout / gn_groups; a.gn_nparts = np;
    }
    const int64_t tiles = (int64_t)d.B * (d.oD / 2) * (d.oH / 2) * (d.oW / 2);
    const dim3 grid((unsigned)((tiles / X3_TILES) * (d.Cout / X3_BM)));
#define X3_LAUNCH(D)                                                                                             \
    do {                                                                                                         \
        static std::atomic<uint64_t> attr{0};                                                                    \
        SDC_LDS_OPTIN(attr, (conv_wg3_x3_kernel<16, D>), 160 * 1024, "sdc_conv_wino3_x3");                       \
        hipLaunchKernelGGL((conv_wg3_x3_kernel<16, D>), grid, dim3(256), X3_LDS, sdc::as_stream(stream), a);     \
    } while (0)
#ifdef SDC_KERNEL_EXPERIMENTS
    // kernel experiments (WRONG RESULTS): bits 1 no V transform / split / park, 2 no weight loads, 4 no weight park, 8 no row loads,
    // 16 no fragment reads, 32 no barrier, 64 one MFMA per component
    static const int dbg = exp_env("SDC_WG3X_DBG");
    switch (dbg) {
        case 0: break;
        case 1: X3_LAUNCH(1); return sdc::check_launch("sdc_conv_wino3_x3"); case 2: X3_LAUNCH(2); return sdc::check_launch("sdc_conv_wino3_x3");
        case 4: X3_LAUNCH(4); return sdc::check_launch("sdc_conv_wino3_x3"); case 8: X3_LAUNCH(8); return sdc::check_launch("sdc_conv_wino3_x3");
        case 16: X3_LAUNCH(16); return sdc::check_launch("sdc_conv_wino3_x3"); case 32: X3_LAUNCH(32); return sdc::check_launch("sdc_conv_wino3_x3");
        case 64: X3_LAUNCH(64); return sdc::check_launch("sdc_conv_wino3_x3"); case 6: X3_LAUNCH(6); return sdc::check_launch("sdc_conv_wino3_x3");
        case 15: X3_LAUNCH(15); return sdc::check_launch("sdc_conv_wino3_x3"); case 31: X3_LAUNCH(31); return sdc::check_launch("sdc_conv_wino3_x3");
        default: X3_LAUNCH(63); return sdc::check_launch("sdc_conv_wino3_x3");
    }
#endif
    X3_LAUNCH(0);
#undef X3_LAUNCH
    return sdc::check_launch("sdc_conv_wino3_x3");
}
