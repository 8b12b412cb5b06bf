// net.stem_split (default on at precision >= 4, samplers only): the 7-tap stem convs -- Conv1d k7 (1x1x7), Conv2d 7x7 (1x7x7) and Conv3d
// 7x7x7, Cin <= 8, 'same' padding -- as a direct-form implicit GEMM on v_mfma_f32_32x32x16_bf16 with EXACT three-way bf16 operand splits:
// fp32 inputs, fp32 accumulation, fp32 outputs.
//
//   x = x1 + x2 + x3 exactly,  x1 = bf16(x), x2 = bf16(x - x1), x3 = bf16(x - x1 - x2)   (RNE; three 8-bit significands carry the 24 of an fp32)
//   a b ~= a3 b1 + a2 b2 + a1 b3 + a2 b1 + a1 b2 + a1 b1      six MFMAs, smallest terms first; the dropped terms are below 2^-24 |a b|
//
// (a = weight, b = activation.)  A bf16 x bf16 product is exact in fp32, so the result is an fp32-grade conv whose error is that of the
// fp32 accumulation order, as with the fp32 matrix pipe.  Non-finite inputs: the residuals form inf - inf = NaN, so an infinite input
// gives NaN where the fp32 kernel gives inf (the samplers refuse non-finite state).
//
// The walk is conv_stem_f16_kernel's (sdc_conv_stem_f16.hip): K layout (one octet of 8 channels per tap, two taps per 16-deep step, NS =
// ceil(7 kH / 2) steps per kd plane), plane-group row staging with zero halo columns, the three fragment bases, the 64 x 256 tile with
// four waves of 2 x 2 32x32 accumulators, the epilogue.  The tile geometry, the common arguments with their host fill, a workgroup's tile
// and the launch ladder are sdc_conv_stem_tile.h's, the split and the term order sdc_split3.h's.  What differs:
//   Weights: Wb[piece][kd][s][co][8 h + ci] bf16 (include/sdc.h, sdc_pack_stem_x3): three planes, each with the layout of sdc_pack_stem_f16.
//   Activations: read as fp32 and split into three pieces while staged (v_cvt_pk_bf16_f32 and exact fp32 subtractions): three LDS images
//     [slot row][col + 6][8] bf16, staged ONCE per kd plane.
//   Stage = SS steps of one kd plane (SS = 5 of the 25 steps of 7x7 taps; all 4 of 1x7 taps): the three weight pieces of a sub-stage are
//     3 * SS * 2 KB = 30 KB beside the activation images (3 * 11.2 KB at the smoke stem, B 64, 32x64x64).  The next sub-stage's weights (and,
//     before a new kd plane, its rows) are loaded into registers before this sub-stage's MFMAs.
//   Per 16-deep step a wave reads 6 weight and 6 activation fragments (12 ds_read_b128) for 24 MFMAs.
// Every stage runs for every tile (a clipped kd adds exact zeros), no K split, no atomics: a sample's bits never depend on its tile
// mates or on the batch.  Epilogue: bias, fp32 stores through the descriptor's strides.
#include "sdc_conv.h"
#include "sdc_conv_stem_tile.h"
#include "sdc_split3.h"

using namespace sdcconv;

namespace {

struct StemX3Args {
    STEM_TILE_ARGS(__bf16, wb)
    int plane;                // bf16 elements of one weight piece: kD * NS * Cout * 16
};

// KH = 7: 7x7 taps per kd plane; KH = 1: 1x7 taps.  ITB: staged positions per thread (NR * W <= ITB * 256).
// The five small terms of a product go to accumulators of their own (sm), added to the main ones once at the end.  Every MFMA rounds
// its accumulator at the accumulator's ulp whatever the size of the term; with one accumulator that is six roundings per 16-deep step
// (measured: 0.9x the fp32 kernel's rms error at K = 2401, but 1.3-1.5x where few k of a step are real: Cin 3, planes of one row), and
// the stem's rounding-order difference then showed in the C4 trajectory against the eager oracle.  With sm the main accumulator is
// rounded once per step and sm's ulp is 2^-8 of it.  128 accumulator registers: one workgroup per CU.
template <int KH, int ITB>
__global__ __launch_bounds__(STEM_NT) __attribute__((amdgpu_waves_per_eu(1))) SDC_NO_DS_MERGE void conv_stem_x3_kernel(const StemX3Args a) {
    constexpr int TAPS = KH * 7;
    constexpr int NS = (TAPS + 1) / 2;                          // 16-deep MFMA steps per kd plane
    constexpr int SS = KH == 7 ? 5 : NS;                        // steps per weight sub-stage
    constexpr int NSUB = NS / SS;
    static_assert(NSUB * SS == NS, "whole sub-stages");
    constexpr int HH = KH - 1;                                  // halo rows per plane group
    constexpr int APC = SS * STEM_BM * 32;                        // bytes of one piece of the A image
    constexpr int ASZ = 3 * APC;
    constexpr int NIA = 3 * SS * STEM_BM * 2;                     // 16-byte A items per sub-stage
    constexpr int ITA = (NIA + STEM_NT - 1) / STEM_NT;
    extern __shared__ __attribute__((aligned(16))) char lds[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, lh = lane >> 5;
    const int W = a.W, RP = W + 6;                              // LDS row pitch in positions
    const int BIMG = a.NR * RP * 16;                            // bytes of one activation image
    const StemTile t = stem_tile(a);
    const int m0 = t.m0, n0 = t.n0, r0 = t.r0, plane0 = t.plane0, oh0 = t.oh0;
    const int GR = a.Hs + HH;                                   // slot rows per plane group

    // ---- per-thread B staging items: (slot row sr, column w), w fastest; bases without the depth-tap part
    int64_t bb[ITB];
    int bod[ITB], bdst[ITB];
    bool bok[ITB];
#pragma unroll
    for (int k = 0; k < ITB; ++k) {
        const int it = tid + k * STEM_NT;
        const int w = it & (W - 1);
        const int sr = it >> a.lgW;
        int pl, ih;
        if (KH == 1) { const int row = r0 + sr; pl = row / a.oH; ih = row - pl * a.oH; }
        else { const int g = sr / GR, q = sr - g * GR; pl = plane0 + g; ih = (g == 0 ? oh0 : 0) - 3 + q; }
        const bool ok = it < a.itemsB && pl < a.B * a.oD && ih >= 0 && ih < a.oH;
        const int b = ok ? pl / a.oD : 0, od = ok ? pl % a.oD : 0, ihc = ok ? ih : 0;
        bok[k] = ok;
        bod[k] = od;
        bb[k] = (int64_t)b * a.xs[0] + (int64_t)od * a.xs[2] + (int64_t)ihc * a.xs[3] + (int64_t)w;
        bdst[k] = ASZ + (sr * RP + w + 3) * 16;
    }
    // ---- per-thread A staging items: 16-byte pieces of the sub-stage's [piece][s][co][16] blocks, in LDS order
    int aoff[ITA];
#pragma unroll
    for (int k = 0; k < ITA; ++k) {
        const int it = tid + k * STEM_NT;
        const int p = it / (SS * 2 * STEM_BM), q = it - p * (SS * 2 * STEM_BM);
        const int s = q / (2 * STEM_BM), r = q - s * (2 * STEM_BM);
        aoff[k] = it < NIA ? p * a.plane + (s * a.Cout + m0) * 16 + r * 8 : 0;      // bf16 elements; + (kd * NS + sub * SS) * Cout * 16 per stage
    }

    float bv[ITB][8];
    uint4 av[ITA];
    auto load_a = [&](int kd, int sub) {
        const int wst = (kd * NS + sub * SS) * a.Cout * 16;
#pragma unroll
        for (int k = 0; k < ITA; ++k) {
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (tid + k * STEM_NT < NIA) v = *reinterpret_cast<const uint4*>(a.wb + wst + aoff[k]);
            av[k] = v;
        }
    };
    auto load_b = [&](int kd) {
        const int dk = kd - a.kD / 2;
#pragma unroll
        for (int k = 0; k < ITB; ++k) {
            const int sd = bod[k] + dk;
            const bool ok = bok[k] && sd >= 0 && sd < a.oD;
            const float* q = a.x + bb[k] + (int64_t)dk * a.xs[2];
#pragma unroll
            for (int i = 0; i < 8; ++i) { bv[k][i] = (ok && i < a.Cin) ? *q : 0.0f; q += a.xs[1]; }
        }
    };
    auto store_a = [&]() {
#pragma unroll
        for (int k = 0; k < ITA; ++k)
            if (tid + k * STEM_NT < NIA) *reinterpret_cast<uint4*>(lds + (tid + k * STEM_NT) * 16) = av[k];
    };
    auto store_b = [&]() {
#pragma unroll
        for (int k = 0; k < ITB; ++k) {
            if (tid + k * STEM_NT < a.itemsB) {
                bf16x8 h, m, l;
                split3x8(bv[k], h, m, l);
                *reinterpret_cast<bf16x8*>(lds + bdst[k]) = h;
                *reinterpret_cast<bf16x8*>(lds + bdst[k] + BIMG) = m;
                *reinterpret_cast<bf16x8*>(lds + bdst[k] + 2 * BIMG) = l;
            }
        }
    };

    // zero halo columns 0..2 and W+3..W+5 of every slot row of the three images (never overwritten: the staged columns are 3..W+2)
    for (int e = tid; e < 3 * a.NR * 6; e += STEM_NT) {
        const int sr = e / 6, c = e - sr * 6;                   // sr runs over the 3 * NR rows of the three images (BIMG = NR rows)
        *reinterpret_cast<uint4*>(lds + ASZ + (sr * RP + (c < 3 ? c : W + c)) * 16) = make_uint4(0u, 0u, 0u, 0u);
    }

    // fragment bases (first image): B position (wave * 64 + 32 j + l31) of the tile.  Lane half h reads tap 2 s + h:
    //   bA: both taps in one kh row (h adds one column);  bB: the pair straddles two kh rows (tap 2 s is kw = 6, tap 2 s + 1 is kw = 0
    //   of the next row);  bC: the last step, whose second tap does not exist (the upper lanes read the zero column 0 of slot row 0)
    int bA[2], bB[2], bC[2];
    constexpr int LAST_OFF = 16 * 6;                            // tap TAPS - 1 = (KH - 1, 6): + (KH - 1) rows
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int p = wave * 64 + 32 * j + l31;
        const bool pok = n0 + p < a.Ntot;
        const int rl = pok ? p >> a.lgW : 0, col = pok ? p & (W - 1) : 0;
        int slot;
        if (KH == 1) slot = rl;
        else {
            const int row = r0 + rl, pl = row / a.oH, oh = row - pl * a.oH, g = pl - plane0;
            slot = g * GR + oh - (g == 0 ? oh0 : 0);
        }
        const int base = ASZ + (slot * RP + col) * 16;
        bA[j] = base + 16 * lh;
        bB[j] = base + lh * (RP * 16 - 16 * 6);
        bC[j] = lh ? ASZ - (HH * RP * 16 + LAST_OFF) : base;
    }
    const int aoffr = l31 * 32 + 16 * lh;
    const int rowb = RP * 16;

    f32x16 acc[2][2], sm[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                acc[i][j][r] = 0.0f;
                sm[i][j][r] = 0.0f;
            }

    load_a(0, 0);
    load_b(0);
    for (int kd = 0; kd < a.kD; ++kd) {
#pragma unroll
        for (int sub = 0; sub < NSUB; ++sub) {
            __syncthreads();                                    // the previous sub-stage's fragments are read
            store_a();
            if (sub == 0) store_b();
            __syncthreads();
            if (sub + 1 < NSUB) load_a(kd, sub + 1);            // in flight during this sub-stage's MFMAs
            else if (kd + 1 < a.kD) { load_a(kd + 1, 0); load_b(kd + 1); }
#pragma unroll
            for (int sl = 0; sl < SS; ++sl) {
                const int s = sub * SS + sl;
                const int t0 = 2 * s, kh = t0 / 7, kw = t0 - 7 * kh;
                const int tb = kh * rowb + kw * 16;
                bf16x8 af[2][3], bf[2][3];
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int p = 0; p < 3; ++p)
                        af[i][p] = *reinterpret_cast<const bf16x8*>(lds + p * APC + (sl * STEM_BM + 32 * i) * 32 + aoffr);
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int bs = (s == NS - 1) ? bC[j] : (kw == 6 ? bB[j] : bA[j]);
#pragma unroll
                    for (int p = 0; p < 3; ++p) bf[j][p] = *reinterpret_cast<const bf16x8*>(lds + bs + tb + p * BIMG);
                }
                // the six terms in sdc_split3.h's order (smallest first); the four accumulators take each term in turn
#pragma unroll
                for (int t = 0; t < 6; ++t)
#pragma unroll
                    for (int i = 0; i < 2; ++i)
#pragma unroll
                        for (int j = 0; j < 2; ++j) {
                            f32x16& c = t < 5 ? sm[i][j] : acc[i][j];
                            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i][X3_PA[t]], bf[j][X3_PB[t]], c, 0, 0, 0);
                        }
            }
        }
    }

#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] += sm[i][j];
    // ---- epilogue: bias, fp32 store.  The 32 bias values of a lane are loaded in one batch under a wave-uniform condition (a load
    // per stored element under the per-lane bounds condition compiles to 32 dependent round trips)
    float bz[2][16];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) bz[i][rr] = 0.0f;
    if (a.bias) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) bz[i][rr] = a.bias[m0 + 32 * i + 4 * lh + (rr & 3) + 8 * (rr >> 2)];      // (Cout % 64 == 0: in range)
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int p = n0 + wave * 64 + 32 * j + l31;
        if (p >= a.Ntot) continue;
        const int row = p >> a.lgW, col = p & (W - 1);
        const int pl = row / a.oH, oh = row - pl * a.oH;
        const int b = pl / a.oD, od = pl - b * a.oD;
        float* yp = a.y + (int64_t)b * a.ys[0] + (int64_t)od * a.ys[2] + (int64_t)oh * a.ys[3] + (int64_t)col
                    + (int64_t)(m0 + 4 * lh) * a.ys[1];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
#pragma unroll
            for (int rr = 0; rr < 16; ++rr)
                yp[(int64_t)(32 * i + (rr & 3) + 8 * (rr >> 2)) * a.ys[1]] = acc[i][j][rr] + bz[i][rr];
        }
    }
}

// Wb[piece][kd][s][co][8 h + ci]: the three bf16 pieces of w[co][ci][kd][tap = 2 s + h], zero for tap >= 7 kH and for ci >= Cin; one
// thread per element of a plane
__global__ __launch_bounds__(256) void pack_stem_x3_kernel(const float* __restrict__ w, __bf16* __restrict__ out, int Cout, int Cin, int kD,
                                                           int taps, int NS, int64_t n) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const int ci = (int)(e & 7), h = (int)((e >> 3) & 1);
    int64_t r = e >> 4;
    const int co = (int)(r % Cout); r /= Cout;
    const int s = (int)(r % NS);
    const int kd = (int)(r / NS);
    const int t = 2 * s + h;
    const float v = (ci < Cin && t < taps) ? w[(((int64_t)co * Cin + ci) * kD + kd) * taps + t] : 0.0f;
    __bf16 ph, pm, pl;
    split3(v, ph, pm, pl);
    out[e] = ph; out[n + e] = pm; out[2 * n + e] = pl;
}

}  // namespace

namespace sdcconv {

int launch_stem_x3(const SdcConvDesc& d, const float* x, const __bf16* wb, const float* bias, float* y, hipStream_t s) {
    SDC_REQUIRE(reinterpret_cast<uintptr_t>(wb) % 16 == 0, SDC_EALIGN, "sdc_conv_stem_x3: the packed weight buffer must be 16-byte aligned");
    const StemShape sh = stem_shape(d);
    const int NS = (d.kH * 7 + 1) / 2, SS = d.kH == 7 ? 5 : NS;
    const size_t lds = (size_t)3 * SS * STEM_BM * 32 + (size_t)3 * sh.NR * (d.oW + 6) * 16;
    // (every descriptor that stem_f16_ok covers stages at most 2048 positions; three images of at most 40 KB and 30 KB of weights)
    SDC_REQUIRE(sh.itemsB <= 8 * STEM_NT && lds <= 160u * 1024u, SDC_EINVAL, "sdc_conv_stem_x3: staging of %d positions / %zu bytes of LDS",
                sh.itemsB, lds);
    StemX3Args a;
    a.wb = wb;
    if (const int rc = stem_fill_args("sdc_conv_stem_x3", d, sh, x, bias, y, a)) return rc;
    const int64_t plane = (int64_t)d.kD * NS * d.Cout * 16;
    SDC_REQUIRE(3 * plane < (1ll << 31), SDC_EINVAL, "sdc_conv_stem_x3: weight too large");
    a.plane = (int)plane;
    STEM_LAUNCH(conv_stem_x3_kernel, "sdc_conv_stem_x3");
    return sdc::check_launch("sdc_conv_stem_x3");
}

}  // namespace sdcconv

// (the tap shapes and channel counts of sdc_pack_stem_f16_bytes: three planes of that layout, two bytes per element either way)
extern "C" size_t sdc_pack_stem_x3_bytes(int Cout, int Cin, int kD, int kH, int kW) {
    return 3 * sdc_pack_stem_f16_bytes(Cout, Cin, kD, kH, kW);
}

extern "C" int sdc_pack_stem_x3(const float* w, void* out, int Cout, int Cin, int kD, int kH, int kW, void* stream) {
    SDC_REQUIRE(w && out, SDC_ENULL, "sdc_pack_stem_x3: null pointer");
    SDC_REQUIRE(sdc_pack_stem_x3_bytes(Cout, Cin, kD, kH, kW) > 0, SDC_EINVAL,
                "sdc_pack_stem_x3: taps 1x1x7, 1x7x7 or 7x7x7 and 1 <= Cin <= 8 (got %dx%dx%d, Cin %d, Cout %d)", kD, kH, kW, Cin, Cout);
    const int NS = (kH * 7 + 1) / 2;
    const int64_t n = (int64_t)kD * NS * Cout * 16;
    SDC_REQUIRE(n / 256 + 1 < (1ll << 31), SDC_EINVAL, "sdc_pack_stem_x3: weight too large");
    hipLaunchKernelGGL(pack_stem_x3_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, sdc::as_stream(stream), w,
                       reinterpret_cast<__bf16*>(out), Cout, Cin, kD, kH * 7, NS, n);
    return sdc::check_launch("sdc_pack_stem_x3");
}
