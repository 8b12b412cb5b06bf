// net.stem_f16 (opt-in, samplers only): the 7-tap stem convs -- Conv1d k7 (1x1x7), Conv2d 7x7 (1x7x7) and Conv3d 7x7x7, Cin <= 8, 'same'
// padding -- as a direct-form implicit GEMM on v_mfma_f32_32x32x16_f16: fp16 operands (RNE), fp32 accumulation, fp32 activations in HBM.
//
//   D[co][p] = sum_k Wh[k][co] * X[k][p],   k = (kd, tap = kh * 7 + kw, ci),  p = (b, od, oh, ow) flattened
//
// K layout.  Cin is zero-padded to one octet of 8 channels, so a lane's eight consecutive k values for one position are the eight
// channels of ONE (kh, kw) tap: one ds_read_b128.  A 16-deep MFMA step covers the taps (2 s, 2 s + 1) of the (kh, kw) walk flattened
// to tap = kh * 7 + kw: NS = ceil(7 kH / 2) steps per kd plane (25 for 7x7 taps: 400 issued k for 392; 4 for 1x7 taps: 64 for 56).
// The one tap past the end (49, or 7) has zero weights, and its lanes read a zero LDS entry.
//
// Weights: Wh[kd][s][co][16] halves (include/sdc.h, sdc_pack_stem_f16), element (8 h + ci) = w[co][ci][kd][tap = 2 s + h].  One kd
// plane of 64 output channels is NS blocks of 2 KB; it is staged as it lies: LDS A image [s][co][16].
// Activations: the input rows that a tile's kh taps reach, staged ONCE per kd plane as fp16 [slot row][col + 6][8] (16 bytes per
// position: contiguous, so a fragment read of 32 consecutive columns is one 512-byte run), three zero columns at either row end.
// The (kh, kw) shift of the implicit GEMM is an LDS offset, (kh * (W + 6) + kw) positions.
//
// Tile: 64 output channels x 256 positions = R = 256 / W whole rows of the flattened (b, od, oh) row walk; 4 waves of 2 x 2
// 32 x 32 accumulators (as conv_f16_kernel).  The tile's rows may lie in several (sample, depth) planes: plane g of the tile (g = 0 ..
// NG - 1) owns a group of Hs + 6 slot rows, Hs = min(oH, R), holding input rows base_g - 3 .. base_g + Hs + 2 of that plane (base_g =
// the tile's first row in the plane).  Rows outside the plane, planes outside the depth range of this kd and padded channels are
// staged as zeros; every stage runs for every tile (a clipped kd adds exact zeros), so the k order of a position's accumulator, and
// with it a sample's bits, never depend on its tile mates or on the batch.
// Stage = one kd plane: the next plane's global loads (weights and rows) are issued before this plane's MFMAs; two workgroups per CU.
// No K split, no atomics.  Epilogue: bias, fp32 stores through the descriptor's strides.
// The tile geometry, the common arguments with their host fill, a workgroup's tile and the launch ladder are in sdc_conv_stem_tile.h,
// shared with the bf16-split variant (sdc_conv_stem_x3.hip).
#include "sdc_conv.h"
#include "sdc_conv_stem_tile.h"
#include "sdc_f16frag.h"

using namespace sdcconv;

namespace {

struct StemArgs { STEM_TILE_ARGS(_Float16, wh) };

// KH = 7: 7x7 taps per kd plane; KH = 1: 1x7 taps.  ITB: staged positions per thread (NR * W <= ITB * 256)
template <int KH, int ITB>
__global__ __launch_bounds__(STEM_NT) __attribute__((amdgpu_waves_per_eu(ITB > 4 ? 1 : 2))) SDC_NO_DS_MERGE void conv_stem_f16_kernel(const StemArgs a) {
    constexpr int TAPS = KH * 7;
    constexpr int NS = (TAPS + 1) / 2;                          // 16-deep MFMA steps per kd plane
    constexpr int HH = KH - 1;                                  // halo rows per plane group
    constexpr int ASZ = NS * STEM_BM * 32;                        // bytes of the A image
    constexpr int ITA = (NS * STEM_BM * 2 + STEM_NT - 1) / STEM_NT;   // 16-byte A items per thread
    extern __shared__ __attribute__((aligned(16))) char lds[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, lh = lane >> 5;
    const int W = a.W, RP = W + 6;                              // LDS row pitch in positions
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
    // ---- per-thread A staging items: 16-byte pieces of the plane's NS blocks [co][16], in LDS order
    int aoff[ITA];
#pragma unroll
    for (int k = 0; k < ITA; ++k) {
        const int it = tid + k * STEM_NT;
        const int s = it / (2 * STEM_BM), r = it - s * (2 * STEM_BM);
        aoff[k] = (s * a.Cout + m0) * 16 + r * 8;               // halves; + kd * NS * Cout * 16 per stage
    }

    float bv[ITB][8];
    uint4 av[ITA];
    auto load_stage = [&](int kd) {
        const int64_t wst = (int64_t)kd * NS * a.Cout * 16;
#pragma unroll
        for (int k = 0; k < ITA; ++k) {
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (tid + k * STEM_NT < NS * STEM_BM * 2) v = *reinterpret_cast<const uint4*>(a.wh + wst + aoff[k]);
            av[k] = v;
        }
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
    auto store_stage = [&]() {
#pragma unroll
        for (int k = 0; k < ITA; ++k)
            if (tid + k * STEM_NT < NS * STEM_BM * 2) *reinterpret_cast<uint4*>(lds + (tid + k * STEM_NT) * 16) = av[k];
#pragma unroll
        for (int k = 0; k < ITB; ++k) {
            if (tid + k * STEM_NT < a.itemsB) {
                half8 h;
#pragma unroll
                for (int i = 0; i < 8; ++i) h[i] = (_Float16)bv[k][i];       // RNE (v_cvt_pk_f16_f32)
                *reinterpret_cast<half8*>(lds + bdst[k]) = h;
            }
        }
    };

    // zero halo columns 0..2 and W+3..W+5 of every slot row (never overwritten: the staged columns are 3..W+2)
    for (int e = tid; e < a.NR * 6; e += STEM_NT) {
        const int sr = e / 6, c = e - sr * 6;
        *reinterpret_cast<uint4*>(lds + ASZ + (sr * RP + (c < 3 ? c : W + c)) * 16) = make_uint4(0u, 0u, 0u, 0u);
    }

    // fragment bases: B position (wave * 64 + 32 j + l31) of the tile.  Lane half h reads tap 2 s + h:
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

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    load_stage(0);
    for (int kd = 0; kd < a.kD; ++kd) {
        __syncthreads();                                        // the previous stage's fragments are read
        store_stage();
        __syncthreads();
        if (kd + 1 < a.kD) load_stage(kd + 1);                  // in flight during this stage's MFMAs
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int t0 = 2 * s, kh = t0 / 7, kw = t0 - 7 * kh;
            const int tb = kh * rowb + kw * 16;
            half8 af[2], bf[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) af[i] = *reinterpret_cast<const half8*>(lds + (s * STEM_BM + 32 * i) * 32 + aoffr);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int bs = (s == NS - 1) ? bC[j] : (kw == 6 ? bB[j] : bA[j]);
                bf[j] = *reinterpret_cast<const half8*>(lds + bs + tb);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[i], bf[j], acc[i][j], 0, 0, 0);
        }
    }

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

// Wh[kd][s][co][8 h + ci] = (fp16, RNE) w[co][ci][kd][tap = 2 s + h], zero for tap >= 7 kH and for ci >= Cin; one thread per half
__global__ __launch_bounds__(256) void pack_stem_f16_kernel(const float* __restrict__ w, _Float16* __restrict__ out, int Cout, int Cin, int kD,
                                                            int taps, int NS, int64_t n) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const int ci = (int)(e & 7), h = (int)((e >> 3) & 1);
    int64_t r = e >> 4;
    const int co = (int)(r % Cout); r /= Cout;
    const int s = (int)(r % NS);
    const int kd = (int)(r / NS);
    const int t = 2 * s + h;
    out[e] = (ci < Cin && t < taps) ? (_Float16)w[(((int64_t)co * Cin + ci) * kD + kd) * taps + t] : (_Float16)0.0f;
}

bool stem_taps_ok(int Cin, int kD, int kH, int kW) {
    return kW == 7 && ((kD == 1 && kH == 1) || (kD == 1 && kH == 7) || (kD == 7 && kH == 7)) && Cin >= 1 && Cin <= 8;
}

}  // namespace

namespace sdcconv {

StemShape stem_shape(const SdcConvDesc& d) {
    StemShape sh{};
    const int W = d.oW, R = STEM_BN / W, NS = (d.kH * 7 + 1) / 2;
    if (d.kH == 1) { sh.Hs = R; sh.NG = 1; }
    else {
        sh.Hs = d.oH < R ? d.oH : R;
        // tiles start at multiples of R rows: aligned with the planes when oH divides R or R divides oH; else a tile's R rows
        // touch at most (R - 1) / oH + 2 planes
        const bool al = d.oH % R == 0 || R % d.oH == 0;
        sh.NG = al ? (d.oH >= R ? 1 : R / d.oH) : (R - 1) / d.oH + 2;
    }
    sh.NR = sh.NG * (sh.Hs + d.kH - 1);
    sh.itemsB = sh.NR * W;
    sh.lds = (size_t)NS * STEM_BM * 32 + (size_t)sh.NR * (W + 6) * 16;
    return sh;
}

int launch_stem_f16(const SdcConvDesc& d, const float* x, const _Float16* wh, const float* bias, float* y, hipStream_t s) {
    SDC_REQUIRE(reinterpret_cast<uintptr_t>(wh) % 16 == 0, SDC_EALIGN, "sdc_conv_stem_f16: the packed weight buffer must be 16-byte aligned");
    const StemShape sh = stem_shape(d);
    // (every descriptor that stem_f16_ok covers stages at most 2048 positions in at most 91 KB of LDS)
    SDC_REQUIRE(sh.itemsB <= 8 * STEM_NT && sh.lds <= 160u * 1024u, SDC_EINVAL, "sdc_conv_stem_f16: staging of %d positions / %zu bytes of LDS",
                sh.itemsB, sh.lds);
    StemArgs a;
    a.wh = wh;
    if (const int rc = stem_fill_args("sdc_conv_stem_f16", d, sh, x, bias, y, a)) return rc;
    const size_t lds = sh.lds;
    STEM_LAUNCH(conv_stem_f16_kernel, "sdc_conv_stem_f16");
    return sdc::check_launch("sdc_conv_stem_f16");
}

}  // namespace sdcconv

extern "C" size_t sdc_pack_stem_f16_bytes(int Cout, int Cin, int kD, int kH, int kW) {
    if (Cout <= 0 || !stem_taps_ok(Cin, kD, kH, kW)) return 0;
    return (size_t)kD * ((kH * 7 + 1) / 2) * Cout * 16 * sizeof(_Float16);
}

extern "C" int sdc_pack_stem_f16(const float* w, void* out, int Cout, int Cin, int kD, int kH, int kW, void* stream) {
    SDC_REQUIRE(w && out, SDC_ENULL, "sdc_pack_stem_f16: null pointer");
    SDC_REQUIRE(Cout > 0 && stem_taps_ok(Cin, kD, kH, kW), SDC_EINVAL,
                "sdc_pack_stem_f16: taps 1x1x7, 1x7x7 or 7x7x7 and 1 <= Cin <= 8 (got %dx%dx%d, Cin %d, Cout %d)", kD, kH, kW, Cin, Cout);
    const int NS = (kH * 7 + 1) / 2;
    const int64_t n = (int64_t)kD * NS * Cout * 16;
    SDC_REQUIRE(n / 256 + 1 < (1ll << 31), SDC_EINVAL, "sdc_pack_stem_f16: weight too large");
    hipLaunchKernelGGL(pack_stem_f16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, sdc::as_stream(stream), w,
                       reinterpret_cast<_Float16*>(out), Cout, Cin, kD, kH * 7, NS, n);
    return sdc::check_launch("sdc_pack_stem_f16");
}
