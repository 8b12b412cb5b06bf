// precision = 6 (opt-in, samplers only): the stride-1 pad-1 3-tap convs -- Conv1d k3 (1x1x3), Conv2d 3x3 (1x3x3) and Conv3d
// 3x3x3 -- as a direct-form implicit GEMM on the gfx950 16-bit matrix pipe, v_mfma_f32_32x32x16_f16: fp16 operands, fp32
// accumulation, fp32 activations in HBM.
//
//   D[co][p] = sum_k Wh[k][co] * X[k][p],   k = (tap, ci),  p = (b, od, oh, ow) flattened
//
// Operands.  The weights come pre-rounded (RNE) from the tail of the packed buffer (include/sdc.h, precision 6):
// Wh[tap][ci / KC][co][ci % KC], Cin zero-padded to whole KC chunks, so a (tap, chunk) block of 64 output channels is 64 * KC
// contiguous halves.  Activations are read as fp32 and rounded to fp16 once (RNE, v_cvt_pk_f16_f32) while they are staged.
// Every fp16 x fp16 product is exact in fp32, so the result differs from an fp64 conv of the ROUNDED operands by the fp32
// accumulation order only.
//
// Tile: 64 output channels x 256 output positions = R = 256 / W whole rows of width W (16 / 32 / 64 / 128) per 256-thread
// workgroup; each of the 4 waves owns 64 channels x 64 positions (2 x 2 blocks of 32 x 32 accumulators: two A and two B
// fragments feed four MFMAs).  Stage = (kd, chunk of KC input channels): the input rows that the tile's kh taps reach -- the
// tile's rows plus a halo row above and below every run of rows inside one (sample, depth) plane, and a zero halo column on
// either side -- are staged ONCE into LDS as fp16 [row][col][KC] (16-byte channel octets); the (kh, kw) tap shift of the
// implicit GEMM is then an LDS offset, (kh * (W + 2) + kw) positions.  A (weights) is staged as [tap][co][KC].  Both images
// have a pitch of 2 KC + 16 bytes per position / channel: every ds_read_b128 lane group of a fragment read then hits 16
// distinct 4-bank quads.  KC = 32 (two k-steps per tap): 72 MFMAs per wave and stage for the 3x3 / 3x3x3 convs (9 taps), 24 for
// the 1-D ones (3 taps) -- with KC = 16 (36 MFMAs) a stage was too short to cover its successor's global-load latency.  One LDS
// image, staged from registers: the next stage's global loads are issued before the MFMAs of the current one; two workgroups per
// CU overlap one's staging with the other's MFMAs.
//
// The output of a position never depends on other positions or on the batch (no K split across workgroups; the k order of
// every accumulator is fixed), so a sample's bits do not depend on the batch it rides in.
// Epilogue as sdc_conv: bias, optional fp32 residual, fp32 output through the descriptor's strides, and (sdc_conv_gn) the fp64
// GroupNorm partial sums where the tile grid lines up with (sample, group): S % 256 == 0, or whole samples of 64 / 128 positions per tile.
#include "sdc_conv.h"
#include "sdc_f16frag.h"

using namespace sdcconv;

namespace {

constexpr int F16_BM = 64, F16_BN = 256, F16_NT = 256;

struct F16Args {
    const float* x0;
    const float* x1;
    const _Float16* wh;
    const float* bias;
    const float* res;
    float* y;
    double* gn_part;
    const int32_t* gexp;      // SCALED (data gradient of fine-tuning precision 6 / 7): exponent e of sdc_f16_grad_exponent
    int64_t x0s[5], x1s[5], ys[5], rs[5];
    int B, Cin0, Cin, Cout, oD, oH, W, lgW;
    int pD, kD;
    int R, Hs, NR;            // rows per tile, rows per halo'd run (one plane's share), staged rows
    int nchunks, nstages;     // KC chunks of Cin, kD * nchunks
    int Ntot, nrows, ntiles, mtiles;
    int itemsB;               // (channel octet, staged row, column) items of one B stage
    int ldsB;                 // byte offset of the B image
    int gn_G, gn_cpg, gn_nparts, gn_S;
};

// KH = 3: 3x3 / 3x3x3 taps (9 taps per stage); KH = 1: 1x3 taps (3 taps per stage)
// ITB: B staging items per thread; 8 (rows of 128, or planes of 1-2 rows at rows of 16: more staged rows) takes more registers
// and LDS than two workgroups per CU leave, and runs one
// SCALED (sdc_conv_dgrad_f16 only): the activations -- a loss gradient -- are multiplied by 2^e before they are rounded and the
// accumulators by 2^-e in the epilogue (both exact), e read from device memory; the samplers' instances are the unscaled ones
template <int KH, int ITB, bool SCALED = false>
__global__ __launch_bounds__(F16_NT) __attribute__((amdgpu_waves_per_eu(ITB > 6 ? 1 : 2))) SDC_NO_DS_MERGE void conv_f16_kernel(const F16Args a) {
    constexpr int KC = 32;
    constexpr int NTAP = 3 * KH;
    constexpr int PITCH = 2 * KC + 16;                          // bytes per LDS position / channel row
    constexpr int OCT = KC / 8;                                 // 16-byte channel octets per position
    constexpr int ITA = (NTAP * F16_BM * OCT + F16_NT - 1) / F16_NT;
    constexpr int HH = KH - 1;                                  // halo rows per run
    extern __shared__ __attribute__((aligned(16))) char lds[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, lh = lane >> 5;
    const int W = a.W;
    const int logical = xcd_tile(blockIdx.x, a.ntiles * a.mtiles);
    const int mt = logical % a.mtiles, nt = logical / a.mtiles;
    const int m0 = mt * F16_BM, n0 = nt * F16_BN;
    const int r0 = n0 >> a.lgW;
    float gsc = 1.0f, gunsc = 1.0f;
    if (SCALED) { const int e = *a.gexp; gsc = __builtin_ldexpf(1.0f, e); gunsc = __builtin_ldexpf(1.0f, -e); }

    // ---- per-thread B staging items: (octet o, staged row sr, column w), w fastest; bases without the channel / depth-tap part
    int64_t bb0[ITB], bb1[ITB];
    int bod[ITB], boct[ITB], bdst[ITB];
    bool bok[ITB];
#pragma unroll
    for (int k = 0; k < ITB; ++k) {
        const int it = tid + k * F16_NT;
        const int w = it & (W - 1);
        const int tmp = it >> a.lgW;
        const int sr = tmp % a.NR, o = tmp / a.NR;
        const int seg = sr / (a.Hs + HH), q = sr - seg * (a.Hs + HH);
        const int rs = r0 + seg * a.Hs;
        int row, sh;
        if (KH == 3) { row = rs; sh = rs % a.oH + q - 1; }
        else { row = rs + q; sh = row % a.oH; }
        const int pl = row / a.oH;
        const bool ok = it < a.itemsB && pl < a.B * a.oD && sh >= 0 && sh < a.oH;
        const int b = ok ? pl / a.oD : 0, od = ok ? pl % a.oD : 0, shc = ok ? sh : 0;
        bok[k] = ok;
        bod[k] = od;
        boct[k] = o;
        bb0[k] = (int64_t)b * a.x0s[0] + (int64_t)od * a.x0s[2] + (int64_t)shc * a.x0s[3] + (int64_t)w * a.x0s[4];
        bb1[k] = (int64_t)b * a.x1s[0] + (int64_t)od * a.x1s[2] + (int64_t)shc * a.x1s[3] + (int64_t)w * a.x1s[4];
        bdst[k] = a.ldsB + ((sr * (W + 2) + w + 1) * PITCH) + 16 * o;
    }
    // ---- per-thread A staging items: (octet o, channel row co, tap t), o fastest: 16-byte loads of contiguous global blocks
    int aoff[ITA], adst[ITA];
    bool aok[ITA];
#pragma unroll
    for (int k = 0; k < ITA; ++k) {
        const int it = tid + k * F16_NT;
        const int o = it % OCT, co = (it / OCT) % F16_BM, t = it / (OCT * F16_BM);
        aok[k] = it < NTAP * F16_BM * OCT && m0 + co < a.Cout;
        aoff[k] = ((t * a.nchunks) * a.Cout + m0 + co) * KC + 8 * o;       // + (kd * NTAP * nchunks + chunk) * Cout * KC per stage
        adst[k] = (t * F16_BM + co) * PITCH + 16 * o;
    }

    float bv[ITB][8];
    uint4 av[ITA];
    auto load_stage = [&](int s) {
        const int kd = s / a.nchunks, cc = s - kd * a.nchunks;
        const int ci0 = cc * KC;
        const int64_t wst = ((int64_t)kd * NTAP * a.nchunks + cc) * a.Cout * KC;
#pragma unroll
        for (int k = 0; k < ITA; ++k) {
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (aok[k]) v = *reinterpret_cast<const uint4*>(a.wh + wst + aoff[k]);
            av[k] = v;
        }
        const int dk = kd - a.pD;
#pragma unroll
        for (int k = 0; k < ITB; ++k) {
            const int cb = ci0 + 8 * boct[k];
            const int sd = bod[k] + dk;
            const bool ok = bok[k] && cb < a.Cin && sd >= 0 && sd < a.oD;
            const bool use1 = cb >= a.Cin0;                     // (octets never straddle the two inputs: Cin1 == 0 or Cin0 % 8 == 0)
            const float* p = use1 ? a.x1 + bb1[k] + (int64_t)dk * a.x1s[2] + (int64_t)(cb - a.Cin0) * a.x1s[1]
                                  : a.x0 + bb0[k] + (int64_t)dk * a.x0s[2] + (int64_t)cb * a.x0s[1];
            const int64_t cs = use1 ? a.x1s[1] : a.x0s[1];
            const float* q = p;
#pragma unroll
            for (int i = 0; i < 8; ++i) { bv[k][i] = (ok && cb + i < a.Cin) ? *q : 0.0f; q += cs; }
        }
    };
    auto store_stage = [&]() {
#pragma unroll
        for (int k = 0; k < ITA; ++k)
            if (tid + k * F16_NT < NTAP * F16_BM * OCT) *reinterpret_cast<uint4*>(lds + adst[k]) = av[k];
#pragma unroll
        for (int k = 0; k < ITB; ++k) {
            if (tid + k * F16_NT < a.itemsB) {
                half8 h;
#pragma unroll
                for (int i = 0; i < 8; ++i) h[i] = (_Float16)(SCALED ? bv[k][i] * gsc : bv[k][i]);   // RNE (v_cvt_pk_f16_f32)
                *reinterpret_cast<half8*>(lds + bdst[k]) = h;
            }
        }
    };

    // zero halo columns (never overwritten: the staged columns are 1..W)
    for (int e = tid; e < a.NR * 2 * OCT; e += F16_NT) {
        const int o = e % OCT, sc = e / OCT, sr = sc >> 1, col = (sc & 1) ? W + 1 : 0;
        *reinterpret_cast<uint4*>(lds + a.ldsB + (sr * (W + 2) + col) * PITCH + 16 * o) = make_uint4(0u, 0u, 0u, 0u);
    }

    // fragment offsets: A row (32 i + l31), k half lh; B position (wave * 64 + 32 j + l31) of the tile
    int boff[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int p = wave * 64 + 32 * j + l31;
        const int rl = p >> a.lgW, col = p & (W - 1);
        const int srow = (rl / a.Hs) * (a.Hs + HH) + rl % a.Hs;
        boff[j] = a.ldsB + (srow * (W + 2) + col) * PITCH + 16 * lh;
    }
    const int aoffr = l31 * PITCH + 16 * lh;
    const int rowb = (W + 2) * PITCH;

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    load_stage(0);
    for (int s = 0; s < a.nstages; ++s) {
        __syncthreads();                                        // the previous stage's fragments are read
        store_stage();
        __syncthreads();
        if (s + 1 < a.nstages) load_stage(s + 1);               // in flight during this stage's MFMAs
#pragma unroll
        for (int t = 0; t < NTAP; ++t) {
            const int kh = t / 3, kw = t - 3 * kh;
            const int tb = kh * rowb + kw * PITCH;
#pragma unroll
            for (int ks = 0; ks < KC / 16; ++ks) {
                half8 af[2], bf[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) af[i] = *reinterpret_cast<const half8*>(lds + (t * F16_BM + 32 * i) * PITCH + aoffr + 32 * ks);
#pragma unroll
                for (int j = 0; j < 2; ++j) bf[j] = *reinterpret_cast<const half8*>(lds + boff[j] + tb + 32 * ks);
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[i], bf[j], acc[i][j], 0, 0, 0);
            }
        }
    }

    // ---- epilogue: bias, residual, fp32 store; GroupNorm partial sums of the stored values in fp64
    const bool gn = a.gn_part != nullptr;
    double gs[2][4], gq[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int b4 = 0; b4 < 4; ++b4) { gs[i][b4] = 0.0; gq[i][b4] = 0.0; }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int p = n0 + wave * 64 + 32 * j + l31;
        const bool pok = p < a.Ntot;
        const int pc = pok ? p : 0;
        const int row = pc >> a.lgW, col = pc & (W - 1);
        const int pl = row / a.oH, oh = row - pl * a.oH;
        const int b = pl / a.oD, od = pl - b * a.oD;
        const int64_t yoff = (int64_t)b * a.ys[0] + (int64_t)od * a.ys[2] + (int64_t)oh * a.ys[3] + (int64_t)col * a.ys[4];
        const int64_t roff = (int64_t)b * a.rs[0] + (int64_t)od * a.rs[2] + (int64_t)oh * a.rs[3] + (int64_t)col * a.rs[4];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) {
                const int co = m0 + 32 * i + 4 * lh + (rr & 3) + 8 * (rr >> 2);
                if (pok && co < a.Cout) {
                    float v = (SCALED ? acc[i][j][rr] * gunsc : acc[i][j][rr]) + (a.bias ? a.bias[co] : 0.0f);
                    if (a.res) v = v + a.res[roff + (int64_t)co * a.rs[1]];
                    a.y[yoff + (int64_t)co * a.ys[1]] = v;
                    if (gn) { gs[i][rr >> 2] += (double)v; gq[i][rr >> 2] += (double)v * v; }
                }
            }
        }
    }
    if (gn) {
        __syncthreads();                                        // the LDS images are dead: reuse them as the reduction scratch
        double* scr = reinterpret_cast<double*>(lds);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int b4 = 0; b4 < 4; ++b4) {
                const double s1 = sdc::wave_sum(gs[i][b4]), q1 = sdc::wave_sum(gq[i][b4]);
                if (lane == 0) { scr[(wave * 8 + i * 4 + b4) * 2] = s1; scr[(wave * 8 + i * 4 + b4) * 2 + 1] = q1; }
            }
        __syncthreads();
        const int ngl = a.gn_cpg >= F16_BM ? 1 : F16_BM / a.gn_cpg;     // groups inside this workgroup's rows
        const int nsl = a.gn_S >= F16_BN ? 1 : F16_BN / a.gn_S;           // samples inside its positions (S = 64 / 128: whole samples per wave)
        if (tid < ngl * nsl) {
            const int gl = tid % ngl, sl = tid / ngl;
            const int lr0 = a.gn_cpg >= F16_BM ? 0 : gl * a.gn_cpg, lr1 = a.gn_cpg >= F16_BM ? F16_BM : lr0 + a.gn_cpg;
            double s = 0.0, q = 0.0;
            for (int blk = lr0 / 8; blk < lr1 / 8; ++blk)
                for (int wv = 0; wv < 4; ++wv)
                    if (nsl == 1 || (wv * 64) / a.gn_S == sl) { s += scr[(wv * 8 + blk) * 2]; q += scr[(wv * 8 + blk) * 2 + 1]; }
            if (m0 + lr0 < a.Cout && n0 + sl * a.gn_S < a.Ntot) {
                const int g = (m0 + lr0) / a.gn_cpg;
                const int b = n0 / a.gn_S + sl, ntl = nsl > 1 ? 0 : (n0 - b * a.gn_S) / F16_BN;
                const int idx = a.gn_cpg >= F16_BM ? ntl * (a.gn_cpg / F16_BM) + (m0 - g * a.gn_cpg) / F16_BM : ntl;
                double* pp = a.gn_part + (((int64_t)b * a.gn_G + g) * a.gn_nparts + idx) * 2;
                pp[0] = s; pp[1] = q;
            }
        }
    }
}

struct F16Shape { int R, Hs, NR, itemsB; size_t lds; };

F16Shape f16_shape(const SdcConvDesc& d) {
    F16Shape sh{};
    const int W = d.oW, KC = 32, NTAP = 3 * d.kH, pitch = 2 * KC + 16;
    sh.R = F16_BN / W;
    sh.Hs = d.kH == 3 ? (d.oH < sh.R ? d.oH : sh.R) : sh.R;
    sh.NR = (sh.R / sh.Hs) * (sh.Hs + d.kH - 1);
    sh.itemsB = (KC / 8) * sh.NR * W;
    sh.lds = (size_t)NTAP * F16_BM * pitch + (size_t)sh.NR * (W + 2) * pitch;
    return sh;
}

}  // namespace

namespace sdcconv {

// fp16 padded Cin of the weight tail: whole chunks of KC = 32 channels, for the 1x1x3 / 1x3x3 / 3x3x3 taps (0: no tail)
int f16_kc(int kD, int kH, int kW) {
    if (kW != 3) return 0;
    if ((kD == 1 && kH == 1) || ((kD == 1 || kD == 3) && kH == 3)) return 32;
    return 0;
}

// the dispatch table: covered shapes where the fp16 kernel was measured faster than precision 4's kernel
// Precision 6's dispatch table, measured on MI355X with tools/f16_step.py --shapes (every conv of the C2 / C3 / C4
// plans, sdc_conv / sdc_conv_gn at precision 4 against 7 on the same buffers): the rows where the fp16 kernel is ahead of precision 4's.
//   3x3x3: every covered conv (x1.33-1.81 against F(2x2x2,3x3x3)).
//   3x3: rows of 64 (x1.17-1.79) and of 16 (x1.23-1.30); rows of 32 from 32768 outputs per sample (x1.97-2.13; 16384: x0.99);
//        not rows of 128 (x0.72-0.85).
//   1x3: from 32768 outputs per sample (x1.22-1.62); below, precision 4's small-grid F(2,3) kernel wins (x0.75-0.92).
// Keyed on per-sample sizes only, never on the batch: the kernel a conv runs, and so a sample's bits, do not depend on its batch.
bool f16_faster(const SdcConvDesc& d) {
    const int64_t per_sample = (int64_t)d.Cout * d.oD * d.oH * d.oW;
    if (d.kD == 3) return true;
    if (d.kH == 3) return d.oW == 64 || d.oW == 16 || (d.oW == 32 && per_sample >= 32768);
    return per_sample >= 32768;
}

// coverage of conv_f16_kernel (precision 6): the tap shapes above at stride 1, pad 1 along every 3-wide axis, no upsampling, output size =
// input size, rows of 16 / 32 / 64 / 128 columns, whole rows per tile (for 3-row taps the rows of a (sample, depth) plane are a multiple or a
// divisor of the tile's 256 / W rows), octets of channels that never straddle the two inputs; plus the measured dispatch table f16_faster().
bool f16_ok(const SdcConvDesc& d) {
    if ((d.precision != 6 && d.precision != 7) || !f16_kc(d.kD, d.kH, d.kW)) return false;
    if (!(d.sD == 1 && d.sH == 1 && d.sW == 1 && d.uD == 1 && d.uH == 1 && d.uW == 1 && d.up_mode == 0 &&
          d.pW == 1 && d.pH == d.kH / 2 && d.pD == d.kD / 2 && d.oD == d.iD && d.oH == d.iH && d.oW == d.iW)) return false;
    if (!(d.oW == 16 || d.oW == 32 || d.oW == 64 || d.oW == 128)) return false;
    const int R = F16_BN / d.oW;
    if (d.kH == 3 && !(d.oH % R == 0 || R % d.oH == 0)) return false;
    if (d.Cin1 > 0 && d.Cin0 % 8 != 0) return false;
    const F16Shape sh = f16_shape(d);
    if (sh.itemsB > 8 * F16_NT || sh.lds > 160u * 1024u) return false;
    return d.precision == 7 || f16_faster(d);
}

int f16_gnparts(const SdcConvDesc& d, int G) {
    if (G <= 0 || d.Cout % G) return 0;
    const int cpg = d.Cout / G;
    const int64_t S = (int64_t)d.oD * d.oH * d.oW;
    if (cpg % 8 || !(S % F16_BN == 0 || (F16_BN % S == 0 && S % 64 == 0)) || !(cpg % F16_BM == 0 || F16_BM % cpg == 0)) return 0;
    return (int)(S >= F16_BN ? S / F16_BN : 1) * (cpg >= F16_BM ? cpg / F16_BM : 1);
}

const char* f16_name(const SdcConvDesc& d) {
    return d.kD == 3 ? "conv_f16_kernel<3x3x3>" : (d.kH == 3 ? "conv_f16_kernel<3x3>" : "conv_f16_kernel<1x3>");
}

int launch_f16(const ConvArgs& c, const _Float16* wh, hipStream_t s, const int32_t* gexp) {
    const SdcConvDesc& d = c.d;
    SDC_REQUIRE(reinterpret_cast<uintptr_t>(wh) % 16 == 0, SDC_EALIGN, "sdc_conv[fp16]: the packed weight buffer must be 16-byte aligned");
    const F16Shape sh = f16_shape(d);
    const int KC = f16_kc(d.kD, d.kH, d.kW);
    F16Args a;
    a.x0 = c.x0; a.x1 = c.x1 ? c.x1 : c.x0; a.wh = wh; a.bias = c.bias; a.res = c.res; a.y = c.y; a.gn_part = c.gn_part; a.gexp = gexp;
    for (int i = 0; i < 5; ++i) { a.x0s[i] = d.x0s[i]; a.x1s[i] = d.Cin1 ? d.x1s[i] : d.x0s[i]; a.ys[i] = d.ys[i]; a.rs[i] = d.rs[i]; }
    a.B = d.B; a.Cin0 = d.Cin0; a.Cin = d.Cin0 + d.Cin1; a.Cout = d.Cout; a.oD = d.oD; a.oH = d.oH; a.W = d.oW;
    a.lgW = d.oW == 16 ? 4 : d.oW == 32 ? 5 : d.oW == 64 ? 6 : 7;
    a.pD = d.pD; a.kD = d.kD;
    a.R = sh.R; a.Hs = sh.Hs; a.NR = sh.NR;
    a.nchunks = (a.Cin + KC - 1) / KC; a.nstages = d.kD * a.nchunks;
    a.Ntot = c.Ntot; a.nrows = c.Ntot / d.oW;
    a.ntiles = (c.Ntot + F16_BN - 1) / F16_BN; a.mtiles = (d.Cout + F16_BM - 1) / F16_BM;
    a.itemsB = sh.itemsB;
    a.ldsB = 3 * d.kH * F16_BM * (2 * KC + 16);
    a.gn_G = c.gn_G; a.gn_cpg = c.gn_cpg; a.gn_nparts = c.gn_nparts; a.gn_S = c.gn_S;
    SDC_REQUIRE((int64_t)a.ntiles * a.mtiles < (1ll << 31), SDC_EINVAL, "sdc_conv[fp16]: grid too large");
    // (the GroupNorm scratch -- 4 waves x 8 blocks x 2 doubles -- lives in the dead stage images)
    const dim3 grid((unsigned)(a.ntiles * a.mtiles));
#define F16_LAUNCH_SC(KH, ITB, SC)                                                                      \
    do {                                                                                                \
        static std::atomic<uint64_t> attr{0};                                                           \
        SDC_LDS_OPTIN(attr, (conv_f16_kernel<KH, ITB, SC>), 160 * 1024, "sdc_conv[fp16]");              \
        hipLaunchKernelGGL((conv_f16_kernel<KH, ITB, SC>), grid, dim3(F16_NT), sh.lds, s, a);           \
    } while (0)
#define F16_LAUNCH(KH, ITB)                                                                             \
    do {                                                                                                \
        if (gexp) F16_LAUNCH_SC(KH, ITB, true);                                                         \
        else F16_LAUNCH_SC(KH, ITB, false);                                                             \
    } while (0)
    if (d.kH == 3 && sh.itemsB <= 6 * F16_NT && sh.lds <= 80u * 1024u) F16_LAUNCH(3, 6);
    else if (d.kH == 3) F16_LAUNCH(3, 8);
    else F16_LAUNCH(1, 4);             // (1-D: 4 * 256 items and < 40 KB of LDS at every row width)
#undef F16_LAUNCH
#undef F16_LAUNCH_SC
    return sdc::check_launch("sdc_conv[fp16]");
}

// ------------------------------------------------------------------------------------------------ weight tail (precision 6)
// Wh[tap][ci / KC][co][ci % KC] = (fp16, RNE) w[co][ci][tap], zero for the padded ci; one thread per half
// (and the gap floats in front of the tail, written as zeros)
__global__ __launch_bounds__(256) void pack_f16_kernel(const float* __restrict__ w, _Float16* __restrict__ out, int Cout, int Cin, int taps,
                                                       int KC, int nchunks, int64_t n, int gap) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < gap) reinterpret_cast<float*>(out)[e - gap] = 0.0f;
    if (e >= n) return;
    const int k = (int)(e % KC);
    int64_t r = e / KC;
    const int co = (int)(r % Cout); r /= Cout;
    const int cc = (int)(r % nchunks);
    const int tap = (int)(r / nchunks);
    const int ci = cc * KC + k;
    out[e] = ci < Cin ? (_Float16)w[((int64_t)co * Cin + ci) * taps + tap] : (_Float16)0.0f;
}

int pack_f16_tail(const float* w, float* tail, int64_t gap, int Cout, int Cin, int kD, int kH, int kW, hipStream_t s) {
    const int KC = f16_kc(kD, kH, kW);
    const int taps = kD * kH * kW;
    const int nchunks = (Cin + KC - 1) / KC;
    const int64_t n = (int64_t)taps * nchunks * KC * Cout;
    SDC_REQUIRE(n / 256 + 1 < (1ll << 31), SDC_EINVAL, "sdc_pack_conv_weight: weight too large");
    hipLaunchKernelGGL(pack_f16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, w, reinterpret_cast<_Float16*>(tail), Cout, Cin,
                       taps, KC, nchunks, n, (int)gap);
    return sdc::check_launch("sdc_pack_conv_weight[fp16 tail]");
}

}  // namespace sdcconv
