// net.gemm_split (default on at precision >= 4, samplers only): the strided (1,4,4)/(1,2,2) convs, the 1x2x2 sub-pixel convs of the
// transposed convs and the 1x1x1 convs as an implicit GEMM on v_mfma_f32_32x32x16_bf16 with EXACT three-way bf16 operand splits -- the
// arithmetic of conv_stem_x3_kernel (sdc_conv_stem_x3.hip; split3, split3x8 and the term order are sdc_split3.h's): fp32 inputs, fp32 accumulation, fp32 outputs, x = h + m + l with h = bf16(x),
// m = bf16(x - h), l = bf16(x - h - m) (RNE, contraction off), six MFMAs per product, smallest terms first, the five small terms in
// accumulators of their own that are added to the main ones once at the end.
//
// Forms (template FORM; kD = 1, one input tensor, no residual, no upsampling):
//   0  taps (1,4,4), stride (1,2,2), pad (0,1,1), iH = 2 oH, iW = 2 oW
//   1  taps (1,2,2), stride 1, pad (0, pH, pW) with pH, pW in {0, 1}: the parity (1 - pH, 1 - pW) of a transposed conv, written into a
//      strided view of the full output
//   2  taps 1x1x1
// Tile: 64 output channels x 256 positions (256 / oW whole output rows of the (b, od, oh) walk; whole planes where a plane has fewer rows), four waves of 2 x 2 32x32 accumulators.
// K order: stage = NCB blocks of 16 input channels; inside a stage, channel block by channel block, tap by tap; one 16-deep MFMA step is
// the 16 channels of one (block, tap), lane half h holding the channel octet h.
//   Activations: the input rows a tile needs are staged ONCE per stage -- read as fp32, split, written to three bf16 LDS images
//     [piece][block, octet][column parity (form 0)][slot row][column + halo] of 16 bytes (one channel octet) per position -- and every tap
//     is an LDS offset: a value enters all its taps x 64 Cout products from one global load and one split.  Form 0 keeps even and odd
//     input columns in images of their own so that the 32 lanes of a fragment read walk consecutive 16-byte positions (stride 2 in one
//     image would put them 32 bytes apart).  Halo columns are zeroed once; rows outside the plane are staged as zeros: clipped taps add
//     exact zeros.  Slot rows: as the stem kernels', one group of SH (Hs - 1) + kH rows per plane a tile touches.
//   Weights: Wb[piece][m tile][stage][step][64 co][16 ci] bf16 (include/sdc.h, sdc_pack_gemm_x3): the SS steps of a sub-stage are one
//     contiguous run of SS * 2 KB per piece.
//   The next sub-stage's weights (and, before a new stage, its rows) are loaded into registers before this sub-stage's MFMAs.
// Every stage runs for every tile, fixed k order, no K split, no atomics: a sample's bits never depend on its tile mates or on the batch.
// Epilogue: bias, fp32 stores through the descriptor's strides (the parity views of form 1 are strided along H and W).
#include "sdc_conv.h"
#include "sdc_split3.h"

using namespace sdcconv;

namespace {

constexpr int GX_BM = 64, GX_BN = 256, GX_NT = 256;

struct GemmX3Args {
    const float* x;
    const __bf16* wb;
    const float* bias;
    float* y;
    int64_t xs[5], ys[5];
    int NP, oD, Cout, oH, W, lgW, iH, iW, lgIW;     // NP = B * oD planes
    int pH, pW;
    int Hs, GR, NR, RP;       // rows of a plane a tile can hold, slot rows per plane group, slot rows, LDS row pitch in positions
    int IMG;                  // bytes of one (channel block, octet) image
    int RT, nrows, ntiles, mtiles, itemsB, nst;      // rows of a tile, rows of the (b, od, oh) walk
    int plane;                // bf16 elements of one weight piece
};

template <int FORM> struct GxForm;
template <> struct GxForm<0> { static constexpr int TAPS = 16, NCB = 1, SS = 4, SH = 2, NPAR = 2; };
template <> struct GxForm<1> { static constexpr int TAPS = 4, NCB = 2, SS = 8, SH = 1, NPAR = 1; };
template <> struct GxForm<2> { static constexpr int TAPS = 1, NCB = 4, SS = 4, SH = 1, NPAR = 1; };

// ITB: staged 16-byte items per thread (2 NCB NR iW <= ITB * 256).  128 accumulator registers: one workgroup per CU.
// Up to 9 items the next stage's rows are held in registers during this stage's MFMAs; the 12-item instance (planes of a few rows,
// where the halo rows outnumber the rest) loads them when it stages them and keeps its registers free of spills.
template <int FORM, int ITB>
__global__ __launch_bounds__(GX_NT) __attribute__((amdgpu_waves_per_eu(1))) SDC_NO_DS_MERGE void conv_gemm_x3_kernel(const GemmX3Args a) {
    using F = GxForm<FORM>;
    constexpr int TAPS = F::TAPS, NCB = F::NCB, SS = F::SS, SH = F::SH;
    constexpr int KS = NCB * TAPS;                              // 16-deep MFMA steps per stage
    constexpr int NSUB = KS / SS;
    constexpr bool PREF = ITB <= 9;
    static_assert(NSUB * SS == KS, "whole sub-stages");
    constexpr int APC = SS * GX_BM * 32;                        // bytes of one piece of the A image
    constexpr int ASZ = 3 * APC;
    constexpr int NIA = 3 * SS * GX_BM * 2;                     // 16-byte A items per sub-stage
    constexpr int ITA = (NIA + GX_NT - 1) / GX_NT;
    extern __shared__ __attribute__((aligned(16))) char lds[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, lh = lane >> 5;
    const int W = a.W, RP = a.RP;
    const int IMG = a.IMG, BIMG = 2 * NCB * IMG;                // bytes of one image, of one piece
    const int PIMG = a.NR * RP * 16;                            // bytes of one column-parity image (form 0)
    const int logical = xcd_tile(blockIdx.x, a.ntiles * a.mtiles);
    const int mt = logical % a.mtiles, nt = logical / a.mtiles;
    const int m0 = mt * GX_BM;
    const int r0 = nt * a.RT;                                   // first row of the tile in the (b, od, oh) walk
    const int plane0 = r0 / a.oH, oh0 = r0 - plane0 * a.oH;

    // ---- per-thread B staging items: (image q = 2 block + octet, slot row sr, input column w), w fastest
    int64_t bb[ITB];
    int bdst[ITB];
    bool bok[ITB];
#pragma unroll
    for (int k = 0; k < ITB; ++k) {
        const int it = tid + k * GX_NT;
        const int w = it & (a.iW - 1);
        const int rest = it >> a.lgIW;
        const int q = rest / a.NR, sr = rest - q * a.NR;
        const int g = sr / a.GR, sq = sr - g * a.GR;
        const int pl = plane0 + g, ih = SH * (g == 0 ? oh0 : 0) - a.pH + sq;
        const bool ok = it < a.itemsB && pl < a.NP && ih >= 0 && ih < a.iH;
        const int b = ok ? pl / a.oD : 0, od = ok ? pl % a.oD : 0, ihc = ok ? ih : 0;
        bok[k] = ok;
        bb[k] = (int64_t)b * a.xs[0] + (int64_t)od * a.xs[2] + (int64_t)ihc * a.xs[3] + (int64_t)w * a.xs[4]
                + (int64_t)((q >> 1) * 16 + (q & 1) * 8) * a.xs[1];
        int col;
        if (FORM == 0) col = (w & 1) * (PIMG / 16) + sr * RP + (w >> 1) + 1;
        else if (FORM == 1) col = sr * RP + w + 1;
        else col = sr * RP + w;
        bdst[k] = ASZ + q * IMG + col * 16;
    }
    // ---- per-thread A staging items: 16-byte pieces of the sub-stage's [piece][step][co][16] blocks, in LDS order
    int aoff[ITA];
#pragma unroll
    for (int k = 0; k < ITA; ++k) {
        const int it = tid + k * GX_NT;
        const int p = it / (SS * 2 * GX_BM), q = it - p * (SS * 2 * GX_BM);
        aoff[k] = it < NIA ? p * a.plane + mt * (a.nst * KS * GX_BM * 16) + q * 8 : 0;      // bf16 elements; + (st KS + sub SS) 1024 per sub-stage
    }

    float bv[ITB][8];
    uint4 av[ITA];
    auto load_a = [&](int st, int sub) {
        const int wst = (st * KS + sub * SS) * (GX_BM * 16);
#pragma unroll
        for (int k = 0; k < ITA; ++k) {
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (tid + k * GX_NT < NIA) v = *reinterpret_cast<const uint4*>(a.wb + wst + aoff[k]);
            av[k] = v;
        }
    };
    auto load_b = [&](int st) {
        const int64_t co = (int64_t)st * (NCB * 16) * a.xs[1];
#pragma unroll
        for (int k = 0; k < ITB; ++k) {
            const float* q = a.x + bb[k] + co;
#pragma unroll
            for (int i = 0; i < 8; ++i) { bv[k][i] = bok[k] ? *q : 0.0f; q += a.xs[1]; }
        }
    };
    auto store_a = [&]() {
#pragma unroll
        for (int k = 0; k < ITA; ++k)
            if (tid + k * GX_NT < NIA) *reinterpret_cast<uint4*>(lds + (tid + k * GX_NT) * 16) = av[k];
    };
    auto store_b = [&]() {
#pragma unroll
        for (int k = 0; k < ITB; ++k) {
            if (tid + k * GX_NT < a.itemsB) {
                bf16x8 h, m, l;
                split3x8(bv[k], h, m, l);
                *reinterpret_cast<bf16x8*>(lds + bdst[k]) = h;
                *reinterpret_cast<bf16x8*>(lds + bdst[k] + BIMG) = m;
                *reinterpret_cast<bf16x8*>(lds + bdst[k] + 2 * BIMG) = l;
            }
        }
    };

    // zero halo columns 0 and RP - 1 of every row of every image (never overwritten: the staged columns are 1 .. RP - 2)
    if (FORM != 2) {
        const int nrows = 3 * 2 * NCB * F::NPAR * a.NR;         // the images are back to back: rows of RP positions
        for (int e = tid; e < 2 * nrows; e += GX_NT) {
            const int row = e >> 1;
            *reinterpret_cast<uint4*>(lds + ASZ + (row * RP + ((e & 1) ? RP - 1 : 0)) * 16) = make_uint4(0u, 0u, 0u, 0u);
        }
    }

    // fragment bases (first piece, block 0): B position (wave * 64 + 32 j + l31) of the tile, the top-left tap; lane half h reads octet h
    int bB[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int p = wave * 64 + 32 * j + l31;
        const bool pok = (p >> a.lgW) < a.RT && r0 + (p >> a.lgW) < a.nrows;
        const int rl = pok ? p >> a.lgW : 0, col = pok ? p & (W - 1) : 0;
        const int row = r0 + rl, pl = row / a.oH, oh = row - pl * a.oH, g = pl - plane0;
        const int slot = g * a.GR + SH * (oh - (g == 0 ? oh0 : 0));
        bB[j] = ASZ + (slot * RP + col + (FORM == 1 ? 1 - a.pW : 0)) * 16 + lh * IMG;
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
    if (PREF) load_b(0);
    for (int st = 0; st < a.nst; ++st) {
#pragma unroll
        for (int sub = 0; sub < NSUB; ++sub) {
            __syncthreads();                                    // the previous sub-stage's fragments are read
            store_a();
            if (sub == 0) {
                if (!PREF) load_b(st);
                store_b();
            }
            __syncthreads();
            if (sub + 1 < NSUB) load_a(st, sub + 1);            // in flight during this sub-stage's MFMAs
            else if (st + 1 < a.nst) {
                load_a(st + 1, 0);
                if (PREF) load_b(st + 1);
            }
#pragma unroll
            for (int sl = 0; sl < SS; ++sl) {
                const int ks = sub * SS + sl;
                const int cbk = ks / TAPS, tap = ks - cbk * TAPS;
                int tb = cbk * 2 * IMG;
                if (FORM == 0) {
                    const int kh = tap >> 2, kw = tap & 3;      // input column 2 ow - 1 + kw: parity (kw + 1) & 1, index ow + (kw + 1) / 2
                    tb += ((kw + 1) & 1) * PIMG + kh * rowb + ((kw + 1) >> 1) * 16;
                } else if (FORM == 1) {
                    tb += (tap >> 1) * rowb + (tap & 1) * 16;
                }
                bf16x8 af[2][3], bf[2][3];
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int p = 0; p < 3; ++p)
                        af[i][p] = *reinterpret_cast<const bf16x8*>(lds + p * APC + (sl * GX_BM + 32 * i) * 32 + aoffr);
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int p = 0; p < 3; ++p) bf[j][p] = *reinterpret_cast<const bf16x8*>(lds + bB[j] + tb + p * BIMG);
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
    // ---- epilogue: bias (loaded in one batch under a wave-uniform condition), fp32 stores through the strides
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
        const int p = wave * 64 + 32 * j + l31;
        if ((p >> a.lgW) >= a.RT || r0 + (p >> a.lgW) >= a.nrows) continue;
        const int row = r0 + (p >> a.lgW), col = p & (W - 1);
        const int pl = row / a.oH, oh = row - pl * a.oH;
        const int b = pl / a.oD, od = pl - b * a.oD;
        float* yp = a.y + (int64_t)b * a.ys[0] + (int64_t)od * a.ys[2] + (int64_t)oh * a.ys[3] + (int64_t)col * a.ys[4]
                    + (int64_t)(m0 + 4 * lh) * a.ys[1];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
#pragma unroll
            for (int rr = 0; rr < 16; ++rr)
                yp[(int64_t)(32 * i + (rr & 3) + 8 * (rr >> 2)) * a.ys[1]] = acc[i][j][rr] + bz[i][rr];
        }
    }
}

// Wb[piece][m tile][stage][step = block * taps + tap][64 co][16 ci]: the three bf16 pieces of Wp[tap * Cin + ci][co] with
// ci = (stage * NCB + block) * 16 + (0..15), co = 64 m tile + (0..63); one thread per element of a plane
__global__ __launch_bounds__(256) void pack_gemm_x3_kernel(const float* __restrict__ wp, __bf16* __restrict__ out, int Cout, int Cin, int taps,
                                                           int ncb, int64_t n) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const int c16 = (int)(e & 15), col = (int)((e >> 4) & 63);
    int64_t r = e >> 10;
    const int KS = ncb * taps, nst = Cin / (16 * ncb);
    const int ks = (int)(r % KS); r /= KS;
    const int st = (int)(r % nst);
    const int mt = (int)(r / nst);
    const int cbk = ks / taps, tap = ks - cbk * taps;
    const int ci = (st * ncb + cbk) * 16 + c16, co = mt * 64 + col;
    __bf16 ph, pm, pl;
    split3(wp[((int64_t)tap * Cin + ci) * Cout + co], ph, pm, pl);
    out[e] = ph; out[n + e] = pm; out[2 * n + e] = pl;
}

// channel blocks of 16 per stage for a tap shape (0: not a covered tap shape)
int gx_ncb(int kH, int kW) { return kH == 4 && kW == 4 ? 1 : kH == 2 && kW == 2 ? 2 : kH == 1 && kW == 1 ? 4 : 0; }

struct GxShape { int form, RT, Hs, NG, GR, NR, RP, itemsB, IMG; size_t lds; };

GxShape gx_shape(const SdcConvDesc& d) {
    GxShape s{};
    s.form = d.kH == 4 ? 0 : d.kH == 2 ? 1 : 2;
    const int ncb = gx_ncb(d.kH, d.kW), npar = s.form == 0 ? 2 : 1, sh = s.form == 0 ? 2 : 1;
    const int ss = s.form == 1 ? 8 : 4;
    const int R = GX_BN / d.oW;
    // planes of fewer than R rows: a tile is R / oH whole planes (the rows left over stay empty), so that the halo rows of a plane are
    // staged once -- fewer planes where their halo rows would not fit the LDS or the largest instance (planes of two or three rows:
    // more empty positions in the tile); else a tile is R rows, inside one plane when R divides oH and across two otherwise
    const int maxit = (s.form == 0 ? 12 : 8) * GX_NT;
    auto fill = [&](int ng) {
        s.NG = ng;
        s.GR = sh * (s.Hs - 1) + d.kH;
        s.NR = s.NG * s.GR;
        s.RP = s.form == 0 ? d.iW / 2 + 2 : s.form == 1 ? d.iW + 2 : d.iW;
        s.IMG = npar * s.NR * s.RP * 16;
        s.itemsB = 2 * ncb * s.NR * d.iW;
        s.lds = (size_t)3 * ss * GX_BM * 32 + (size_t)3 * 2 * ncb * s.IMG;
        return s.itemsB <= maxit && s.lds <= 160u * 1024u;
    };
    if (d.oH < R) {
        s.Hs = d.oH;
        int ng = R / d.oH;
        while (!fill(ng) && ng > 1) --ng;
        s.RT = s.NG * d.oH;
    } else {
        s.Hs = R; s.RT = R;
        fill(d.oH % R == 0 ? 1 : 2);
    }
    return s;
}

}  // namespace

namespace sdcconv {

// coverage of conv_gemm_x3_kernel: descriptor only, per-sample sizes only (never B)
bool gemm_x3_covers(const SdcConvDesc& d) {
    if (!(d.kD == 1 && d.sD == 1 && d.pD == 0 && d.uD == 1 && d.uH == 1 && d.uW == 1 && d.up_mode == 0 && d.oD == d.iD)) return false;
    if (!(d.B > 0 && d.oD > 0 && d.oH > 0 && d.Cin1 == 0 && d.Cout > 0 && d.Cout % 64 == 0)) return false;
    for (int i = 0; i < 5; ++i)
        if (d.rs[i] != 0 || d.x1s[i] != 0) return false;       // a residual or a second input
    const int ncb = gx_ncb(d.kH, d.kW);
    if (ncb == 0 || d.Cin0 <= 0 || d.Cin0 % (16 * ncb) != 0) return false;
    if (d.kH == 4) {
        if (!(d.sH == 2 && d.sW == 2 && d.pH == 1 && d.pW == 1 && d.iH == 2 * d.oH && d.iW == 2 * d.oW)) return false;
    } else if (d.kH == 2) {
        if (!(d.sH == 1 && d.sW == 1 && (d.pH == 0 || d.pH == 1) && (d.pW == 0 || d.pW == 1) && d.iH == d.oH && d.iW == d.oW)) return false;
    } else {
        if (!(d.sH == 1 && d.sW == 1 && d.pH == 0 && d.pW == 0 && d.iH == d.oH && d.iW == d.oW)) return false;
    }
    if (!(d.oW == 16 || d.oW == 32 || d.oW == 64 || d.oW == 128)) return false;
    const GxShape s = gx_shape(d);
    return s.itemsB <= (s.form == 0 ? 12 : 8) * GX_NT && s.lds <= 160u * 1024u;      // (the largest instance of each form)
}

int launch_gemm_x3(const SdcConvDesc& d, const float* x, const __bf16* wb, const float* bias, float* y, hipStream_t s) {
    SDC_REQUIRE(reinterpret_cast<uintptr_t>(wb) % 16 == 0, SDC_EALIGN, "sdc_conv_gemm_x3: the packed weight buffer must be 16-byte aligned");
    const GxShape sh = gx_shape(d);
    const int ncb = gx_ncb(d.kH, d.kW);
    GemmX3Args a;
    a.x = x; a.wb = wb; a.bias = bias; a.y = y;
    for (int i = 0; i < 5; ++i) { a.xs[i] = d.x0s[i]; a.ys[i] = d.ys[i]; }
    a.NP = d.B * d.oD; a.oD = d.oD; a.Cout = d.Cout; a.oH = d.oH; a.W = d.oW; a.iH = d.iH; a.iW = d.iW;
    a.lgW = d.oW == 16 ? 4 : d.oW == 32 ? 5 : d.oW == 64 ? 6 : 7;
    a.lgIW = d.iW == d.oW ? a.lgW : a.lgW + 1;
    a.pH = d.pH; a.pW = d.pW;
    a.Hs = sh.Hs; a.GR = sh.GR; a.NR = sh.NR; a.RP = sh.RP; a.IMG = sh.IMG;
    const int64_t nrows = (int64_t)d.B * d.oD * d.oH;
    SDC_REQUIRE(nrows * d.oW < (1ll << 31), SDC_EINVAL, "sdc_conv_gemm_x3: too many output positions");
    const int64_t plane = (int64_t)d.kH * d.kW * d.Cin0 * d.Cout;
    SDC_REQUIRE(3 * plane < (1ll << 31), SDC_EINVAL, "sdc_conv_gemm_x3: weight too large");
    a.plane = (int)plane;
    a.nrows = (int)nrows; a.RT = sh.RT;
    a.ntiles = (a.nrows + sh.RT - 1) / sh.RT; a.mtiles = d.Cout / GX_BM;
    a.itemsB = sh.itemsB;
    a.nst = d.Cin0 / (16 * ncb);
    SDC_REQUIRE((int64_t)a.ntiles * a.mtiles < (1ll << 31), SDC_EINVAL, "sdc_conv_gemm_x3: grid too large");
    const dim3 grid((unsigned)(a.ntiles * a.mtiles));
#define GX_LAUNCH(FORM, ITB)                                                                                        \
    do {                                                                                                            \
        static std::atomic<uint64_t> attr{0};                                                                       \
        SDC_LDS_OPTIN(attr, (conv_gemm_x3_kernel<FORM, ITB>), 160 * 1024, "sdc_conv_gemm_x3");                      \
        hipLaunchKernelGGL((conv_gemm_x3_kernel<FORM, ITB>), grid, dim3(GX_NT), sh.lds, s, a);                      \
    } while (0)
    if (sh.form == 0) { if (sh.itemsB <= 9 * GX_NT) GX_LAUNCH(0, 9); else GX_LAUNCH(0, 12); }
    else if (sh.form == 1) { if (sh.itemsB <= 5 * GX_NT) GX_LAUNCH(1, 5); else GX_LAUNCH(1, 8); }
    else GX_LAUNCH(2, 8);
#undef GX_LAUNCH
    return sdc::check_launch("sdc_conv_gemm_x3");
}

}  // namespace sdcconv

extern "C" size_t sdc_pack_gemm_x3_bytes(int Cout, int Cin, int kH, int kW) {
    const int ncb = gx_ncb(kH, kW);
    if (ncb == 0 || Cout <= 0 || Cout % 64 != 0 || Cin <= 0 || Cin % (16 * ncb) != 0) return 0;
    return (size_t)3 * kH * kW * Cin * Cout * sizeof(__bf16);
}

extern "C" int sdc_pack_gemm_x3(const float* wp, void* out, int Cout, int Cin, int kH, int kW, void* stream) {
    SDC_REQUIRE(wp && out, SDC_ENULL, "sdc_pack_gemm_x3: null pointer");
    SDC_REQUIRE(sdc_pack_gemm_x3_bytes(Cout, Cin, kH, kW) > 0, SDC_EINVAL,
                "sdc_pack_gemm_x3: taps 4x4, 2x2 or 1x1, Cout a multiple of 64, Cin a multiple of 16 / 32 / 64 (got %dx%d, Cin %d, Cout %d)",
                kH, kW, Cin, Cout);
    const int64_t n = (int64_t)kH * kW * Cin * Cout;
    SDC_REQUIRE(n / 256 + 1 < (1ll << 31), SDC_EINVAL, "sdc_pack_gemm_x3: weight too large");
    hipLaunchKernelGGL(pack_gemm_x3_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, sdc::as_stream(stream), wp,
                       reinterpret_cast<__bf16*>(out), Cout, Cin, kH * kW, gx_ncb(kH, kW), n);
    return sdc::check_launch("sdc_pack_gemm_x3");
}

// The routing table of net.gemm_split: the shapes where every repeat of sdc_conv_gemm_x3 measured faster than every
// repeat of sdc_conv at precision 4 on the same buffers (profiles/gemm_x3_shapes.log).  Per-sample sizes only -- taps, stride, channels,
// output plane -- never B: a sample's bits do not depend on its batch.
//   strided (1,4,4)/(1,2,2):  64 -> 64 into 32 x 32 (x1.68),  128 -> 128 into 16 x 16 (x1.57)
//   sub-pixel (1,2,2), every parity:  128 -> 128 over 16 x 16 (x1.38-1.40),  64 -> 64 over 32 x 32 (x1.32-1.33)
//   1x1x1: none (x0.71-0.81 on the smoke net's shapes: conv_pw2_kernel's two waves per SIMD win where a staged value enters 64 products)
static bool gemm_x3_faster(const SdcConvDesc& d) {
    const bool c64 = d.Cin0 == 64 && d.Cout == 64 && d.oH == 32 && d.oW == 32;
    const bool c128 = d.Cin0 == 128 && d.Cout == 128 && d.oH == 16 && d.oW == 16;
    return (d.kH == 4 || d.kH == 2) && (c64 || c128);
}

extern "C" int sdc_conv_gemm_x3_ok(const SdcConvDesc* dp) {
    return dp && gemm_x3_covers(*dp) && gemm_x3_faster(*dp) ? 1 : 0;
}

extern "C" int sdc_conv_gemm_x3(const SdcConvDesc* dp, const float* x, const void* wb, const float* bias, float* y, void* stream) {
    SDC_REQUIRE(dp && x && wb && y, SDC_ENULL, "sdc_conv_gemm_x3: null pointer");
    SDC_REQUIRE(gemm_x3_covers(*dp), SDC_EINVAL, "sdc_conv_gemm_x3: descriptor not covered: %dx%dx%d taps, stride %dx%dx%d, Cin %d+%d, Cout %d, "
                "residual %d, output %dx%dx%d", dp->kD, dp->kH, dp->kW, dp->sD, dp->sH, dp->sW, dp->Cin0, dp->Cin1, dp->Cout, (int)(dp->rs[1] != 0),
                dp->oD, dp->oH, dp->oW);
    return launch_gemm_x3(*dp, x, reinterpret_cast<const __bf16*>(wb), bias, y, sdc::as_stream(stream));
}
