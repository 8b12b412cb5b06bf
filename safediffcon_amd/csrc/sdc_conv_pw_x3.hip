// conv_pw_x3_kernel: the pointwise (1x1x1, stride 1) convs over a dense layout as EXACT three-way bf16 operand splits on the bf16 matrix
// pipe, with the weights resident in LDS for the whole launch.  Reference ops: those of conv_pw2_kernel
// (sdc_conv_pw2.inc) -- the to_qkv / to_out projections of the attention blocks and the res_conv 1x1x1 convs of the smoke U-Net.
//
// Arithmetic: section 14's, the stem's and conv_gemm_x3_kernel's (sdc_split3.h): fp32 inputs, fp32 accumulation, fp32 outputs,
// x = h + m + l with h = bf16(x), m = bf16(x - h), l = bf16(x - h - m) (RNE, contraction off), six v_mfma_f32_32x32x16_bf16 per product,
// smallest terms first, the five small terms in accumulators of their own that are added to the main ones once at the end.  Fixed k
// order, no K split, no atomics: a position's bits depend on its own K values and the weights only, never on its batch or tile mates.
//
// Form (what differs from conv_gemm_x3_kernel's form 2, which staged every activation through LDS between two barriers per 64 channels
// for 64 products each):
//   * One workgroup per CU (persistent), bound to ONE block of MB = 32 TM output channels.  Before its position walk it reads its block
//     of the conv's ordinary fp32 Wp[ci][co], splits every value once and writes three bf16 images [piece][k octet][co] of 16 bytes
//     (8 consecutive k of one output channel) each: lane (r, h) of an A fragment reads octet 2 chunk + h of channel r, so the 16 lanes of
//     a ds_read_b128 group walk 16 consecutive 16-byte slots -- conflict-free without padding.  K * MB * 6 bytes (+ the bias block).
//   * Activations never touch LDS: a wave owns WP = 32 TN positions (lane n of position tile j owns position TN n + j, conv_pw2's
//     interleave: one load per channel serves the TN tiles, one store per output row) and ALL MB channels of its workgroup.  Lane half h
//     loads channels 16 chunk + 8 h + (0..7) of its positions straight from global memory -- the B fragment's k order -- and splits them
//     in registers.  A split value enters MB products; every weight fragment read feeds TN MFMAs.
//   * No barrier after the weight staging.  The four waves walk tiles of their own: tile = 4 walker + wave, + 4 walkers per round.
//   * The k walk is one continuous stream of steps (tile, chunk of 16 channels) across tile boundaries: during the MFMAs of step s the
//     wave reads the weight fragments of step s + 1, splits the activations of step s + 1 (loaded during step s - 2) and issues the loads
//     of step s + 3; a sched_barrier per term keeps each piece of that work with its term, and a step holds no branch.
//   * MB is the widest of 128, 96 and 64 channels that divides Cout and fits the LDS (pw_x3_block): TM = 4, 3 or 2 tiles of 32 channels.
//   * Workgroup order: the MT = Cout / MB blocks of a walker are neighbours among the workgroups that share an XCD (blockIdx % 8), block
//     index fastest: they read the same positions at the same time, so x comes from HBM once and from that XCD's L2 MT - 1 times.
//   * Epilogue: small + main, + bias (from LDS), + residual (batches of 8 rows of loads), stores of TN floats through the strides.
// Non-finite inputs give NaN where the fp32 kernels give +-Inf (Inf - Inf in the split), confined to the value's own position.
#include "sdc_conv.h"
#include "sdc_split3.h"

namespace sdc { int ta_grid(const char* entry, int64_t nblk, unsigned* grid); }      // sdc_tablock.hip: min(nblk, CU count), cached per device

using namespace sdcconv;

namespace {

constexpr int PX_NT = 256;
constexpr int PX_LDS_MAX = 160 * 1024;

struct PwX3Args {
    const float *x0, *x1, *wp, *bias, *res;
    float* y;
    int64_t x0s1, x1s1, ys1, rs1;         // channel strides (elements)
    int x0s0, x1s0, ys0, rs0;             // sample strides: every (sample, position) offset is below 2^30 (route()'s `small`, y_dense)
    int Cin0, K, Cout, S, Ntot;
    int ntiles, MT, nwalk, gx;            // wave tiles, Cout blocks, walkers (workgroups per block), workgroups per XCD label (0: plain order)
};

template <int TM, int TN, bool RES>
__global__ __launch_bounds__(PX_NT) __attribute__((amdgpu_waves_per_eu(1))) SDC_NO_DS_MERGE void conv_pw_x3_kernel(const PwX3Args a) {
    constexpr int MB = 32 * TM, WP = 32 * TN;
    static_assert(TN == 2 || TN == 4, "position tiles per wave");      // (launch_pw_x3 instantiates TN = 2: TM = 4 leaves no accumulators for more)
    typedef float vecn __attribute__((ext_vector_type(TN)));
    typedef float nfloat4 __attribute__((ext_vector_type(4)));
    typedef const __attribute__((address_space(1))) vecn* gvec_p;
    typedef __attribute__((address_space(1))) vecn* gwvec_p;
    typedef const __attribute__((address_space(1))) char* gchar_p;
    typedef __attribute__((address_space(1))) char* gwchar_p;
    extern __shared__ __attribute__((aligned(16))) char px_lds[];

    const int tid = threadIdx.x, lane = tid & 63, wave = SDC_UNIFORM(tid >> 6);
    const int l31 = lane & 31, lh = lane >> 5;
    const int K = a.K, nch = K >> 4;
    const int PSZ = K * MB * 2;                                 // bytes of one piece's image
    int mt, walker;
    if (a.gx) {
        const int q = blockIdx.x >> 3;
        mt = q % a.MT;
        walker = (blockIdx.x & 7) * (a.gx / a.MT) + q / a.MT;
    } else {
        mt = blockIdx.x % a.MT;
        walker = blockIdx.x / a.MT;
    }
    const int m0 = mt * MB;

    // ---- the weight block, once: item e = (k octet, co); 8 rows of Wp (co fastest: coalesced), one split, three 16-byte writes
    for (int e = tid; e < (K >> 3) * MB; e += PX_NT) {
        const int oct = e / MB, co = e - oct * MB;
        const float* w = a.wp + (int64_t)(oct * 8) * a.Cout + m0 + co;
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = w[(int64_t)j * a.Cout];
        bf16x8 h, m, l;
        split3x8(v, h, m, l);
        *reinterpret_cast<bf16x8*>(px_lds + e * 16) = h;
        *reinterpret_cast<bf16x8*>(px_lds + PSZ + e * 16) = m;
        *reinterpret_cast<bf16x8*>(px_lds + 2 * PSZ + e * 16) = l;
    }
    float* const lbias = reinterpret_cast<float*>(px_lds + 3 * PSZ);
    if (tid < MB) lbias[tid] = a.bias ? a.bias[m0 + tid] : 0.0f;
    __syncthreads();

    // ---- the load stream: step = (tile, chunk), tiles of this wave in walk order; past the last tile it reads (sample 0, position 0)
    const int nww = a.nwalk * 4;
    const int t_first = walker * 4 + wave;
    auto tile_off = [&](const int t, uint32_t& o0, uint32_t& o1) {
        const int p = t < a.ntiles ? t * WP + TN * l31 : a.Ntot;
        const int pp = p < a.Ntot ? p : 0;                      // (Ntot % 4 == 0: a lane's TN positions are all inside or all outside)
        const int b = pp / a.S, sp = pp - b * a.S;
        o0 = (uint32_t)(b * a.x0s0 + sp + 8 * lh * (int)a.x0s1) * 4u;
        o1 = K > a.Cin0 ? (uint32_t)(b * a.x1s0 + sp + 8 * lh * (int)a.x1s1) * 4u : 0u;
    };
    // (no branch inside a step: with one, the compiler sinks the next step's splits out of the MFMA shadows into the block that uses them.
    // The stream crosses into the wave's next tile once per tile; that tile's offsets -- an integer division -- are formed before the
    // tile's first step and selected here)
    int l_c = 0;
    uint32_t l_o0, l_o1, n_o0 = 0, n_o1 = 0;
    tile_off(t_first, l_o0, l_o1);
    vecn raw[2][8];
    auto issue = [&](const int set) __attribute__((always_inline)) {
        const int ci = l_c * 16;
        const bool first = ci < a.Cin0;
        const int64_t cs = first ? a.x0s1 : a.x1s1;
        const gchar_p base = (gchar_p)uniform_ptr(first ? a.x0 + ci * cs : a.x1 + (ci - a.Cin0) * cs);
        const uint32_t cs4 = (uint32_t)cs * 4u;
        uint32_t o = first ? l_o0 : l_o1;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            raw[set][j] = *(gvec_p)(base + o);
            o += cs4;
        }
        const bool wrap = ++l_c == nch;
        l_c = wrap ? 0 : l_c;
        l_o0 = wrap ? n_o0 : l_o0;
        l_o1 = wrap ? n_o1 : l_o1;
    };

    // weight fragments: piece 0 (h) is read by terms 2, 4 and 5 and has a register set per step parity; pieces 2 and 1 are last read by
    // terms 0 and 3, so the next step's are read into the same registers right behind those terms (96 -> 64 registers at TM = 4)
    bf16x8 a0[2][TM], a1[TM], a2[TM], bfr[2][TN][3];
    const int a_lane = (lh * MB + l31) * 16;
    auto read_a = [&](bf16x8 (&dst)[TM], const int piece, const int c) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
            dst[i] = *reinterpret_cast<const bf16x8*>(px_lds + piece * PSZ + (c * 2 * MB + 32 * i) * 16 + a_lane);
    };
    // part = (position tile j, k half): four values of a lane, the elements 4 half .. 4 half + 3 of the tile's three fragments
    auto split_part = [&](const int set, const int part) __attribute__((always_inline)) {
        const int j = part >> 1, kh = part & 1;
#pragma unroll
        for (int k = 4 * kh; k < 4 * kh + 4; ++k) {
            __bf16 ph, pm, pl;
            split3(raw[set][k][j], ph, pm, pl);
            bfr[set][j][0][k] = ph; bfr[set][j][1][k] = pm; bfr[set][j][2][k] = pl;
        }
    };

    f32x16 acc[TM][TN], sm[TM][TN];
    // step s = chunk c of the current tile, P = s & 1 = c & 1 (K % 32 == 0: a tile is an even number of steps).  FIRST: the tile's first
    // step starts both accumulator sets from zero (the MFMA's inline constant: no register is cleared).  LAST: the tile's last step
    // leaves the next tile's weight fragments to be read behind the epilogue, whose rows need those 16 TM registers
    auto step = [&](auto pc, auto fc, auto lc, const int c) __attribute__((always_inline)) {
        constexpr int P = decltype(pc)::value;
        constexpr bool FIRST = decltype(fc)::value, LAST = decltype(lc)::value;
        const int cn = c + 1 == nch ? 0 : c + 1;
#pragma unroll
        for (int t = 0; t < 6; ++t) {
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    f32x16& c16 = t < 5 ? sm[i][j] : acc[i][j];
                    f32x16 cin = c16;
                    if (FIRST && (t == 0 || t == 5)) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) cin[r] = 0.0f;
                    }
                    const bf16x8 av = X3_PA[t] == 0 ? a0[P][i] : (X3_PA[t] == 1 ? a1[i] : a2[i]);
                    c16 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, bfr[P][j][X3_PB[t]], cin, 0, 0, 0);
                }
            // the next step's operands, a piece per term: weight fragments behind their last reader, the splits of 2 TN half fragments
            // over terms 0 .. 3, the loads of step s + 3 into the registers the splits have read
            if (!LAST) {
                if (t == 0) read_a(a2, 2, cn);
                if (t == 1) read_a(a0[P ^ 1], 0, cn);
                if (t == 3) read_a(a1, 1, cn);
            }
            if (t < 4) {
#pragma unroll
                for (int q = 0; q < TN / 2; ++q) split_part(P ^ 1, t * (TN / 2) + q);
            }
            if (t == 5) issue(P ^ 1);
            __builtin_amdgcn_sched_barrier(0);
        }
    };

    // prologue: steps 0 and 1 travel together; step 0 is split, step 2 follows it into its registers
    issue(0);
    issue(1);
#pragma unroll
    for (int q = 0; q < 2 * TN; ++q) split_part(0, q);
    issue(0);
    read_a(a2, 2, 0);
    read_a(a1, 1, 0);
    read_a(a0[0], 0, 0);

    constexpr std::integral_constant<int, 0> P0{};
    constexpr std::integral_constant<int, 1> P1{};
    for (int t = t_first; t < a.ntiles; t += nww) {
        tile_off(t + nww, n_o0, n_o1);
        constexpr std::true_type Y{};
        constexpr std::false_type N{};
        step(P0, Y, N, 0);
        step(P1, N, N, 1);
        for (int c = 2; c + 2 < nch; c += 2) {
            step(P0, N, N, c);
            step(P1, N, N, c + 1);
        }
        step(P0, N, N, nch - 2);
        step(P1, N, Y, nch - 1);
        // ---- epilogue: tile (i, j), register rr of lane (l31, lh) is channel m0 + 32 i + 8 (rr >> 2) + 4 lh + (rr & 3) and position
        // t WP + TN l31 + j: the TN tiles of a lane are consecutive positions -> one store per (i, rr)
        const int p = t * WP + TN * l31;
        const bool pok = p < a.Ntot;
        const int pp = pok ? p : 0;
        const int b = pp / a.S, sp = pp - b * a.S;
        uint32_t yo = (uint32_t)(b * a.ys0 + sp + 4 * lh * (int)a.ys1) * 4u;
        uint32_t ro = RES ? (uint32_t)(b * a.rs0 + sp + 4 * lh * (int)a.rs1) * 4u : 0u;
        // (the channel walks on the lane offsets, rows 0 1 2 3 8 9 10 11 ...: a scalar base per row would be hoisted out of the tile
        // loop, 2 x 32 TM register pairs that spill)
        const uint32_t ys4 = (uint32_t)a.ys1 * 4u, rs4 = (uint32_t)a.rs1 * 4u;
        const gchar_p rb = (gchar_p)uniform_ptr(RES ? a.res + (int64_t)m0 * a.rs1 : a.y);
        const gwchar_p yb = (gwchar_p)(__attribute__((address_space(1))) void*)uniform_ptr(a.y + (int64_t)m0 * a.ys1);
#pragma unroll
        for (int i = 0; i < TM; ++i) {
#pragma unroll
            for (int hb = 0; hb < 2; ++hb) {
                // residual and bias of 8 rows as one batch of loads (one memory round trip per batch, not one per row)
                vecn rv[8];
                nfloat4 bz[2];
                if (RES) {
#pragma unroll
                    for (int q = 0; q < 8; ++q) {
                        rv[q] = *(gvec_p)(rb + ro);
                        ro += (q & 3) < 3 ? rs4 : 5 * rs4;
                    }
                }
#pragma unroll
                for (int g = 0; g < 2; ++g) bz[g] = *reinterpret_cast<const nfloat4*>(lbias + 32 * i + 8 * (2 * hb + g) + 4 * lh);
                vecn v[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const int rr = hb * 8 + q;
#pragma unroll
                    for (int j = 0; j < TN; ++j) v[q][j] = (acc[i][j][rr] + sm[i][j][rr]) + bz[q >> 2][q & 3];
                    if (RES) v[q] += rv[q];
                }
                if (pok) {                                   // (one masked region per batch, not a branch per store)
                    uint32_t o = yo;
#pragma unroll
                    for (int q = 0; q < 8; ++q) {
                        *(gwvec_p)(yb + o) = v[q];
                        o += (q & 3) < 3 ? ys4 : 5 * ys4;
                    }
                }
                yo += 16 * ys4;
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        read_a(a2, 2, 0);
        read_a(a1, 1, 0);
        read_a(a0[0], 0, 0);
    }
}

template <int TM, int TN>
int launch_px(PwX3Args& a, int ncu, hipStream_t s) {
    constexpr int MB = 32 * TM, WP = 32 * TN;
    a.ntiles = (a.Ntot + WP - 1) / WP;
    a.MT = a.Cout / MB;
    // one workgroup per CU; the blocks of a walker among the workgroups of one XCD label.  Fewer wave tiles than waves: a workgroup
    // per four tiles, plain order
    const int need = (a.ntiles + 3) / 4;
    const int per = ncu / 8;
    if (ncu % 8 == 0 && per >= a.MT && 8 * (per / a.MT) <= need) {
        a.gx = (per / a.MT) * a.MT;
        a.nwalk = 8 * (per / a.MT);
    } else {
        a.gx = 0;
        a.nwalk = ncu / a.MT < 1 ? 1 : ncu / a.MT;
        if (a.nwalk > need) a.nwalk = need;
    }
    const size_t lds = (size_t)3 * a.K * MB * 2 + MB * sizeof(float);
    if (a.res) {
        static std::atomic<uint64_t> attr{0};
        SDC_LDS_OPTIN(attr, (conv_pw_x3_kernel<TM, TN, true>), PX_LDS_MAX, "sdc_conv_pw_x3");
        hipLaunchKernelGGL((conv_pw_x3_kernel<TM, TN, true>), dim3((unsigned)(a.nwalk * a.MT)), dim3(PX_NT), lds, s, a);
    } else {
        static std::atomic<uint64_t> attr{0};
        SDC_LDS_OPTIN(attr, (conv_pw_x3_kernel<TM, TN, false>), PX_LDS_MAX, "sdc_conv_pw_x3");
        hipLaunchKernelGGL((conv_pw_x3_kernel<TM, TN, false>), dim3((unsigned)(a.nwalk * a.MT)), dim3(PX_NT), lds, s, a);
    }
    return sdc::check_launch("sdc_conv_pw_x3");
}

}  // namespace

namespace sdcconv {

// the Cout block of a conv: the widest of 128, 96 and 64 channels that divides Cout and whose three images fit the LDS beside the bias
// (0: none)
int pw_x3_block(int K, int Cout) {
    for (const int mb : {128, 96, 64})
        if (Cout % mb == 0 && (size_t)3 * K * mb * 2 + mb * sizeof(float) <= (size_t)PX_LDS_MAX) return mb;
    return 0;
}

int launch_pw_x3(const ConvArgs& c, hipStream_t s) {
    const SdcConvDesc& d = c.d;
    PwX3Args a;
    a.x0 = c.x0; a.x1 = c.x1; a.wp = c.wp; a.bias = c.bias; a.res = c.res; a.y = c.y;
    a.x0s1 = d.x0s[1]; a.x1s1 = d.x1s[1]; a.ys1 = d.ys[1]; a.rs1 = d.rs[1];
    // (B == 1: the sample stride is never multiplied by anything but 0)
    a.x0s0 = d.B > 1 ? (int)d.x0s[0] : 0; a.x1s0 = d.B > 1 ? (int)d.x1s[0] : 0; a.ys0 = d.B > 1 ? (int)d.ys[0] : 0; a.rs0 = d.B > 1 ? (int)d.rs[0] : 0;
    a.Cin0 = d.Cin0; a.K = d.Cin0 + d.Cin1; a.Cout = d.Cout; a.S = d.oD * d.oH * d.oW; a.Ntot = c.Ntot;
    unsigned ncu = 0;
    if (const int rc = sdc::ta_grid("sdc_conv_pw_x3", 1 << 30, &ncu)) return rc;
    const int mb = pw_x3_block(a.K, a.Cout);
    return mb == 128 ? launch_px<4, 2>(a, (int)ncu, s) : mb == 96 ? launch_px<3, 2>(a, (int)ncu, s) : launch_px<2, 2>(a, (int)ncu, s);
}

}  // namespace sdcconv
