// Tile helpers shared by the two 7-tap stem conv kernels (sdc_conv_stem_f16.hip: fp16 operands; sdc_conv_stem_x3.hip: bf16-split
// operands): the tile geometry, the common kernel arguments and their host fill, a workgroup's tile, and the KH / ITB launch ladder.
// The walk itself is described in sdc_conv_stem_f16.hip.  The row staging, the halo zeroing, the fragment bases and the epilogue are
// the same text in both kernels but stay there: as functions of this header they compiled to other instructions
// (profiles/share_headers_isa.log).
#pragma once
#include "sdc_conv.h"

namespace {

constexpr int STEM_BM = 64, STEM_BN = 256, STEM_NT = 256;      // tile: output channels x positions; threads (4 waves of 2 x 2 32x32 accumulators)

// The members the two kernels' argument structs share, in their kernel-argument order (WT w: the packed weights, _Float16 or __bf16).
// Each kernel keeps a struct of its own name: the kernels' symbol names carry it.
#define STEM_TILE_ARGS(WT, w)                                                                                                          \
    const float* x;                                                                                                                    \
    const WT* w;                                                                                                                       \
    const float* bias;                                                                                                                 \
    float* y;                                                                                                                          \
    int64_t xs[5], ys[5];                                                                                                              \
    int B, Cin, Cout, oD, oH, W, lgW;                                                                                                  \
    int kD;                                                                                                                            \
    int Hs, NR;               /* rows of a plane a tile can hold, staged slot rows (planes a tile can touch * (Hs + KH - 1)) */        \
    int Ntot, ntiles, mtiles;                                                                                                          \
    int itemsB;               /* NR * W staged positions */

// The tile of a workgroup: m0 / n0 its first output channel / position, r0 its first row in the (b, od, oh) walk, (plane0, oh0) that
// row's plane and row in the plane
struct StemTile { int m0, n0, r0, plane0, oh0; };
template <class A>
__device__ __forceinline__ StemTile stem_tile(const A& a) {
    const int logical = sdcconv::xcd_tile(blockIdx.x, a.ntiles * a.mtiles);
    const int mt = logical % a.mtiles, nt = logical / a.mtiles;
    const int m0 = mt * STEM_BM, n0 = nt * STEM_BN;
    const int r0 = n0 >> a.lgW;
    const int plane0 = r0 / a.oH, oh0 = r0 - plane0 * a.oH;
    return StemTile{m0, n0, r0, plane0, oh0};
}

// ---- host side of launch_stem_f16 / launch_stem_x3

// the common members of the arguments from the descriptor and its staging geometry (the weight pointer is the launcher's); errors are
// reported under the entry's name
template <class A>
inline int stem_fill_args(const char* entry, const SdcConvDesc& d, const sdcconv::StemShape& sh, const float* x, const float* bias, float* y, A& a) {
    a.x = x; a.bias = bias; a.y = y;
    for (int i = 0; i < 5; ++i) { a.xs[i] = d.x0s[i]; a.ys[i] = d.ys[i]; }
    a.B = d.B; a.Cin = d.Cin0; a.Cout = d.Cout; a.oD = d.oD; a.oH = d.oH; a.W = d.oW;
    a.lgW = d.oW == 16 ? 4 : d.oW == 32 ? 5 : d.oW == 64 ? 6 : 7;
    a.kD = d.kD;
    a.Hs = sh.Hs; a.NR = sh.NR;
    const int64_t ntot = (int64_t)d.B * d.oD * d.oH * d.oW;
    SDC_REQUIRE(ntot < (1ll << 31), SDC_EINVAL, "%s: too many output positions", entry);
    a.Ntot = (int)ntot;
    a.ntiles = (a.Ntot + STEM_BN - 1) / STEM_BN; a.mtiles = d.Cout / STEM_BM;
    a.itemsB = sh.itemsB;
    SDC_REQUIRE((int64_t)a.ntiles * a.mtiles < (1ll << 31), SDC_EINVAL, "%s: grid too large", entry);
    return SDC_OK;
}

// The instance ladder: KH by the tap shape, ITB (staged positions per thread) by the staged positions.  KERNEL is the kernel template's
// name; d, sh, a, lds (bytes) and s (stream) are the launcher's.
#define STEM_LAUNCH_ONE(KERNEL, ENTRY, KH, ITB)                                                                      \
    do {                                                                                                            \
        static std::atomic<uint64_t> attr{0};                                                                       \
        SDC_LDS_OPTIN(attr, (KERNEL<KH, ITB>), 160 * 1024, ENTRY);                                                  \
        hipLaunchKernelGGL((KERNEL<KH, ITB>), dim3((unsigned)(a.ntiles * a.mtiles)), dim3(STEM_NT), lds, s, a);     \
    } while (0)
#define STEM_LAUNCH(KERNEL, ENTRY)                                                                                  \
    do {                                                                                                            \
        if (d.kH == 1) STEM_LAUNCH_ONE(KERNEL, ENTRY, 1, 1);      /* (256 / W rows of W columns: one position per thread) */ \
        else if (sh.itemsB <= 2 * STEM_NT) STEM_LAUNCH_ONE(KERNEL, ENTRY, 7, 2);                                    \
        else if (sh.itemsB <= 4 * STEM_NT) STEM_LAUNCH_ONE(KERNEL, ENTRY, 7, 4);                                    \
        else STEM_LAUNCH_ONE(KERNEL, ENTRY, 7, 8);                                                                  \
    } while (0)

}  // namespace
