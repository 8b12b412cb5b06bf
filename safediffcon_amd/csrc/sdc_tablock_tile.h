// Tile helpers shared by the fused temporal-attention block kernels (sdc_tablock.hip: fp32 operands; sdc_tablock_f16.hip: fp16
// operands; sdc_tablock_x3.hip: bf16-split projections; sdc_tablock_bwd.hip: the fp32 block's backward): the kernel arguments,
// the tile geometry, the wave-uniform-base global accesses, the workgroup walk, and the host entries' common checks and grid choice.
//
// The three forward kernels differ in their weight arguments only (the backward adds dy and its workspace there; its y is dx).
// A translation unit names them before it includes this header,
//   #define TA_WEIGHT_ARGS const float* wqkv; const float* wo;
// and gets its own TaArgs (the kernels' symbol names carry the type's name, the kernel arguments its layout).
#pragma once
#include "sdc_common.h"
#include <cstdlib>

#ifndef TA_WEIGHT_ARGS
#error "define TA_WEIGHT_ARGS (the weight pointer members of TaArgs) before including sdc_tablock_tile.h"
#endif

namespace sdc {

// The launch grid of the three entries: one persistent workgroup per CU (125 - 157 KB of LDS: one fits), at most one per pixel group.
// Defined in sdc_tablock.hip, which owns the per-device CU-count cache; errors are reported under the entry's name.
int ta_grid(const char* entry, int64_t nblk, unsigned* grid);

}  // namespace sdc

namespace {

constexpr int NT = 512;                  // 8 waves: one pixel each, two waves per SIMD
constexpr int C = 64;
constexpr int NS = 8;                    // pixels per workgroup
constexpr int XP = NS * 33;              // LDS pitch of one channel row of the y image (the fp32 kernel: of xn too): [pixel][33 frames]
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float nfloat4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct TaArgs {
    const float* x; const float* g; TA_WEIGHT_ARGS const float* rot; const float* bias;
    float* y;
    int inner;               // pixels per outer index (H*W)
    int nblk;                // pixel groups of NS
    float eps;
    int64_t so, sc, st;      // element (o, c, pixel i, frame f) at o*so + c*sc + f*st + i
#ifdef SDC_KERNEL_EXPERIMENTS
    int dbg;                 // kernel experiments of ta_block_kernel (SDC_TA_DBG; WRONG RESULTS): 1 no head loop, 2 no weight fetches, 4 no softmax / rotary
#define TA_DBG(a) ((a).dbg)
#else
#define TA_DBG(a) 0         // the shipping library has no result-changing switches (build with -DSDC_KERNEL_EXPERIMENTS for them)
#endif
};
#undef TA_WEIGHT_ARGS

// accumulator register r of half-wave lh holds row crow(r, lh) of a 32x32 MFMA tile
__host__ __device__ __forceinline__ int crow(int r, int lh) { return (r & 3) + 8 * (r >> 2) + 4 * lh; }

// wave-uniform base (SGPR pair) + 32-bit per-lane byte offset: `global_load_dword v, v_off, s[base:base+1]` -- one VGPR of
// address for all 32 channel rows of a token instead of a 64-bit pointer per row
typedef __attribute__((address_space(1))) float* gptr_t;
typedef __attribute__((address_space(1))) char* gcptr_t;
__device__ __forceinline__ gptr_t uni(const float* p) {
    const uint64_t u = reinterpret_cast<uint64_t>(p);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)u), hi = __builtin_amdgcn_readfirstlane((uint32_t)(u >> 32));
    return (gptr_t)(((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ float ldu(gptr_t base, uint32_t byte_off) { return *(gptr_t)((gcptr_t)base + byte_off); }
__device__ __forceinline__ void stu(gptr_t base, uint32_t byte_off, float v) { *(gptr_t)((gcptr_t)base + byte_off) = v; }

// (cos, sin) pairs of the rotary step; each kernel has its own ta_rot (packed inline assembly on the fp32 pipe, plain C++ where bf16
// MFMA accumulators are its inputs: DESIGN.md section 19)
typedef float ta2 __attribute__((ext_vector_type(2)));

// Persistent workgroups (one per CU) walk the pixel groups.  XCD-aware: workgroup w runs on XCD w & 7 (round-robin dispatch); each
// XCD takes a contiguous eighth of the pixel groups and its workgroups interleave over it, so the 4 groups sharing a 128-byte line
// are in flight on one XCD at about the same time (speed only).  A workgroup's tiles are li = first, first + stride, .. < per.
struct TaWalk { int per, base, first, stride; };
__device__ __forceinline__ TaWalk ta_walk(int nblk) {
    const int nwg = gridDim.x, w = blockIdx.x;
    const bool xcd = ((nblk & 7) == 0) && ((nwg & 7) == 0);
    const int per = xcd ? (nblk >> 3) : nblk;             // tiles of this workgroup's share
    const int base = xcd ? (w & 7) * per : 0;
    const int first = xcd ? (w >> 3) : w, stride = xcd ? (nwg >> 3) : nwg;
    return TaWalk{per, base, first, stride};
}
// element offset of tile li's first pixel, channel 0, frame 0
__device__ __forceinline__ int64_t ta_tile_ptr(const TaArgs& a, const TaWalk& wk, int li) {
    const int seq0 = (wk.base + li) * NS;
    const int o = seq0 / a.inner, i0 = seq0 - o * a.inner;
    return (int64_t)o * a.so + i0;
}

// ---- host side of the three sdc_tattn_block* entries

// The checks the entries share, under the entry's own name, and the members of TaArgs they share.  The weight pointers are the entry's.
inline int ta_check_args(const char* entry, const float* x, const float* g_pre, const float* rot, const float* bias, float* y, int outer,
                         int inner, int Cc, int ntok, int64_t so, int64_t sc, int64_t st, float eps, TaArgs& a) {
    SDC_REQUIRE(x && g_pre && y, SDC_ENULL, "%s: null pointer", entry);
    SDC_REQUIRE(Cc == 64 && ntok == 32, SDC_EINVAL, "%s: dim 64 and 32 frames only (got %d, %d)", entry, Cc, ntok);
    SDC_REQUIRE(outer > 0 && inner > 0 && inner % NS == 0, SDC_EINVAL, "%s: pixels per image must be a multiple of 8", entry);
    const int64_t nblk = (int64_t)outer * inner / NS;
    SDC_REQUIRE(nblk < (1ll << 31), SDC_EINVAL, "%s: too many sequences", entry);
    SDC_REQUIRE(((int64_t)31 * st + inner + (int64_t)63 * sc) * 4 < (1ll << 32) && so >= 0 && sc >= 0 && st >= 0, SDC_EINVAL,
                "%s: one outer index must span less than 4 GB (32-bit lane offsets)", entry);
    a.x = x; a.g = g_pre; a.rot = rot; a.bias = bias; a.y = y;
    a.inner = inner; a.nblk = (int)nblk; a.eps = eps; a.so = so; a.sc = sc; a.st = st;
#ifdef SDC_KERNEL_EXPERIMENTS
    static const int dbg = getenv("SDC_TA_DBG") ? atoi(getenv("SDC_TA_DBG")) : 0;
    a.dbg = dbg;
#endif
    return SDC_OK;
}

}  // namespace
