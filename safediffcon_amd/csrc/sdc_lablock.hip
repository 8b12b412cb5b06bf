// Fused LinearAttention block (Residual(PreNorm(dim, LinearAttention(dim))), heads 4 x dim_head 32, dim C in {64,128}):
//
//   y = x + post( Wo . LA(pre(x)) + bo ),   LA: q = softmax_d(Wq xn) * 32^-0.5, k = softmax_n(Wk xn), v = Wv xn,
//                                               ctx = k v^T (32x32 per head), out = ctx^T q
// 1D/model/unet.py:182-222 (+ PreNorm :64-71, LayerNorm :53-63), tokamak/model/unet.py:186-222 (RMSNorm :45-51),
// conv3d.py:232-258 (SpatialLinearAttention, PreNorm :176-184).
//
// The unfused chain writes xn, q/k/v (3 x 128 channels), out (128 channels) and the projected y to HBM and reads them
// back -- ~27 x the bytes of x per block at C = 64.  Here x is read three times and y written once:
//   pass 1  la_blk_ctx : x tile -> channel norm -> K^T = xn^T Wk^T on the matrix cores -> online softmax over tokens
//                        (running max per d, rescaled accumulators) -> M^T[c][d] += sum_tok xn[c][tok] p[tok][d]
//                        (ctx = M Wv^T / rowsum: V is never formed per token)
//   mid     la_blk_mid : merge the token splits (log-sum-exp), ctx = M Wv^T / sum, T[co][h,d] = sum_e Wo[co][h,e] ctx_h[d][e]
//   pass 2  la_blk_out : x tile -> channel norm -> Q = Wq xn -> softmax over d, * scale -> y = T q + bo -> channel
//                        norm (LayerNorm / RMSNorm / none) -> + x -> store
// All products are v_mfma_f32_32x32x2_f32 (fp32 in, fp32 accumulate).  Tokens contiguous, n % 64 == 0.
#include "sdc_common.h"
#include "sdc_lablock_pass.h"

namespace {

// The fp32 build of the pass bodies (sdc_lablock_pass.h): xn as one fp32 image xs[c][tok], weight fragments as C/2 floats.
struct La32 {
    // byte offsets into the dynamic LDS; pass 1 leaves pass 2's q image empty: both passes have the same offsets
    template <int C> struct Ctx {
        static constexpr int XS = 0, RED = 4 * (C + HID) * XP, GCOEF = RED + 4 * 8 * TT;
        static constexpr size_t BYTES = GCOEF + 4 * 2 * C;
    };
    template <int C> struct Out {
        static constexpr int XS = 0, QS = 4 * C * XP, RED = QS + 4 * HID * XP, XR = RED + 4 * 8 * TT, BG = XR + 4 * C * XP;
        static constexpr size_t BYTES = BG + 4 * 2 * C;
    };
    template <int C> using W = float[C / 2];        // W_h[d = l31][c = 2ks + lh] (a plain array, as in the bf16-split policy)
    template <int C>
    static __device__ __forceinline__ void load_w(const float* __restrict__ wqkv, int col, int lh, W<C>& w) {
#pragma unroll
        for (int ks = 0; ks < C / 2; ++ks) w[ks] = wqkv[(int64_t)(2 * ks + lh) * (3 * HID) + col];
    }
    template <int C, class L>
    static __device__ __forceinline__ void norm(float (&v)[C / 4], const LaArgs& a, const L& l, float* __restrict__ xr, int tid) {
        constexpr int CG = C / 4;
        const int tok = tid & 63, grp = tid >> 6;
        float o[CG];
        norm_tile_regs<C>(v, a.g_pre, a.pre_mode, a.eps, xr, l.red, tid, o);
#pragma unroll
        for (int k = 0; k < CG; ++k) l.xs[(grp * CG + k) * XP + tok] = o[k];
        __syncthreads();
    }
    // acc[j][r]: XA, K^T[tok = j*32 + crow(r, lh)][d = l31]; otherwise (W_h xn)[d = crow(r, lh)][tok = j*32 + l31]
    template <int C, bool XA, class L>
    static __device__ __forceinline__ void project(const W<C>& w, const L& l, int l31, int lh, f32x16 (&acc)[2]) {
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc[0][r] = 0.f; acc[1][r] = 0.f; }
#pragma unroll
        for (int ks = 0; ks < C / 2; ++ks) {
            const float x0 = l.xs[(2 * ks + lh) * XP + l31], x1 = l.xs[(2 * ks + lh) * XP + 32 + l31];
            acc[0] = XA ? __builtin_amdgcn_mfma_f32_32x32x2f32(x0, w[ks], acc[0], 0, 0, 0) : __builtin_amdgcn_mfma_f32_32x32x2f32(w[ks], x0, acc[0], 0, 0, 0);
            acc[1] = XA ? __builtin_amdgcn_mfma_f32_32x32x2f32(x1, w[ks], acc[1], 0, 0, 0) : __builtin_amdgcn_mfma_f32_32x32x2f32(w[ks], x1, acc[1], 0, 0, 0);
        }
    }
    static __device__ __forceinline__ float max3(float a, float b, float c) { return la_max3(a, b, c); }
};

// pass 1; C = 128 needs 67 KB of LDS: dynamic
template <int C, bool GN>
__global__ __launch_bounds__(NT, (C == 64 ? 2 : 1)) SDC_NO_DS_MERGE void la_blk_ctx(const LaArgs a) { la_ctx_body<C, GN, La32>(a); }

// ------------------------------------------------------------------ mid: per (sequence, head)
template <int C>
__global__ __launch_bounds__(NT) void la_blk_mid(const LaArgs a) {
    __shared__ float Ms[32][C + 1];
    __shared__ float cs[32][33];
    __shared__ float fsp[8][32];                    // per split: exp(m_s - m) ; nsplit <= 8
    __shared__ float rs[32];
    const int tid = threadIdx.x;
    const int head = blockIdx.x, seq = blockIdx.y;
    const float* pb = a.part + ((int64_t)seq * a.nsplit * 4 + head) * (32 * (C + 2));
    const int64_t sstride = (int64_t)4 * 32 * (C + 2);
    if (tid < 32) {
        float m = -INFINITY;
        for (int s = 0; s < a.nsplit; ++s) m = fmaxf(m, pb[s * sstride + 32 * C + tid]);
        float tot = 0.f;
        for (int s = 0; s < a.nsplit; ++s) {
            const float f = __expf(pb[s * sstride + 32 * C + tid] - m);
            fsp[s][tid] = f;
            tot += f * pb[s * sstride + 32 * C + 32 + tid];
        }
        rs[tid] = 1.0f / tot;
    }
    __syncthreads();
    for (int e = tid; e < 32 * C; e += NT) {
        const int d = e / C, c = e - d * C;
        float v = 0.f;
        for (int s = 0; s < a.nsplit; ++s) v += fsp[s][d] * pb[s * sstride + e];
        Ms[d][c] = v;
    }
    __syncthreads();
    // ctx[d][e] = sum_c M[d][c] Wv[e][c] / rowsum[d]
    for (int q = tid; q < 32 * 32; q += NT) {
        const int d = q >> 5, e = q & 31;
        float v = 0.f;
        for (int c = 0; c < C; ++c) v += Ms[d][c] * a.wqkv[(int64_t)c * (3 * HID) + 2 * HID + head * 32 + e];
        cs[d][e] = v * rs[d];
    }
    __syncthreads();
    // Tt[h*32 + d][co] = sum_e Wo[(h*32 + e)][co] ctx[d][e]
    float* tb = a.tt + (int64_t)seq * HID * C + (int64_t)head * 32 * C;
    for (int q = tid; q < 32 * C; q += NT) {
        const int d = q / C, co = q - d * C;
        float v = 0.f;
#pragma unroll 8
        for (int e = 0; e < 32; ++e) v += a.wo[(int64_t)(head * 32 + e) * C + co] * cs[d][e];
        tb[d * C + co] = v;
    }
}

// pass 2
template <int C>
__global__ __launch_bounds__(NT, (C == 64 ? 2 : 1)) SDC_NO_DS_MERGE void la_blk_out(const LaArgs a) { la_out_body<C, La32>(a); }

}  // namespace

extern "C" size_t sdc_linattn_block_bytes(int outer, int inner, int C, int64_t n) {
    if (outer <= 0 || inner <= 0 || n <= 0 || (C != 64 && C != 128)) return 0;
    const int64_t nseq = (int64_t)outer * inner;
    return sizeof(float) * (la_part_floats(nseq, C, n) + (size_t)(nseq * HID * C));
}

int sdc::la_launch_ctx(const LaArgs& a, int C, dim3 grid, hipStream_t stream) {
    const size_t ldsb = la_ctx_bytes<La32>(C);
    static std::atomic<uint64_t> attr{0};
    SDC_LDS_OPTIN(attr, (la_blk_ctx<128, false>), 96 * 1024, "sdc_linattn_block_bwd");
    if (C == 64) hipLaunchKernelGGL((la_blk_ctx<64, false>), grid, dim3(NT), ldsb, stream, a);
    else hipLaunchKernelGGL((la_blk_ctx<128, false>), grid, dim3(NT), ldsb, stream, a);
    return SDC_OK;
}

namespace {
int linattn_block_impl(const float* x, const float* gn_stats, const float* gn_gamma, const float* gn_beta, int gn_G,
                       const float* gn_res, const float* g_pre, const float* wqkv, const float* wo, const float* bo,
                       const float* g_post, float* work, float* y, int outer, int inner, int C, int64_t n,
                       int64_t so, int64_t sc, int64_t si, int pre_mode, int post_mode, float eps, int impl, void* stream) {
    const char* who = "sdc_linattn_block";
    SDC_REQUIRE(x && g_pre && wqkv && wo && work && y, SDC_ENULL, "%s: null pointer", who);
    // impl 0: every product on the fp32 pipe (la_blk_ctx / la_blk_out); 1: the q / k projections as bf16 splits (sdc_lablock_x3.hip)
    SDC_REQUIRE(impl == 0 || impl == 1, SDC_EINVAL, "%s: impl must be 0 or 1 (got %d)", who, impl);
    LaArgs a;
    LaGrids g;
    const int rc0 = la_host_setup(who, a, x, gn_stats, gn_gamma, gn_beta, gn_G, gn_res, g_pre, bo, g_post, work, y, outer, inner, C, n, so, sc,
                                  si, pre_mode, post_mode, eps, g, &a.tt);
    if (rc0 != SDC_OK) return rc0;
    a.wqkv = wqkv; a.wo = wo;
    hipStream_t s = sdc::as_stream(stream);
    const size_t ldsb = la_ctx_bytes<La32>(C), ldsb2 = la_out_bytes<La32>(C);
    static std::atomic<uint64_t> attr0{0}, attr1{0}, attr2{0};
    static std::atomic<uint64_t> attr3{0};
    SDC_LDS_OPTIN(attr0, (la_blk_ctx<128, false>), 96 * 1024, who);
    SDC_LDS_OPTIN(attr1, la_blk_out<128>, 128 * 1024, who);
    SDC_LDS_OPTIN(attr2, la_blk_out<64>, 96 * 1024, who);
    SDC_LDS_OPTIN(attr3, (la_blk_ctx<128, true>), 96 * 1024, who);
    const bool gn = gn_stats != nullptr;
    LaArgs a2 = a;                                  // pass 2 of the GroupNorm-on-load form: x = the h pass 1 left in y
    if (gn) { a.gn_hout = y; a2.x = y; a2.gn_stats = nullptr; }
    if (impl == 1) {
        int rc = sdc::la_x3_launch_ctx(a, C, gn, g.ctx, s);
        if (rc != SDC_OK) return rc;
        if (C == 64) hipLaunchKernelGGL(la_blk_mid<64>, g.mid, dim3(NT), 0, s, a);
        else hipLaunchKernelGGL(la_blk_mid<128>, g.mid, dim3(NT), 0, s, a);
        rc = sdc::la_x3_launch_out(a2, C, g.out, s);
        if (rc != SDC_OK) return rc;
    } else if (C == 64) {
        if (gn) hipLaunchKernelGGL((la_blk_ctx<64, true>), g.ctx, dim3(NT), ldsb, s, a);
        else hipLaunchKernelGGL((la_blk_ctx<64, false>), g.ctx, dim3(NT), ldsb, s, a);
        hipLaunchKernelGGL(la_blk_mid<64>, g.mid, dim3(NT), 0, s, a);
        hipLaunchKernelGGL(la_blk_out<64>, g.out, dim3(NT), ldsb2, s, a2);
    } else {
        if (gn) hipLaunchKernelGGL((la_blk_ctx<128, true>), g.ctx, dim3(NT), ldsb, s, a);
        else hipLaunchKernelGGL((la_blk_ctx<128, false>), g.ctx, dim3(NT), ldsb, s, a);
        hipLaunchKernelGGL(la_blk_mid<128>, g.mid, dim3(NT), 0, s, a);
        hipLaunchKernelGGL(la_blk_out<128>, g.out, dim3(NT), ldsb2, s, a2);
    }
    return sdc::check_launch(who);
}
}  // namespace

extern "C" int sdc_linattn_block_sel(const float* x, const float* g_pre, const float* wqkv, const float* wo, const float* bo,
                                     const float* g_post, float* work, float* y, int outer, int inner, int C, int64_t n,
                                     int64_t so, int64_t sc, int64_t si, int pre_mode, int post_mode, float eps, int impl, void* stream) {
    return linattn_block_impl(x, nullptr, nullptr, nullptr, 0, nullptr, g_pre, wqkv, wo, bo, g_post, work, y, outer, inner, C, n, so, sc,
                              si, pre_mode, post_mode, eps, impl, stream);
}

extern "C" int sdc_linattn_block(const float* x, const float* g_pre, const float* wqkv, const float* wo, const float* bo,
                                 const float* g_post, float* work, float* y, int outer, int inner, int C, int64_t n,
                                 int64_t so, int64_t sc, int64_t si, int pre_mode, int post_mode, float eps, void* stream) {
    return sdc_linattn_block_sel(x, g_pre, wqkv, wo, bo, g_post, work, y, outer, inner, C, n, so, sc, si, pre_mode, post_mode, eps,
                                 sdc_linattn_block_x3_ok(C, n), stream);
}

extern "C" int sdc_linattn_block_gn_sel(const float* x_raw, const float* gn_stats, const float* gn_gamma, const float* gn_beta, int gn_G,
                                        const float* gn_residual, const float* g_pre, const float* wqkv, const float* wo, const float* bo,
                                        const float* g_post, float* work, float* y, int outer, int inner, int C, int64_t n,
                                        int64_t so, int64_t sc, int64_t si, int pre_mode, int post_mode, float eps, int impl, void* stream) {
    SDC_REQUIRE(gn_stats && gn_gamma && gn_beta, SDC_ENULL, "sdc_linattn_block_gn: null GroupNorm pointer");
    SDC_REQUIRE(gn_G > 0 && (C == 64 || C == 128) && C % gn_G == 0, SDC_EINVAL, "sdc_linattn_block_gn: groups must divide the channels");
    return linattn_block_impl(x_raw, gn_stats, gn_gamma, gn_beta, gn_G, gn_residual, g_pre, wqkv, wo, bo, g_post, work, y, outer, inner,
                              C, n, so, sc, si, pre_mode, post_mode, eps, impl, stream);
}

extern "C" int sdc_linattn_block_gn(const float* x_raw, const float* gn_stats, const float* gn_gamma, const float* gn_beta, int gn_G,
                                    const float* gn_residual, const float* g_pre, const float* wqkv, const float* wo, const float* bo,
                                    const float* g_post, float* work, float* y, int outer, int inner, int C, int64_t n,
                                    int64_t so, int64_t sc, int64_t si, int pre_mode, int post_mode, float eps, void* stream) {
    return sdc_linattn_block_gn_sel(x_raw, gn_stats, gn_gamma, gn_beta, gn_G, gn_residual, g_pre, wqkv, wo, bo, g_post, work, y, outer,
                                    inner, C, n, so, sc, si, pre_mode, post_mode, eps, sdc_linattn_block_x3_ok(C, n), stream);
}
