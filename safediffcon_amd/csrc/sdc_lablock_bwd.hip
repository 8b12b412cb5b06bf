// Backward of the fused LinearAttention block (sdc_lablock.hip, SpatialLinearAttention form: channel LayerNorm in front, no norm
// behind) for fine-tuning: given dy, the gradient of
//
//   y = x + Wo . LA(xn) + bo,   xn = channel LayerNorm(x) * gamma,
//   LA per head: s = softmax_d(Wq xn), q~ = 32^-0.5 s, p = softmax_n(Wk xn), ctx = p (Wv xn)^T, out = ctx^T q~
//
// with respect to x, gamma, Wqkv, Wo and bo from x and dy alone: xn, Q, K, p, dQ, dK and dxn are recomputed tile by tile and never
// leave the chip; V is never formed per token in either direction.  The token reductions collapse to small tables per (sequence,
// head): M^[d][c] = sum_n p xn, ctx = M^ Wv^T, T = Wo ctx (as the forward has them) and, backwards,
//   dT[co][hd] = sum_n dy[co,n] q~[hd,n]                           -- the only token reduction of the first sweep
//   dctx = dT^T Wo, dWo += dT ctx, U = dctx Wv, dWv += dctx^T M^, delta[d] = sum_e dctx ctx  (= sum_n p dp: the token softmax's
//   backward needs no sweep of its own)
// Launches per chunk of at most lab_slots() sequences (the workspace holds that many sequence slots, whatever outer * inner is):
//   1. la_blk_ctx (sdc_lablock.hip, unchanged, fp32) : the token-split partials of M^T, running max and sum
//   2. lab_mid1  : merge the splits -> kmax, 1 / ksum, M^, ctx, T
//   3. lab_dt    : x, dy tile -> xn -> q~ -> dT and dbo partials per (sequence, split)
//   4. lab_mid2  : the small tables above; dWo, dWv per sequence slot
//   5. lab_dx    : x, dy tile -> xn, s, p -> dq~ = T^T dy, dQ, dp = U xn, dK -> dxn = Wq^T dQ + Wk^T dK + U^T p -> LayerNorm
//                  backward + residual -> dx;  dWq, dWk, dgamma partials per (sequence, split)
//   6. lab_sum   : the partial tables in a fixed order (the first chunk overwrites the outputs, later chunks add to them)
// The post-norm form of the 1-D nets (sdc_linattn_block_post_bwd), y = x + N_post(Wo . LA(N_pre(x)) + bo) g_post
// with N in {channel LayerNorm, RMSNorm}, runs the same launches with the POST instantiations of the two sweeps: lab_dt also forms
// z = T q~ + bo, the post norm's backward dz and dg_post, uses dz for dy and leaves the dz tile in dx's memory; lab_dx reads it there
// in dy's place and adds dy itself only as the residual.
// All matrix products are v_mfma_f32_32x32x2_f32.  No atomics; every partial has one owner and is written in full; the token splits
// are pick_nsplit's (a function of the sequence length only), so a sequence's dx does not depend on what shares the launch.
#include "sdc_common.h"
#include "sdc_lablock_tile.h"

namespace {

// sequence slots of the workspace = sequences per chunk: a function of the split count (that is, of the sequence length) only;
// slots x splits <= 256 bounds the per-split tables and gives a chunk's sweeps up to 256 workgroups
inline int lab_slots(int ns) { const int s = 256 / ns; return s > 128 ? 128 : s; }
constexpr float SCALE = 0.17677669529663687f;   // dim_head^-0.5
#define MFMA(a_, b_, c_) __builtin_amdgcn_mfma_f32_32x32x2f32(a_, b_, c_, 0, 0, 0)

// the workspace: offsets in floats.  Every region but wt is [slot][...]; ns = pick_nsplit's (unclamped) split count
struct LabWs {
    int64_t part;       // [ns][4][32 (C + 2)]      la_blk_ctx's partials
    int64_t stat;       // [2][128]                 kmax | 1 / ksum
    int64_t mh;         // [128 hd][C]              M^ (normalised)
    int64_t ctx;        // [4][32 d][32 e]
    int64_t tq;         // [4][C co][32 d]          T
    int64_t dtp;        // [ns][128 hd][C co]       dT partials
    int64_t dbop;       // [ns][C]                  dbo partials
    int64_t u;          // [128 hd][C]              U
    int64_t ut;         // [4][C][32 d]             U, d contiguous
    int64_t delta;      // [128]
    int64_t tabqk;      // [ns][C (256 + 1)]        dWq | dWk partials as [C][256], then dgamma [C]
    int64_t tabv;       // [C][128]                 dWv of the slot's sequences
    int64_t tabo;       // [128][C]                 dWo
    int64_t wt;         // [256 hd][C]              Wq | Wk with c contiguous (one copy per call)
    int64_t tt;         // [128 hd][C co]           T with co contiguous        (post-norm form only)
    int64_t dgpp;       // [ns][C]                  dg_post partials            (post-norm form only)
    int64_t total;
};

inline LabWs lab_layout(int C, int ns, int nslot, bool post = false) {
    LabWs L;
    int64_t o = 0;
    const int64_t s = nslot;
    L.part = o;  o += s * ns * 4 * 32 * (C + 2);
    L.stat = o;  o += s * 256;
    L.mh = o;    o += s * HID * C;
    L.ctx = o;   o += s * 4 * 1024;
    L.tq = o;    o += s * HID * C;
    L.dtp = o;   o += s * ns * HID * C;
    L.dbop = o;  o += s * ns * C;
    L.u = o;     o += s * HID * C;
    L.ut = o;    o += s * HID * C;
    L.delta = o; o += s * HID;
    L.tabqk = o; o += s * ns * (C * 257);
    L.tabv = o;  o += s * C * HID;
    L.tabo = o;  o += s * HID * C;
    L.wt = o;    o += 256 * C;
    L.tt = o;    if (post) o += s * HID * C;
    L.dgpp = o;  if (post) o += s * ns * C;
    L.total = o;
    return L;
}

struct LabArgs {
    const float* x; const float* dy; const float* g; const float* wqkv; const float* wo;
    float* dx; float* ws;
    const float* bo; const float* gp;               // post-norm form: the output bias (or null) and the post norm's gain
    LabWs L;
    int inner, ns0, nsplit, tiles_per_split, ntiles;
    int pre_mode, post_mode;                        // 0 LayerNorm, 1 RMSNorm; post_mode -1: no post norm
    float eps;
    int64_t so, sc, si;
};

// wt[hd][c] = wqkv[c][hd] for the q and k columns: block = c, thread = hd
__global__ __launch_bounds__(NT) void lab_wt_kernel(const float* __restrict__ wqkv, float* __restrict__ wt, int C) {
    wt[(int64_t)threadIdx.x * C + blockIdx.x] = wqkv[(int64_t)blockIdx.x * (3 * HID) + threadIdx.x];
}

// channel norm of a tile as norm_tile_regs (sdc_lablock_tile.h) has it: xs[c][tok] = xh * g; v becomes xh; returns the factor xh was scaled
// by: rstd (mode 0, LayerNorm: xh = (x - mean) rstd) or sqrt(C) / max(||x||, 1e-12) (mode 1, RMSNorm: xh = x f).  `live` is 0 where
// mode 1's clamp holds (the backward then drops the term through the norm, as sdc_chan_norm_bwd does) and 1 everywhere else.
template <int C>
__device__ __forceinline__ float ln_tile(float (&v)[C / 4], const float* __restrict__ g, int mode, float eps, float* __restrict__ xs,
                                         float* __restrict__ red, int tid, float& live) {
    constexpr int CG = C / 4;
    const int tok = tid & 63, grp = tid >> 6;
    float rstd;
    live = 1.f;
    if (mode == 0) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < CG; ++k) s += v[k];
        red[grp * TT + tok] = s;
        __syncthreads();
        const float mean = (red[tok] + red[TT + tok] + red[2 * TT + tok] + red[3 * TT + tok]) * (1.0f / C);
        float q = 0.f;
#pragma unroll
        for (int k = 0; k < CG; ++k) { v[k] -= mean; q += v[k] * v[k]; }
        red[(4 + grp) * TT + tok] = q;
        __syncthreads();
        const float var = (red[4 * TT + tok] + red[5 * TT + tok] + red[6 * TT + tok] + red[7 * TT + tok]) * (1.0f / C);
        rstd = rsqrtf(var + eps);
    } else {
        float q = 0.f;
#pragma unroll
        for (int k = 0; k < CG; ++k) q += v[k] * v[k];
        red[grp * TT + tok] = q;
        __syncthreads();
        const float nrm = sqrtf(red[tok] + red[TT + tok] + red[2 * TT + tok] + red[3 * TT + tok]);
        rstd = sqrtf((float)C) / fmaxf(nrm, 1e-12f);
        live = nrm > 1e-12f ? 1.f : 0.f;
    }
#pragma unroll
    for (int k = 0; k < CG; ++k) {
        v[k] *= rstd;
        xs[(grp * CG + k) * XP + tok] = v[k] * g[grp * CG + k];
    }
    __syncthreads();
    return rstd;
}

// Backward of the post norm on a tile (post-norm form, sweep 1).  zs[c][tok] holds z = T q~ + bo; gy the dy values of this thread's
// (channel group, token) and becomes dz; dgp gathers dg_post = sum dy u.  With u = N(z) and du = dy g_post:
//   mode 0: dz = rstd (du - mean_c du - u mean_c(du u));   mode 1: dz = f (du - u mean_c(du u)), f = sqrt(C) / max(||z||, 1e-12), the
//   second term dropped where the clamp holds (sdc_chan_norm_bwd).
// red: 12 rows; rows 0 - 7 are ln_tile's (free here: its last read lies behind a barrier), 8 - 11 take the third pair of sums.
template <int C>
__device__ __forceinline__ void post_bwd_tile(const float* __restrict__ zs, float (&gy)[C / 4], float (&dgp)[C / 4],
                                              const float* __restrict__ gp, int mode, float eps, float* __restrict__ red, int tid) {
    constexpr int CG = C / 4;
    const int tok = tid & 63, grp = tid >> 6;
    float u[CG];
#pragma unroll
    for (int k = 0; k < CG; ++k) u[k] = zs[(grp * CG + k) * XP + tok];
    float f, live = 1.f;
    if (mode == 0) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < CG; ++k) s += u[k];
        red[grp * TT + tok] = s;
        __syncthreads();
        const float mean = (red[tok] + red[TT + tok] + red[2 * TT + tok] + red[3 * TT + tok]) * (1.0f / C);
        float q = 0.f;
#pragma unroll
        for (int k = 0; k < CG; ++k) { u[k] -= mean; q += u[k] * u[k]; }
        red[(4 + grp) * TT + tok] = q;
        __syncthreads();
        const float var = (red[4 * TT + tok] + red[5 * TT + tok] + red[6 * TT + tok] + red[7 * TT + tok]) * (1.0f / C);
        f = rsqrtf(var + eps);
    } else {
        float q = 0.f;
#pragma unroll
        for (int k = 0; k < CG; ++k) q += u[k] * u[k];
        red[(4 + grp) * TT + tok] = q;
        __syncthreads();
        const float nrm = sqrtf(red[4 * TT + tok] + red[5 * TT + tok] + red[6 * TT + tok] + red[7 * TT + tok]);
        f = sqrtf((float)C) / fmaxf(nrm, 1e-12f);
        live = nrm > 1e-12f ? 1.f : 0.f;
    }
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int k = 0; k < CG; ++k) {
        u[k] *= f;
        dgp[k] += gy[k] * u[k];
        gy[k] *= gp[grp * CG + k];                  // du
        s1 += gy[k];
        s2 += gy[k] * u[k];
    }
    red[grp * TT + tok] = s1;                       // (rows 0 - 3: every thread read them before the barrier above)
    red[(8 + grp) * TT + tok] = s2;
    __syncthreads();
    const float m1 = mode == 0 ? ((red[tok] + red[TT + tok]) + (red[2 * TT + tok] + red[3 * TT + tok])) * (1.0f / C) : 0.f;
    const float m2 = ((red[8 * TT + tok] + red[9 * TT + tok]) + (red[10 * TT + tok] + red[11 * TT + tok])) * (1.0f / C) * live;
#pragma unroll
    for (int k = 0; k < CG; ++k) gy[k] = f * (gy[k] - m1 - u[k] * m2);
}

// acc[j][r] = (W xn)[d = crow(r, lh)][tok = j*32 + l31], W[d][c] = wp[c * 384 + d]: wp points at column (head*32 + l31) of row lh
template <int C>
__device__ __forceinline__ void project(const float* __restrict__ wp, const float* __restrict__ xs, int l31, int lh, f32x16 (&acc)[2]) {
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc[0][r] = 0.f; acc[1][r] = 0.f; }
#pragma unroll 8
    for (int ks = 0; ks < C / 2; ++ks) {
        const float w = wp[2 * ks * (3 * HID)];
        const float* xr = xs + (2 * ks + lh) * XP + l31;
        acc[0] = MFMA(w, xr[0], acc[0]);
        acc[1] = MFMA(w, xr[32], acc[1]);
    }
}

// softmax over d (the 32 rows: 16 registers x 2 half-waves) of each token column, in place
__device__ __forceinline__ void softmax_d(f32x16& t) {
    float m = t[0];
#pragma unroll
    for (int r = 1; r < 16; ++r) m = fmaxf(m, t[r]);
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    const float nml = -m * LOG2E;
    float s = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) { t[r] = __builtin_amdgcn_exp2f(fmaf(t[r], LOG2E, nml)); s += t[r]; }
    s += __shfl_xor(s, 32, 64);
    const float inv = 1.0f / s;
#pragma unroll
    for (int r = 0; r < 16; ++r) t[r] *= inv;
}

// ------------------------------------------------------------------ mid 1: per (head, sequence slot)
template <int C>
__global__ __launch_bounds__(NT) void lab_mid1_kernel(const LabArgs a) {
    __shared__ float Ms[32][C + 1];
    __shared__ float cs[32][33];
    __shared__ float fsp[8][32];                    // per split: exp(m_s - m); nsplit <= 8
    __shared__ float rs[32];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lh = lane >> 5;
    const int head = blockIdx.x;
    const int64_t slot = blockIdx.y;
    const float* pb = a.ws + a.L.part + ((slot * a.nsplit) * 4 + head) * (32 * (C + 2));
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
        const float r = 1.0f / tot;
        rs[tid] = r;
        float* st = a.ws + a.L.stat + slot * 256;
        st[head * 32 + tid] = m;
        st[HID + head * 32 + tid] = r;
    }
    __syncthreads();
    float* mh = a.ws + a.L.mh + slot * (HID * C) + head * 32 * C;
    for (int e = tid; e < 32 * C; e += NT) {
        const int d = e / C, c = e - d * C;
        float v = 0.f;
        for (int s = 0; s < a.nsplit; ++s) v += fsp[s][d] * pb[s * sstride + e];
        v *= rs[d];
        Ms[d][c] = v;
        mh[e] = v;
    }
    __syncthreads();
    if (wave == 0) {                                // ctx[d][e] = sum_c M^[d][c] Wv[e][c]
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        const float* wv = a.wqkv + 2 * HID + head * 32 + l31;
#pragma unroll 8
        for (int ks = 0; ks < C / 2; ++ks) { const int k = 2 * ks + lh; acc = MFMA(Ms[l31][k], wv[k * (3 * HID)], acc); }
        float* cg = a.ws + a.L.ctx + slot * 4096 + head * 1024;
#pragma unroll
        for (int r = 0; r < 16; ++r) { cs[crow(r, lh)][l31] = acc[r]; cg[crow(r, lh) * 32 + l31] = acc[r]; }
    }
    __syncthreads();
    // T[co][d] = sum_e Wo[co][h, e] ctx[d][e]
    float* tq = a.ws + a.L.tq + slot * (HID * C) + head * C * 32;
    for (int rt = wave; rt < C / 32; rt += 4) {
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) { const int k = 2 * ks + lh; acc = MFMA(a.wo[(head * 32 + k) * C + rt * 32 + l31], cs[l31][k], acc); }
#pragma unroll
        for (int r = 0; r < 16; ++r) tq[(rt * 32 + crow(r, lh)) * 32 + l31] = acc[r];
        if (a.post_mode >= 0) {                     // the post-norm form's sweep 1 forms z = T q~ with co on the lanes
            float* tt = a.ws + a.L.tt + slot * (HID * C) + (head * 32 + l31) * C + rt * 32;
#pragma unroll
            for (int r = 0; r < 16; ++r) tt[crow(r, lh)] = acc[r];
        }
    }
}

// ------------------------------------------------------------------ sweep 1: dT and dbo partials per (split, sequence); wave = head
// POST (the post-norm form): z = T q~ + bo goes over xn once every wave has projected, the post norm's backward turns the dy tile
// into dz, which takes dy's place in the products below and is left in dx's memory at the tile's own address for sweep 2
template <int C, bool POST>
__global__ __launch_bounds__(NT) void lab_dt_kernel(const LabArgs a) {
    constexpr int NCT = C / 32, CG = C / 4;
    extern __shared__ float lds[];
    float* const xs = lds;                          // [C][XP]   xn; POST: then z
    float* const dys = xs + C * XP;                 // [C][XP]   dy; POST: dz
    float* const qs = dys + C * XP;                 // [128][XP] q~
    float* const red = qs + HID * XP;               // [8][TT]; POST: [12][TT]
    const int tid = threadIdx.x, lane = tid & 63, head = tid >> 6, l31 = lane & 31, lh = lane >> 5;
    const int tok = tid & 63, grp = tid >> 6;
    const int split = blockIdx.x;
    const int64_t slot = blockIdx.y;
    const int o = (int)slot / a.inner, i = (int)slot - o * a.inner;
    const float* xseq = a.x + o * a.so + i * a.si;
    const float* dyseq = a.dy + o * a.so + i * a.si;
    const float* wq = a.wqkv + head * 32 + l31 + lh * (3 * HID);

    f32x16 dt[NCT];                                 // dT^T tile t: rows d, columns co = t*32 + l31
#pragma unroll
    for (int t = 0; t < NCT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) dt[t][r] = 0.f;
    float dbacc = 0.f;                              // channel tid (< C)
    float dgp[POST ? CG : 1];                       // POST: dg_post of channel grp*CG + k over this lane's tokens
#pragma unroll
    for (int k = 0; k < (POST ? CG : 1); ++k) dgp[k] = 0.f;
    const int pre = POST ? a.pre_mode : 0;
    const int zrt = (NCT == 2) ? (head & 1) : head; // POST: this wave's row tile of z and its first column tile (as lab_dx's dxn)
    const int zct0 = (NCT == 2) ? (head >> 1) : 0;

    const int t0 = split * a.tiles_per_split;
    const int t1 = min(t0 + a.tiles_per_split, a.ntiles);
    for (int tile = t0; tile < t1; ++tile) {
        float xv[CG], gy[CG];
        fetch_tile<C>(xseq + (int64_t)tile * TT, a.sc, tid, xv);
        fetch_tile<C>(dyseq + (int64_t)tile * TT, a.sc, tid, gy);
        if constexpr (!POST) {
#pragma unroll
            for (int k = 0; k < CG; ++k) dys[(grp * CG + k) * XP + tok] = gy[k];
        }
        float live;
        ln_tile<C>(xv, a.g, pre, a.eps, xs, red, tid, live);
        f32x16 q[2];
        project<C>(wq, xs, l31, lh, q);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            softmax_d(q[j]);
#pragma unroll
            for (int r = 0; r < 16; ++r) qs[(head * 32 + crow(r, lh)) * XP + j * 32 + l31] = q[j][r] * SCALE;
        }
        __syncthreads();
        if constexpr (POST) {
            // z[co][tok] = bo[co] + sum_hd T[co][hd] q~[hd][tok]: NCT x 2 tiles of 32 x 32 over 4 waves, T's fragments from L2
            constexpr int TPW = NCT / 2;
            f32x16 z[TPW];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float b = a.bo ? a.bo[zrt * 32 + crow(r, lh)] : 0.f;
#pragma unroll
                for (int u = 0; u < TPW; ++u) z[u][r] = b;
            }
            const float* tt = a.ws + a.L.tt + slot * (HID * C) + zrt * 32 + l31;
#pragma unroll 4
            for (int ks = 0; ks < HID / 2; ++ks) {
                const int k = 2 * ks + lh;
                const float ta = tt[k * C];
#pragma unroll
                for (int u = 0; u < TPW; ++u) z[u] = MFMA(ta, qs[k * XP + (zct0 + u) * 32 + l31], z[u]);
            }
#pragma unroll
            for (int u = 0; u < TPW; ++u)
#pragma unroll
                for (int r = 0; r < 16; ++r) xs[(zrt * 32 + crow(r, lh)) * XP + (zct0 + u) * 32 + l31] = z[u][r];
            __syncthreads();
            post_bwd_tile<C>(xs, gy, dgp, a.gp, a.post_mode, a.eps, red, tid);       // gy = dz from here on
            la_gptr dp_ = la_uni(a.dx + o * a.so + i * a.si + (int64_t)tile * TT + (int64_t)(__builtin_amdgcn_readfirstlane(grp) * CG) * a.sc);
            uint32_t off = (uint32_t)tok * 4u;
#pragma unroll
            for (int k = 0; k < CG; ++k) {
                dys[(grp * CG + k) * XP + tok] = gy[k];
                asm volatile("" : "+v"(off));
                la_st(dp_, off, gy[k]);
                dp_ += a.sc;
                asm volatile("" : "+s"(dp_));
            }
            __syncthreads();
        }
        // dT^T[hd][co] += sum_tok q~[hd][tok] dy[co][tok]      (POST: dz)
#pragma unroll 4
        for (int s = 0; s < TT / 2; ++s) {
            const int tk = 2 * s + lh;
            const float qa = qs[(head * 32 + l31) * XP + tk];
#pragma unroll
            for (int t = 0; t < NCT; ++t) dt[t] = MFMA(qa, dys[(t * 32 + l31) * XP + tk], dt[t]);
        }
        if (tid < C) {
            float s = 0.f;
            for (int t = 0; t < TT; ++t) s += dys[tid * XP + t];
            dbacc += s;
        }
        __syncthreads();                            // xs / dys / qs / red are rewritten by the next tile
    }
    float* dtp = a.ws + a.L.dtp + (slot * a.ns0 + split) * (HID * C);
#pragma unroll
    for (int t = 0; t < NCT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) dtp[(head * 32 + crow(r, lh)) * C + t * 32 + l31] = dt[t][r];
    if (tid < C) a.ws[a.L.dbop + (slot * a.ns0 + split) * C + tid] = dbacc;
    if constexpr (POST) {                           // (the tile loop ended on a barrier: xs is free)
#pragma unroll
        for (int k = 0; k < CG; ++k) xs[(grp * CG + k) * XP + tok] = dgp[k];
        __syncthreads();
        if (tid < C) {
            float s = 0.f;
            for (int t = 0; t < TT; ++t) s += xs[tid * XP + t];
            a.ws[a.L.dgpp + (slot * a.ns0 + split) * C + tid] = s;
        }
    }
}

// ------------------------------------------------------------------ mid 2: per (head, sequence slot)
template <int C>
__global__ __launch_bounds__(NT) void lab_mid2_kernel(const LabArgs a) {
    constexpr int NCT = C / 32;
    __shared__ float dTs[32][C + 1];                // dT^T[d][co] of this head
    __shared__ float Mh[32][C + 1];
    __shared__ float cs[32][33];
    __shared__ float dcs[32][33];                   // dctx[d][e]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lh = lane >> 5;
    const int head = blockIdx.x;
    const int64_t slot = blockIdx.y;
    const float* dtp = a.ws + a.L.dtp + slot * a.ns0 * (HID * C) + head * 32 * C;
    const float* mh = a.ws + a.L.mh + slot * (HID * C) + head * 32 * C;
    for (int e = tid; e < 32 * C; e += NT) {
        const int d = e / C, co = e - d * C;
        float v = 0.f;
        for (int s = 0; s < a.nsplit; ++s) v += dtp[(int64_t)s * (HID * C) + e];
        dTs[d][co] = v;
        Mh[d][co] = mh[e];
    }
    const float* cg = a.ws + a.L.ctx + slot * 4096 + head * 1024;
    for (int e = tid; e < 1024; e += NT) cs[e >> 5][e & 31] = cg[e];
    __syncthreads();
    if (wave == 0) {                                // dctx[d][e] = sum_co dT[co][h, d] Wo[co][h, e]
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        const float* wr = a.wo + (head * 32 + l31) * C;
#pragma unroll 8
        for (int ks = 0; ks < C / 2; ++ks) { const int k = 2 * ks + lh; acc = MFMA(dTs[l31][k], wr[k], acc); }
#pragma unroll
        for (int r = 0; r < 16; ++r) dcs[crow(r, lh)][l31] = acc[r];
    }
    __syncthreads();
    if (tid < 32) {
        float s = 0.f;
        for (int e = 0; e < 32; ++e) s += dcs[tid][e] * cs[tid][e];
        a.ws[a.L.delta + slot * HID + head * 32 + tid] = s;
    }
    for (int job = wave; job < 3 * NCT; job += 4) {
        const int kind = job / NCT, t = job - kind * NCT;
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        if (kind == 0) {                            // dWo[h, e][co] = sum_d ctx[d][e] dT[co][h, d]
#pragma unroll
            for (int ks = 0; ks < 16; ++ks) { const int k = 2 * ks + lh; acc = MFMA(cs[k][l31], dTs[k][t * 32 + l31], acc); }
            float* to = a.ws + a.L.tabo + slot * (HID * C);
#pragma unroll
            for (int r = 0; r < 16; ++r) to[(head * 32 + crow(r, lh)) * C + t * 32 + l31] = acc[r];
        } else if (kind == 1) {                     // U[d][c] = sum_e dctx[d][e] Wv[e][c]
            const float* wv = a.wqkv + (int64_t)(t * 32 + l31) * (3 * HID) + 2 * HID + head * 32;
#pragma unroll
            for (int ks = 0; ks < 16; ++ks) { const int k = 2 * ks + lh; acc = MFMA(dcs[l31][k], wv[k], acc); }
            float* u = a.ws + a.L.u + slot * (HID * C), * ut = a.ws + a.L.ut + slot * (HID * C) + head * C * 32;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                u[(head * 32 + crow(r, lh)) * C + t * 32 + l31] = acc[r];
                ut[(t * 32 + l31) * 32 + crow(r, lh)] = acc[r];
            }
        } else {                                    // dWv[c][h, e] = sum_d M^[d][c] dctx[d][e]
#pragma unroll
            for (int ks = 0; ks < 16; ++ks) { const int k = 2 * ks + lh; acc = MFMA(Mh[k][t * 32 + l31], dcs[k][l31], acc); }
            float* tv = a.ws + a.L.tabv + slot * (C * HID);
#pragma unroll
            for (int r = 0; r < 16; ++r) tv[(t * 32 + crow(r, lh)) * HID + head * 32 + l31] = acc[r];
        }
    }
}

// ------------------------------------------------------------------ sweep 2: dx; dWq, dWk, dgamma partials per (split, sequence)
// POST (the post-norm form): the tile sweep 1 left in dx (dz) takes dy's place in the products; dy itself only enters the residual.
// One workgroup owns a tile of dx, and each thread reads exactly the elements it overwrites at the end of the tile.
template <int C, bool POST>
__global__ __launch_bounds__(NT) void lab_dx_kernel(const LabArgs a) {
    constexpr int NCT = C / 32, CG = C / 4;
    constexpr int TPW = NCT / 2;                    // dxn tiles per wave (one row tile, TPW column tiles)
    extern __shared__ float lds[];
    float* const xs = lds;                          // [C][XP]   xn; at the end the dgamma lanes
    float* const dys = xs + C * XP;                 // [C][XP]   dy
    float* const gq = dys + C * XP;                 // [128][XP] dQ; then dxn [C][XP]
    float* const gk = gq + HID * XP;                // [128][XP] dK
    float* const pp = (C == 128) ? dys : gk + HID * XP;      // [128][XP] p (width 128: over dy, which lives on in registers)
    float* const red = (C == 128) ? gk + HID * XP : pp + HID * XP;     // [8][TT]
    float* const st = red + 8 * TT;                 // [3][128] -kmax log2e | 1 / ksum | delta
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, head = wave, l31 = lane & 31, lh = lane >> 5;
    const int tok = tid & 63, grp = tid >> 6;
    const int split = blockIdx.x;
    const int64_t slot = blockIdx.y;
    const int o = (int)slot / a.inner, i = (int)slot - o * a.inner;
    const float* xseq = a.x + o * a.so + i * a.si;
    const float* dyseq = a.dy + o * a.so + i * a.si;
    float* dxseq = a.dx + o * a.so + i * a.si;
    const int rt = (NCT == 2) ? (wave & 1) : wave;  // this wave's row tile of dxn
    const int ct0 = (NCT == 2) ? (wave >> 1) : 0;   // its first column tile

    if (tid < HID) {
        st[tid] = -a.ws[a.L.stat + slot * 256 + tid] * LOG2E;
        st[HID + tid] = a.ws[a.L.stat + slot * 256 + HID + tid];
        st[2 * HID + tid] = a.ws[a.L.delta + slot * HID + tid];
    }
    const float* wq = a.wqkv + head * 32 + l31 + lh * (3 * HID);
    const float* wk = wq + HID;
    const float* tq = a.ws + a.L.tq + slot * (HID * C) + head * C * 32 + l31;          // T[co][d = l31]
    const float* ut = a.ws + a.L.ut + slot * (HID * C) + head * C * 32 + l31;          // U[c][d = l31]
    const float* aq = a.ws + a.L.wt + rt * 32 + l31;                                   // Wq[hd][c = rt*32 + l31]
    const float* ak = aq + HID * C;
    const float* au = a.ws + a.L.u + slot * (HID * C) + rt * 32 + l31;                 // U[hd][c]

    f32x16 dwq[NCT], dwk[NCT];                      // tile t: rows c = t*32 + crow, columns d = l31 (this wave's head)
#pragma unroll
    for (int t = 0; t < NCT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) { dwq[t][r] = 0.f; dwk[t][r] = 0.f; }
    float dgacc[CG];
#pragma unroll
    for (int k = 0; k < CG; ++k) dgacc[k] = 0.f;
    const int pre = POST ? a.pre_mode : 0;
    __syncthreads();                                // st

    const int t0 = split * a.tiles_per_split;
    const int t1 = min(t0 + a.tiles_per_split, a.ntiles);
    for (int tile = t0; tile < t1; ++tile) {
        float xv[CG], gy[CG];
        fetch_tile<C>(xseq + (int64_t)tile * TT, a.sc, tid, xv);
        fetch_tile<C>((POST ? dxseq : dyseq) + (int64_t)tile * TT, a.sc, tid, gy);
#pragma unroll
        for (int k = 0; k < CG; ++k) dys[(grp * CG + k) * XP + tok] = gy[k];
        if constexpr (POST) fetch_tile<C>(dyseq + (int64_t)tile * TT, a.sc, tid, gy);      // the residual's dy, under the products
        float live;
        const float rstd = ln_tile<C>(xv, a.g, pre, a.eps, xs, red, tid, live);            // xv = xh from here on
        {   // s, dq~ = T_h^T dy, dQ = s (scale dq~ - sum_d s scale dq~)
            f32x16 q[2], dq[2];
            project<C>(wq, xs, l31, lh, q);
#pragma unroll
            for (int r = 0; r < 16; ++r) { dq[0][r] = 0.f; dq[1][r] = 0.f; }
#pragma unroll 8
            for (int ks = 0; ks < C / 2; ++ks) {
                const int k = 2 * ks + lh;
                const float ta = tq[k * 32];
                dq[0] = MFMA(ta, dys[k * XP + l31], dq[0]);
                dq[1] = MFMA(ta, dys[k * XP + 32 + l31], dq[1]);
            }
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                softmax_d(q[j]);
                float dot = 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) { dq[j][r] *= SCALE; dot += q[j][r] * dq[j][r]; }
                dot += __shfl_xor(dot, 32, 64);
#pragma unroll
                for (int r = 0; r < 16; ++r) gq[(head * 32 + crow(r, lh)) * XP + j * 32 + l31] = q[j][r] * (dq[j][r] - dot);
            }
        }
        f32x16 p[2];
        {   // p = exp(K - kmax) / ksum, dp = U_h xn, dK = p (dp - delta)
            f32x16 dp[2];
            project<C>(wk, xs, l31, lh, p);
#pragma unroll
            for (int r = 0; r < 16; ++r) { dp[0][r] = 0.f; dp[1][r] = 0.f; }
#pragma unroll 8
            for (int ks = 0; ks < C / 2; ++ks) {
                const int k = 2 * ks + lh;
                const float ua = ut[k * 32];
                dp[0] = MFMA(ua, xs[k * XP + l31], dp[0]);
                dp[1] = MFMA(ua, xs[k * XP + 32 + l31], dp[1]);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int d = head * 32 + crow(r, lh);
                const float nml = st[d], rk = st[HID + d], dl = st[2 * HID + d];
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const float pv = __builtin_amdgcn_exp2f(fmaf(p[j][r], LOG2E, nml)) * rk;
                    p[j][r] = pv;
                    gk[d * XP + j * 32 + l31] = pv * (dp[j][r] - dl);
                }
            }
        }
        __syncthreads();                            // every wave is done with the dy image (p goes over it at width 128)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) pp[(head * 32 + crow(r, lh)) * XP + j * 32 + l31] = p[j][r];
        __syncthreads();
        // dxn[c][tok] = sum_hd Wq[hd][c] dQ[hd][tok] + Wk[hd][c] dK[hd][tok] + U[hd][c] p[hd][tok]
        f32x16 dxa[TPW];
#pragma unroll
        for (int u = 0; u < TPW; ++u)
#pragma unroll
            for (int r = 0; r < 16; ++r) dxa[u][r] = 0.f;
#pragma unroll 4
        for (int ks = 0; ks < HID / 2; ++ks) {
            const int k = 2 * ks + lh;
            const float a0 = aq[k * C], a1 = ak[k * C], a2 = au[k * C];
#pragma unroll
            for (int u = 0; u < TPW; ++u) {
                const int col = (ct0 + u) * 32 + l31;
                dxa[u] = MFMA(a0, gq[k * XP + col], dxa[u]);
                dxa[u] = MFMA(a1, gk[k * XP + col], dxa[u]);
                dxa[u] = MFMA(a2, pp[k * XP + col], dxa[u]);
            }
        }
        // dWq^T[c][h, d] += sum_tok xn[c][tok] dQ[h, d][tok], dWk likewise
#pragma unroll 4
        for (int s = 0; s < TT / 2; ++s) {
            const int tk = 2 * s + lh;
            const float bq = gq[(head * 32 + l31) * XP + tk], bk = gk[(head * 32 + l31) * XP + tk];
#pragma unroll
            for (int t = 0; t < NCT; ++t) {
                const float xa = xs[(t * 32 + l31) * XP + tk];
                dwq[t] = MFMA(xa, bq, dwq[t]);
                dwk[t] = MFMA(xa, bk, dwk[t]);
            }
        }
        __syncthreads();                            // every wave is done with dQ: dxn goes over it
#pragma unroll
        for (int u = 0; u < TPW; ++u)
#pragma unroll
            for (int r = 0; r < 16; ++r) gq[(rt * 32 + crow(r, lh)) * XP + (ct0 + u) * 32 + l31] = dxa[u][r];
        __syncthreads();
        // LayerNorm backward + the residual: dx = dy + rstd (g dxn - mean_c(g dxn) - xh mean_c(g dxn xh)); dgamma += dxn xh
        // (RMSNorm, pre_mode 1: no mean term, and no xh term where the norm's clamp holds)
        float gd[CG];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int k = 0; k < CG; ++k) {
            const float dn = gq[(grp * CG + k) * XP + tok];
            gd[k] = dn * a.g[grp * CG + k];
            dgacc[k] += dn * xv[k];
            s1 += gd[k];
            s2 += gd[k] * xv[k];
        }
        red[grp * TT + tok] = s1;
        red[(4 + grp) * TT + tok] = s2;
        __syncthreads();
        float m1 = ((red[tok] + red[TT + tok]) + (red[2 * TT + tok] + red[3 * TT + tok])) * (1.0f / C);
        float m2 = ((red[4 * TT + tok] + red[5 * TT + tok]) + (red[6 * TT + tok] + red[7 * TT + tok])) * (1.0f / C);
        if (pre != 0) { m1 = 0.f; m2 *= live; }
        {
            la_gptr dp_ = la_uni(dxseq + (int64_t)tile * TT + (int64_t)(__builtin_amdgcn_readfirstlane(grp) * CG) * a.sc);
            uint32_t off = (uint32_t)tok * 4u;
#pragma unroll
            for (int k = 0; k < CG; ++k) {
                asm volatile("" : "+v"(off));
                la_st(dp_, off, gy[k] + rstd * (gd[k] - m1 - xv[k] * m2));
                dp_ += a.sc;
                asm volatile("" : "+s"(dp_));
            }
        }
        __syncthreads();                            // every image is rewritten by the next tile
    }
    // this block's partial table: every element written, whatever the split gave it
    float* tab = a.ws + a.L.tabqk + (slot * a.ns0 + split) * (C * 257);
#pragma unroll
    for (int t = 0; t < NCT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            tab[(t * 32 + crow(r, lh)) * 256 + head * 32 + l31] = dwq[t][r];
            tab[(t * 32 + crow(r, lh)) * 256 + HID + head * 32 + l31] = dwk[t][r];
        }
#pragma unroll
    for (int k = 0; k < CG; ++k) xs[(grp * CG + k) * XP + tok] = dgacc[k];
    __syncthreads();
    if (tid < C) {
        float s = 0.f;
        for (int t = 0; t < TT; ++t) s += xs[tid * XP + t];
        tab[C * 256 + tid] = s;
    }
}

// ------------------------------------------------------------------ the partial tables of a chunk, in a fixed order
// 64 output elements x SR_G groups per block (the scheme of tab_sum_kernel, sdc_tablock_bwd.hip): group g adds the tables k = g (mod
// SR_G) in rising order, group 0 then adds the SR_G sums in order.  Tables per element: (slot, split) for dWq | dWk, dgamma and dbo,
// slot for dWv and dWo.  The post-norm form adds C elements (dg_post, tables per (slot, split)) and C / 64 blocks.
constexpr int SR_G = 16;
__global__ __launch_bounds__(64 * SR_G) void lab_sum_kernel(const float* __restrict__ ws, const LabWs L, int C, int ns0, int nsplit,
                                                           int nslot, int accum, float* __restrict__ dwqkv, float* __restrict__ dwo,
                                                           float* __restrict__ dg, float* __restrict__ dbo, float* __restrict__ dgp) {
    __shared__ float sh[SR_G][64];
    const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int e = blockIdx.x * 64 + lane;           // the outputs are a multiple of 64 (514 C)
    const int n0 = C * 3 * HID, n1 = n0 + HID * C, n2 = n1 + C, n3 = n2 + C;
    const float* base;                              // element of table (slot 0, split 0)
    int64_t slot_stride, split_stride = 0;
    float* out;
    if (e < n0) {
        const int c = e / (3 * HID), j = e - c * (3 * HID);
        out = dwqkv + e;
        if (j < 2 * HID) { base = ws + L.tabqk + c * 256 + j; split_stride = C * 257; slot_stride = (int64_t)ns0 * split_stride; }
        else { base = ws + L.tabv + c * HID + (j - 2 * HID); slot_stride = C * HID; }
    } else if (e < n1) {
        out = dwo + (e - n0); base = ws + L.tabo + (e - n0); slot_stride = HID * C;
    } else if (e < n2) {
        out = dg + (e - n1); base = ws + L.tabqk + C * 256 + (e - n1); split_stride = C * 257; slot_stride = (int64_t)ns0 * split_stride;
    } else if (e < n3) {
        out = dbo ? dbo + (e - n2) : nullptr; base = ws + L.dbop + (e - n2); split_stride = C; slot_stride = (int64_t)ns0 * C;
    } else {
        out = dgp + (e - n3); base = ws + L.dgpp + (e - n3); split_stride = C; slot_stride = (int64_t)ns0 * C;
    }
    const int per = split_stride ? nsplit : 1, K = nslot * per;
    float s = 0.f;
    if (out)
        for (int k = g; k < K; k += SR_G) {
            const int sl = k / per, sp = k - sl * per;
            s += base[sl * slot_stride + sp * split_stride];
        }
    sh[g][lane] = s;
    __syncthreads();
    if (g == 0 && out) {
        float t = sh[0][lane];
        for (int q = 1; q < SR_G; ++q) t += sh[q][lane];
        *out = accum ? *out + t : t;
    }
}

template <int C, bool POST>
int lab_chunk(LabArgs a, LaArgs f, int cnt, int accum, float* dwqkv, float* dwo, float* dg, float* dbo, float* dgp, const char* what,
              hipStream_t s) {
    constexpr size_t lds1 = sizeof(float) * (size_t)(2 * C * XP + HID * XP + (POST ? 12 : 8) * TT);
    constexpr size_t lds2 = sizeof(float) * (size_t)(2 * C * XP + (C == 128 ? 2 : 3) * HID * XP + 8 * TT + 3 * HID);
    static_assert(lds1 <= 160 * 1024 && lds2 <= 160 * 1024, "LDS budget");
    static std::atomic<uint64_t> attr1{0}, attr2{0};
    SDC_LDS_OPTIN(attr1, (lab_dt_kernel<C, POST>), 160 * 1024, what);
    SDC_LDS_OPTIN(attr2, (lab_dx_kernel<C, POST>), 160 * 1024, what);
    const dim3 gs((unsigned)a.nsplit, (unsigned)cnt), gm(4, (unsigned)cnt);
    if (const int rc = sdc::la_launch_ctx(f, C, gs, s)) return rc;
    hipLaunchKernelGGL(lab_mid1_kernel<C>, gm, dim3(NT), 0, s, a);
    hipLaunchKernelGGL((lab_dt_kernel<C, POST>), gs, dim3(NT), lds1, s, a);
    hipLaunchKernelGGL(lab_mid2_kernel<C>, gm, dim3(NT), 0, s, a);
    hipLaunchKernelGGL((lab_dx_kernel<C, POST>), gs, dim3(NT), lds2, s, a);
    constexpr int NOUT = C * 3 * HID + HID * C + (POST ? 3 : 2) * C;
    static_assert(NOUT % 64 == 0, "lab_sum_kernel walks whole groups of 64");
    hipLaunchKernelGGL(lab_sum_kernel, dim3(NOUT / 64), dim3(64 * SR_G), 0, s, (const float*)a.ws, a.L, C, a.ns0, a.nsplit, cnt, accum,
                       dwqkv, dwo, dg, dbo, dgp);
    return SDC_OK;
}

// the launches of both entries (arguments checked by the caller): g_post / dg_post null and post_mode -1 for the form without a post norm
int lab_backward(const char* what, const float* x, const float* g_pre, const float* wqkv, const float* wo, const float* bo,
                 const float* g_post, const float* dy, float* dx, float* dg, float* dwqkv, float* dwo, float* dbo, float* dg_post,
                 void* work, int outer, int inner, int C, int64_t n, int64_t so, int64_t sc, int64_t si, int pre_mode, int post_mode,
                 float eps, void* stream) {
    const bool post = post_mode >= 0;
    const int64_t nseq = (int64_t)outer * inner;
    LabArgs a;
    a.x = x; a.dy = dy; a.g = g_pre; a.wqkv = wqkv; a.wo = wo; a.dx = dx; a.ws = static_cast<float*>(work);
    a.bo = bo; a.gp = g_post; a.pre_mode = pre_mode; a.post_mode = post_mode;
    a.ntiles = (int)(n / TT);
    a.ns0 = pick_nsplit(nseq, a.ntiles);
    a.tiles_per_split = (a.ntiles + a.ns0 - 1) / a.ns0;
    a.nsplit = (a.ntiles + a.tiles_per_split - 1) / a.tiles_per_split;      // no empty splits (as the forward)
    const int SG = lab_slots(a.ns0);
    a.L = lab_layout(C, a.ns0, (int)(nseq < SG ? nseq : SG), post);
    a.inner = inner; a.eps = eps; a.so = so; a.sc = sc; a.si = si;
    LaArgs f{};
    f.g_pre = g_pre; f.wqkv = wqkv; f.wo = wo; f.part = a.ws + a.L.part;
    f.nsplit = a.nsplit; f.tiles_per_split = a.tiles_per_split; f.ntiles = a.ntiles; f.tiles_per_blk = 1;
    f.pre_mode = pre_mode; f.post_mode = -1; f.eps = eps; f.so = so; f.sc = sc; f.si = si;
    hipStream_t s = sdc::as_stream(stream);
    hipLaunchKernelGGL(lab_wt_kernel, dim3(C), dim3(NT), 0, s, wqkv, a.ws + a.L.wt, C);
    // chunks of at most SG sequences: whole outer indices while they fit, else runs of one outer index's sequences
    int accum = 0;
    auto chunk = [&](int64_t off, int cinner, int cnt) -> int {
        a.x = x + off; a.dy = dy + off; a.dx = dx + off; a.inner = cinner;
        f.x = a.x; f.inner = cinner;
        float* db = bo ? dbo : nullptr;
        const int rc = post ? (C == 64 ? lab_chunk<64, true>(a, f, cnt, accum, dwqkv, dwo, dg, db, dg_post, what, s)
                                       : lab_chunk<128, true>(a, f, cnt, accum, dwqkv, dwo, dg, db, dg_post, what, s))
                            : (C == 64 ? lab_chunk<64, false>(a, f, cnt, accum, dwqkv, dwo, dg, db, nullptr, what, s)
                                       : lab_chunk<128, false>(a, f, cnt, accum, dwqkv, dwo, dg, db, nullptr, what, s));
        accum = 1;
        return rc;
    };
    if (inner <= SG) {
        const int per = SG / inner;
        for (int o0 = 0; o0 < outer; o0 += per) {
            const int no = outer - o0 < per ? outer - o0 : per;
            if (const int rc = chunk((int64_t)o0 * so, inner, no * inner)) return rc;
        }
    } else {
        for (int o = 0; o < outer; ++o)
            for (int i0 = 0; i0 < inner; i0 += SG) {
                const int cnt = inner - i0 < SG ? inner - i0 : SG;
                if (const int rc = chunk((int64_t)o * so + (int64_t)i0 * si, cnt, cnt)) return rc;
            }
    }
    return sdc::check_launch(what);
}

size_t lab_bytes(int outer, int inner, int C, int64_t n, bool post) {
    if (outer <= 0 || inner <= 0 || n <= 0 || n % TT != 0 || (C != 64 && C != 128)) return 0;
    const int64_t nseq = (int64_t)outer * inner;
    const int ns = pick_nsplit(nseq, (int)(n / TT));
    const int SG = lab_slots(ns);
    return sizeof(float) * (size_t)lab_layout(C, ns, (int)(nseq < SG ? nseq : SG), post).total;
}

}  // namespace

extern "C" size_t sdc_linattn_block_bwd_bytes(int outer, int inner, int C, int64_t n) { return lab_bytes(outer, inner, C, n, false); }

extern "C" int sdc_linattn_block_bwd(const float* x, const float* g_pre, const float* wqkv, const float* wo, const float* bo,
                                     const float* dy, float* dx, float* dg, float* dwqkv, float* dwo, float* dbo, void* work,
                                     int outer, int inner, int C, int64_t n, int64_t so, int64_t sc, int64_t si, int pre_mode,
                                     int post_mode, float eps, void* stream) {
    SDC_REQUIRE(x, SDC_ENULL, "sdc_linattn_block_bwd: null x");
    SDC_REQUIRE(g_pre, SDC_ENULL, "sdc_linattn_block_bwd: null g_pre");
    SDC_REQUIRE(wqkv, SDC_ENULL, "sdc_linattn_block_bwd: null wqkv");
    SDC_REQUIRE(wo, SDC_ENULL, "sdc_linattn_block_bwd: null wo");
    SDC_REQUIRE(dy, SDC_ENULL, "sdc_linattn_block_bwd: null dy");
    SDC_REQUIRE(dx, SDC_ENULL, "sdc_linattn_block_bwd: null dx");
    SDC_REQUIRE(dg, SDC_ENULL, "sdc_linattn_block_bwd: null dg");
    SDC_REQUIRE(dwqkv, SDC_ENULL, "sdc_linattn_block_bwd: null dwqkv");
    SDC_REQUIRE(dwo, SDC_ENULL, "sdc_linattn_block_bwd: null dwo");
    SDC_REQUIRE(work, SDC_ENULL, "sdc_linattn_block_bwd: null work");
    SDC_REQUIRE(!bo || dbo, SDC_ENULL, "sdc_linattn_block_bwd: null dbo although bo is given");
    SDC_REQUIRE(pre_mode == 0, SDC_EINVAL, "sdc_linattn_block_bwd: pre norm mode %d is not supported (0, channel LayerNorm, only)", pre_mode);
    SDC_REQUIRE(post_mode == -1, SDC_EINVAL, "sdc_linattn_block_bwd: post norm mode %d is not supported (-1, no post norm, only)", post_mode);
    SDC_REQUIRE(C == 64 || C == 128, SDC_EINVAL, "sdc_linattn_block_bwd: dim must be 64 or 128 (got %d)", C);
    SDC_REQUIRE(outer > 0 && inner > 0 && n > 0 && n % TT == 0, SDC_EINVAL, "sdc_linattn_block_bwd: tokens must be a multiple of 64");
    SDC_REQUIRE(n / TT < (1ll << 24), SDC_EINVAL, "sdc_linattn_block_bwd: too many tokens");
    SDC_REQUIRE((int64_t)outer * inner < 65536, SDC_EINVAL, "sdc_linattn_block_bwd: outer*inner must be < 65536");
    SDC_REQUIRE(sc > 0 && sc < (1ll << 27), SDC_EINVAL,
                "sdc_linattn_block_bwd: channel stride must stay below 2^27 elements (32-bit lane offsets)");
    SDC_REQUIRE(reinterpret_cast<uintptr_t>(wqkv) % 16 == 0 && reinterpret_cast<uintptr_t>(wo) % 16 == 0, SDC_EINVAL,
                "sdc_linattn_block_bwd: wqkv / wo must be 16-byte aligned");
    SDC_REQUIRE(dx != x && dx != dy, SDC_EINVAL, "sdc_linattn_block_bwd: dx must not alias x or dy");
    return lab_backward("sdc_linattn_block_bwd", x, g_pre, wqkv, wo, bo, nullptr, dy, dx, dg, dwqkv, dwo, dbo, nullptr, work, outer,
                        inner, C, n, so, sc, si, 0, -1, eps, stream);
}

extern "C" size_t sdc_linattn_block_post_bwd_bytes(int outer, int inner, int C, int64_t n) { return lab_bytes(outer, inner, C, n, true); }

extern "C" int sdc_linattn_block_post_bwd(const float* x, const float* g_pre, const float* wqkv, const float* wo, const float* bo,
                                          const float* g_post, const float* dy, float* dx, float* dg_pre, float* dwqkv, float* dwo,
                                          float* dbo, float* dg_post, void* work, int outer, int inner, int C, int64_t n, int64_t so,
                                          int64_t sc, int64_t si, int pre_mode, int post_mode, float eps, void* stream) {
    SDC_REQUIRE(x, SDC_ENULL, "sdc_linattn_block_post_bwd: null x");
    SDC_REQUIRE(g_pre, SDC_ENULL, "sdc_linattn_block_post_bwd: null g_pre");
    SDC_REQUIRE(wqkv, SDC_ENULL, "sdc_linattn_block_post_bwd: null wqkv");
    SDC_REQUIRE(wo, SDC_ENULL, "sdc_linattn_block_post_bwd: null wo");
    SDC_REQUIRE(g_post, SDC_ENULL, "sdc_linattn_block_post_bwd: null g_post");
    SDC_REQUIRE(dy, SDC_ENULL, "sdc_linattn_block_post_bwd: null dy");
    SDC_REQUIRE(dx, SDC_ENULL, "sdc_linattn_block_post_bwd: null dx");
    SDC_REQUIRE(dg_pre, SDC_ENULL, "sdc_linattn_block_post_bwd: null dg_pre");
    SDC_REQUIRE(dwqkv, SDC_ENULL, "sdc_linattn_block_post_bwd: null dwqkv");
    SDC_REQUIRE(dwo, SDC_ENULL, "sdc_linattn_block_post_bwd: null dwo");
    SDC_REQUIRE(dg_post, SDC_ENULL, "sdc_linattn_block_post_bwd: null dg_post");
    SDC_REQUIRE(work, SDC_ENULL, "sdc_linattn_block_post_bwd: null work");
    SDC_REQUIRE(!bo || dbo, SDC_ENULL, "sdc_linattn_block_post_bwd: null dbo although bo is given");
    SDC_REQUIRE(pre_mode == 0 || pre_mode == 1, SDC_EINVAL,
                "sdc_linattn_block_post_bwd: pre norm mode %d is not supported (0 channel LayerNorm, 1 RMSNorm)", pre_mode);
    SDC_REQUIRE(post_mode != -1, SDC_EINVAL,
                "sdc_linattn_block_post_bwd: post norm mode -1 (no post norm) is sdc_linattn_block_bwd's form");
    SDC_REQUIRE(post_mode == 0 || post_mode == 1, SDC_EINVAL,
                "sdc_linattn_block_post_bwd: post norm mode %d is not supported (0 channel LayerNorm, 1 RMSNorm)", post_mode);
    SDC_REQUIRE(C == 64 || C == 128, SDC_EINVAL, "sdc_linattn_block_post_bwd: dim must be 64 or 128 (got %d)", C);
    SDC_REQUIRE(outer > 0 && inner > 0 && n > 0 && n % TT == 0, SDC_EINVAL, "sdc_linattn_block_post_bwd: tokens must be a multiple of 64");
    SDC_REQUIRE(n / TT < (1ll << 24), SDC_EINVAL, "sdc_linattn_block_post_bwd: too many tokens");
    SDC_REQUIRE((int64_t)outer * inner < 65536, SDC_EINVAL, "sdc_linattn_block_post_bwd: outer*inner must be < 65536");
    SDC_REQUIRE(sc > 0 && sc < (1ll << 27), SDC_EINVAL,
                "sdc_linattn_block_post_bwd: channel stride must stay below 2^27 elements (32-bit lane offsets)");
    SDC_REQUIRE(reinterpret_cast<uintptr_t>(wqkv) % 16 == 0, SDC_EINVAL, "sdc_linattn_block_post_bwd: wqkv must be 16-byte aligned");
    SDC_REQUIRE(reinterpret_cast<uintptr_t>(wo) % 16 == 0, SDC_EINVAL, "sdc_linattn_block_post_bwd: wo must be 16-byte aligned");
    SDC_REQUIRE(dx != x, SDC_EINVAL, "sdc_linattn_block_post_bwd: dx must not alias x");
    SDC_REQUIRE(dx != dy, SDC_EINVAL, "sdc_linattn_block_post_bwd: dx must not alias dy");
    return lab_backward("sdc_linattn_block_post_bwd", x, g_pre, wqkv, wo, bo, g_post, dy, dx, dg_pre, dwqkv, dwo, dbo, dg_post, work,
                        outer, inner, C, n, so, sc, si, pre_mode, post_mode, eps, stream);
}
