// Streaming softmax attention past 256 tokens (heads x dim_head 32, fp32, no rotary / bias, tokens contiguous): the mid
// spatial attention of the smoke net above 64 x 64 ((S/4)^2 tokens, conv3d.py:450-452,548) and the 1-D nets' mid Attention
// on grids wider than 1024 cells (1D/model/unet.py:224-258).  attn256_kernel (sdc_attn.hip) keeps all scores of a query in
// registers; here the keys stream through LDS in blocks of 64 and the softmax runs online.
//
// Forward: a workgroup (4 waves) owns 128 queries of one (outer, inner, head) sequence, wave w the 32 queries 32w ... 32w+31.
// Per key block, S^T[key][query] = K . Q^T (2 x 16 v_mfma_f32_32x32x2_f32: the 64 scores of a query sit in the registers of
// lanes l and l + 32), the running maximum m, the running sum l and the rescale of the output accumulator are per-lane
// scalars in fp32, and the P registers are the B operands of O^T[d][query] += V . P as they stand (32 MFMAs).  K and V sit
// in LDS as [d][65]: the S product reads a row (lanes = keys), the O product a column (lanes = d): the odd pitch keeps both
// conflict-free.  The next block's K and V are requested into registers before the products of the current one start.
// The ragged last block is masked on the key side (p = 0) and on the query side (no load, no store).
//
// Backward (three launches, no atomics, nothing ntok x ntok in memory):
//   1. the forward again, writing per row  lse_i = m_i + log l_i  and  D_i = dO_i . O_i  instead of O   (2 floats per row)
//   2. dq: workgroup = 128 queries, K / V stream; P = exp(S - lse), dP^T = V^T . dO^T, dS = P (dP - D), dq^T += K^T . dS
//   3. dk, dv: workgroup = 128 keys, Q / dO / lse / D stream; S[query][key] = Q . K^T, dv^T += dO^T . P, dk^T += Q^T . dS
// Every output element has one owner and every sum runs in block order, so two runs give the same bits, and nothing depends
// on outer or inner (the samplers' rule: a sample's bits do not depend on the batch it rides in).
#include "sdc_common.h"
#include "sdc_attn_long.h"

namespace {

constexpr int NT = 256;
constexpr int DH = 32;
constexpr int KB = 64;                   // tokens per streamed block
constexpr int QB = 128;                  // tokens a workgroup owns (32 per wave)
constexpr int LP = 65;                   // LDS pitch of a [d][64 tokens] image
constexpr float SCALE = 0.17677669529663687f;       // dim_head^-0.5
typedef float f32x16 __attribute__((ext_vector_type(16)));

struct LongArgs {
    const float* qkv; const float* dout; float* out; float* dqkv; float* stats;
    int inner, heads, ntok, nqb;
    int64_t so, sc, si, oso, osc, osi;
};

// row (r & 3) + 8 (r >> 2) + 4 (lane >> 5) of a 32 x 32 accumulator tile sits in register r
__device__ __forceinline__ int acc_row(int r) { return (r & 3) + 8 * (r >> 2); }

// a [32 d][64 tokens] block of a channel-major tensor: thread -> rows wave + 4 it, column lane (256-byte runs); tokens past
// the end read as zero
__device__ __forceinline__ void blk_load(float (&reg)[8], const float* base, int64_t sc, int j0, int ntok, int wave, int lane) {
    const int j = j0 + lane;
#pragma unroll
    for (int it = 0; it < 8; ++it) reg[it] = j < ntok ? base[(int64_t)(wave + 4 * it) * sc + j] : 0.0f;
}
__device__ __forceinline__ void blk_store(float* img, const float (&reg)[8], int wave, int lane, float mul) {
#pragma unroll
    for (int it = 0; it < 8; ++it) img[(wave + 4 * it) * LP + lane] = reg[it] * mul;
}

// ------------------------------------------------------------------------------------------------ forward / row statistics
// STATS = false: out;  STATS = true: lse and D = dO . O of every row into a.stats ([sequence, head][2][ntok])
template <bool STATS>
__global__ __launch_bounds__(NT) void attn_long_fwd_kernel(const LongArgs a) {
    __shared__ float Ks[DH * LP], Vs[DH * LP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lh = lane >> 5;
    const int qblk = blockIdx.x % a.nqb, sh = blockIdx.x / a.nqb;
    const int head = sh % a.heads, sq = sh / a.heads;
    const int o = sq / a.inner, i = sq - o * a.inner;
    const int ntok = a.ntok;
    const float* qb = a.qkv + o * a.so + i * a.si + (int64_t)(head * DH) * a.sc;
    const float* kb = qb + (int64_t)(a.heads * DH) * a.sc;
    const float* vb = kb + (int64_t)(a.heads * DH) * a.sc;
    const int q0 = qblk * QB + wave * 32, qi = q0 + l31;
    const bool qok = qi < ntok;
    // B fragments of Q^T: B[d = 2s + lh][query = l31]
    float qf[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) qf[s] = qok ? qb[(int64_t)(2 * s + lh) * a.sc + qi] * SCALE : 0.0f;

    float kreg[8], vreg[8];
    blk_load(kreg, kb, a.sc, 0, ntok, wave, lane);
    blk_load(vreg, vb, a.sc, 0, ntok, wave, lane);
    float m = -INFINITY, lsum = 0.0f;            // running maximum (both halves agree) and this half's running sum
    f32x16 oacc;
#pragma unroll
    for (int r = 0; r < 16; ++r) oacc[r] = 0.0f;
    const int nkb = (ntok + KB - 1) / KB;
    for (int b = 0; b < nkb; ++b) {
        const int j0 = b * KB;
        __syncthreads();                         // every wave is done with the previous block
        blk_store(Ks, kreg, wave, lane, 1.0f);
        blk_store(Vs, vreg, wave, lane, 1.0f);
        __syncthreads();
        if (b + 1 < nkb) {                       // the next block travels under this block's products
            blk_load(kreg, kb, a.sc, j0 + KB, ntok, wave, lane);
            blk_load(vreg, vb, a.sc, j0 + KB, ntok, wave, lane);
        }
        if (q0 >= ntok) continue;                // (wave-uniform: a wave past the last query only stages)
        f32x16 p[2];
#pragma unroll
        for (int r = 0; r < 16; ++r) { p[0][r] = 0.0f; p[1][r] = 0.0f; }
#pragma unroll
        for (int s = 0; s < 16; ++s) {           // A[key = l31][d = 2s + lh]
            p[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(Ks[(2 * s + lh) * LP + l31], qf[s], p[0], 0, 0, 0);
            p[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(Ks[(2 * s + lh) * LP + 32 + l31], qf[s], p[1], 0, 0, 0);
        }
        // lane (query = l31, half lh) holds keys j0 + 32 u + acc_row(r) + 4 lh
        if (j0 + KB > ntok) {
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (j0 + 32 * u + acc_row(r) + 4 * lh >= ntok) p[u][r] = -INFINITY;
        }
        float bm = -INFINITY;
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int r = 0; r < 16; ++r) bm = fmaxf(bm, p[u][r]);
        bm = fmaxf(bm, __shfl_xor(bm, 32, 64));
        const float mn = fmaxf(m, bm);           // finite: every block holds at least one key
        const float alpha = sdc::softmax_exp(m - mn);     // 0 at the first block (m = -inf)
        float bs = 0.0f;
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int r = 0; r < 16; ++r) { p[u][r] = sdc::softmax_exp(p[u][r] - mn); bs += p[u][r]; }      // masked keys: exp(-inf) = 0
        lsum = lsum * alpha + bs;
        m = mn;
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[r] *= alpha;
        // O^T[d][query] += sum_key V[d][key] P[key][query]: A[d = l31][key], B = P registers (k-step r of half-block u)
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                oacc = __builtin_amdgcn_mfma_f32_32x32x2f32(Vs[l31 * LP + 32 * u + acc_row(r) + 4 * lh], p[u][r], oacc, 0, 0, 0);
    }
    if (q0 >= ntok) return;
    const float l = lsum + __shfl_xor(lsum, 32, 64);
    const float inv = 1.0f / l;
    // lane (query = l31, half lh) holds d = acc_row(r) + 4 lh: 128-byte runs along the tokens
    if (!STATS) {
        float* ob = a.out + o * a.oso + i * a.osi + (int64_t)(head * DH) * a.osc;
        if (qok) {
#pragma unroll
            for (int r = 0; r < 16; ++r) ob[(int64_t)(acc_row(r) + 4 * lh) * a.osc + qi] = oacc[r] * inv;
        }
    } else {
        const float* gb = a.dout + o * a.oso + i * a.osi + (int64_t)(head * DH) * a.osc;
        float dd = 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) dd += (qok ? gb[(int64_t)(acc_row(r) + 4 * lh) * a.osc + qi] : 0.0f) * (oacc[r] * inv);
        dd += __shfl_xor(dd, 32, 64);
        if (qok && lh == 0) {
            float* st = a.stats + (int64_t)sh * 2 * ntok;
            st[qi] = m + logf(l);
            st[ntok + qi] = dd;
        }
    }
}

// ------------------------------------------------------------------------------------------------ dq
__global__ __launch_bounds__(NT) void attn_long_dq_kernel(const LongArgs a) {
    __shared__ float Ks[DH * LP], Vs[DH * LP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lh = lane >> 5;
    const int qblk = blockIdx.x % a.nqb, sh = blockIdx.x / a.nqb;
    const int head = sh % a.heads, sq = sh / a.heads;
    const int o = sq / a.inner, i = sq - o * a.inner;
    const int ntok = a.ntok;
    const float* qb = a.qkv + o * a.so + i * a.si + (int64_t)(head * DH) * a.sc;
    const float* kb = qb + (int64_t)(a.heads * DH) * a.sc;
    const float* vb = kb + (int64_t)(a.heads * DH) * a.sc;
    const float* gb = a.dout + o * a.oso + i * a.osi + (int64_t)(head * DH) * a.osc;
    const int q0 = qblk * QB + wave * 32, qi = q0 + l31;
    const bool qok = qi < ntok;
    // B fragments of Q^T and dO^T: B[d = 2s + lh][query = l31]
    float qf[16], gf[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) {
        qf[s] = qok ? qb[(int64_t)(2 * s + lh) * a.sc + qi] * SCALE : 0.0f;
        gf[s] = qok ? gb[(int64_t)(2 * s + lh) * a.osc + qi] : 0.0f;
    }
    const float* st = a.stats + (int64_t)sh * 2 * ntok;
    const float lse = qok ? st[qi] : 0.0f, dd = qok ? st[ntok + qi] : 0.0f;

    float kreg[8], vreg[8];
    blk_load(kreg, kb, a.sc, 0, ntok, wave, lane);
    blk_load(vreg, vb, a.sc, 0, ntok, wave, lane);
    f32x16 dq;
#pragma unroll
    for (int r = 0; r < 16; ++r) dq[r] = 0.0f;
    const int nkb = (ntok + KB - 1) / KB;
    for (int b = 0; b < nkb; ++b) {
        const int j0 = b * KB;
        __syncthreads();
        blk_store(Ks, kreg, wave, lane, 1.0f);
        blk_store(Vs, vreg, wave, lane, 1.0f);
        __syncthreads();
        if (b + 1 < nkb) {
            blk_load(kreg, kb, a.sc, j0 + KB, ntok, wave, lane);
            blk_load(vreg, vb, a.sc, j0 + KB, ntok, wave, lane);
        }
        if (q0 >= ntok) continue;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            f32x16 sv, dp;
#pragma unroll
            for (int r = 0; r < 16; ++r) { sv[r] = 0.0f; dp[r] = 0.0f; }
#pragma unroll
            for (int s = 0; s < 16; ++s) {       // S^T = K . Q^T and dP^T = V^T . dO^T: A[key = l31][d = 2s + lh]
                sv = __builtin_amdgcn_mfma_f32_32x32x2f32(Ks[(2 * s + lh) * LP + 32 * u + l31], qf[s], sv, 0, 0, 0);
                dp = __builtin_amdgcn_mfma_f32_32x32x2f32(Vs[(2 * s + lh) * LP + 32 * u + l31], gf[s], dp, 0, 0, 0);
            }
            // lane (query = l31, half lh) holds keys j0 + 32 u + acc_row(r) + 4 lh
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float pr = j0 + 32 * u + acc_row(r) + 4 * lh < ntok ? sdc::softmax_exp(sv[r] - lse) : 0.0f;
                sv[r] = pr * (dp[r] - dd);
            }
            // dq^T[d][query] += sum_key K[d][key] dS[key][query]: A[d = l31][key], B = dS registers
#pragma unroll
            for (int r = 0; r < 16; ++r)
                dq = __builtin_amdgcn_mfma_f32_32x32x2f32(Ks[l31 * LP + 32 * u + acc_row(r) + 4 * lh], sv[r], dq, 0, 0, 0);
        }
    }
    if (!qok) return;
    float* dqb = a.dqkv + o * a.so + i * a.si + (int64_t)(head * DH) * a.sc;
#pragma unroll
    for (int r = 0; r < 16; ++r) dqb[(int64_t)(acc_row(r) + 4 * lh) * a.sc + qi] = dq[r] * SCALE;
}

// ------------------------------------------------------------------------------------------------ dk, dv
__global__ __launch_bounds__(NT) void attn_long_dkv_kernel(const LongArgs a) {
    __shared__ float Qs[DH * LP], Gs[DH * LP], Ls[KB], Ds[KB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lh = lane >> 5;
    const int kblk = blockIdx.x % a.nqb, sh = blockIdx.x / a.nqb;
    const int head = sh % a.heads, sq = sh / a.heads;
    const int o = sq / a.inner, i = sq - o * a.inner;
    const int ntok = a.ntok;
    const float* qb = a.qkv + o * a.so + i * a.si + (int64_t)(head * DH) * a.sc;
    const float* kb = qb + (int64_t)(a.heads * DH) * a.sc;
    const float* vb = kb + (int64_t)(a.heads * DH) * a.sc;
    const float* gb = a.dout + o * a.oso + i * a.osi + (int64_t)(head * DH) * a.osc;
    const float* st = a.stats + (int64_t)sh * 2 * ntok;
    const int k0 = kblk * QB + wave * 32, kj = k0 + l31;
    const bool kok = kj < ntok;
    // B fragments of K^T and V^T: B[d = 2s + lh][key = l31]
    float kf[16], vf[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) {
        kf[s] = kok ? kb[(int64_t)(2 * s + lh) * a.sc + kj] : 0.0f;
        vf[s] = kok ? vb[(int64_t)(2 * s + lh) * a.sc + kj] : 0.0f;
    }
    float qreg[8], greg[8], sreg = 0.0f;
    blk_load(qreg, qb, a.sc, 0, ntok, wave, lane);
    blk_load(greg, gb, a.osc, 0, ntok, wave, lane);
    if (tid < 2 * KB) { const int j = tid & (KB - 1); sreg = j < ntok ? st[(tid >> 6) * ntok + j] : 0.0f; }
    f32x16 dk, dv;
#pragma unroll
    for (int r = 0; r < 16; ++r) { dk[r] = 0.0f; dv[r] = 0.0f; }
    const int nqb = (ntok + KB - 1) / KB;
    for (int b = 0; b < nqb; ++b) {
        const int i0 = b * KB;
        __syncthreads();
        blk_store(Qs, qreg, wave, lane, SCALE);
        blk_store(Gs, greg, wave, lane, 1.0f);
        if (tid < KB) Ls[tid] = sreg; else if (tid < 2 * KB) Ds[tid - KB] = sreg;
        __syncthreads();
        if (b + 1 < nqb) {
            blk_load(qreg, qb, a.sc, i0 + KB, ntok, wave, lane);
            blk_load(greg, gb, a.osc, i0 + KB, ntok, wave, lane);
            if (tid < 2 * KB) { const int j = i0 + KB + (tid & (KB - 1)); sreg = j < ntok ? st[(tid >> 6) * ntok + j] : 0.0f; }
        }
        if (k0 >= ntok) continue;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            f32x16 sv, dp;
#pragma unroll
            for (int r = 0; r < 16; ++r) { sv[r] = 0.0f; dp[r] = 0.0f; }
#pragma unroll
            for (int s = 0; s < 16; ++s) {       // S = Q . K^T and dP = dO . V^T: A[query = l31][d = 2s + lh]
                sv = __builtin_amdgcn_mfma_f32_32x32x2f32(Qs[(2 * s + lh) * LP + 32 * u + l31], kf[s], sv, 0, 0, 0);
                dp = __builtin_amdgcn_mfma_f32_32x32x2f32(Gs[(2 * s + lh) * LP + 32 * u + l31], vf[s], dp, 0, 0, 0);
            }
            // lane (key = l31, half lh) holds queries i0 + 32 u + acc_row(r) + 4 lh
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int qq = 32 * u + acc_row(r) + 4 * lh;
                const float pr = i0 + qq < ntok ? sdc::softmax_exp(sv[r] - Ls[qq]) : 0.0f;
                sv[r] = pr;
                dp[r] = pr * (dp[r] - Ds[qq]);
            }
            // dv^T[d][key] += sum_query dO[d][query] P[query][key], dk^T[d][key] += sum_query Q[d][query] dS[query][key]
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                dv = __builtin_amdgcn_mfma_f32_32x32x2f32(Gs[l31 * LP + 32 * u + acc_row(r) + 4 * lh], sv[r], dv, 0, 0, 0);
                dk = __builtin_amdgcn_mfma_f32_32x32x2f32(Qs[l31 * LP + 32 * u + acc_row(r) + 4 * lh], dp[r], dk, 0, 0, 0);
            }
        }
    }
    if (!kok) return;
    float* dkb = a.dqkv + o * a.so + i * a.si + (int64_t)(a.heads * DH + head * DH) * a.sc;
    float* dvb = dkb + (int64_t)(a.heads * DH) * a.sc;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        dkb[(int64_t)(acc_row(r) + 4 * lh) * a.sc + kj] = dk[r];
        dvb[(int64_t)(acc_row(r) + 4 * lh) * a.sc + kj] = dv[r];
    }
}

// the 1-D grid of all three kernels: (sequence, head) x blocks of 128 tokens
int fill_args(LongArgs& a, const char* who, int outer, int inner, int heads, int ntok, unsigned* grid) {
    a.inner = inner; a.heads = heads; a.ntok = ntok; a.nqb = (ntok + QB - 1) / QB;
    const int64_t nblk = (int64_t)outer * inner * heads * a.nqb;
    SDC_REQUIRE(nblk < (1ll << 31), SDC_EINVAL, "%s: outer*inner*heads*ceil(ntok/128) = %lld does not fit the grid", who, (long long)nblk);
    *grid = (unsigned)nblk;
    return SDC_OK;
}

}  // namespace

namespace sdc {

int attn_long(const float* qkv, float* out, int outer, int inner, int heads, int ntok, int64_t q_so, int64_t q_sc, int64_t q_si,
              int64_t o_so, int64_t o_sc, int64_t o_si, void* stream) {
    LongArgs a;
    a.qkv = qkv; a.dout = nullptr; a.out = out; a.dqkv = nullptr; a.stats = nullptr;
    a.so = q_so; a.sc = q_sc; a.si = q_si; a.oso = o_so; a.osc = o_sc; a.osi = o_si;
    unsigned grid;
    const int rc = fill_args(a, "sdc_attn[long]", outer, inner, heads, ntok, &grid);
    if (rc != SDC_OK) return rc;
    hipLaunchKernelGGL(attn_long_fwd_kernel<false>, dim3(grid), dim3(NT), 0, as_stream(stream), a);
    return check_launch("sdc_attn[long]");
}

size_t attn_long_bwd_bytes(int outer, int inner, int heads, int ntok) {
    return (size_t)outer * inner * heads * ntok * 2 * sizeof(float);       // lse and dO . O of every row
}

int attn_long_bwd(const float* qkv, const float* dout, float* dqkv, void* work, int outer, int inner, int heads, int ntok,
                  int64_t q_so, int64_t q_sc, int64_t q_si, int64_t o_so, int64_t o_sc, int64_t o_si, void* stream) {
    LongArgs a;
    a.qkv = qkv; a.dout = dout; a.out = nullptr; a.dqkv = dqkv; a.stats = static_cast<float*>(work);
    a.so = q_so; a.sc = q_sc; a.si = q_si; a.oso = o_so; a.osc = o_sc; a.osi = o_si;
    unsigned grid;
    const int rc = fill_args(a, "sdc_attn_bwd[long]", outer, inner, heads, ntok, &grid);
    if (rc != SDC_OK) return rc;
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(attn_long_fwd_kernel<true>, dim3(grid), dim3(NT), 0, s, a);
    hipLaunchKernelGGL(attn_long_dq_kernel, dim3(grid), dim3(NT), 0, s, a);
    hipLaunchKernelGGL(attn_long_dkv_kernel, dim3(grid), dim3(NT), 0, s, a);
    return check_launch("sdc_attn_bwd[long]");
}

}  // namespace sdc
