// Temporal softmax attention at 64 / 96 / 128 frames on the matrix cores, both directions, and the one
// routing predicate of the softmax attention cores, sdc_attn_route.  Reached only through sdc_attn / sdc_attn_bwd.
//
// Domain: frame-strided tokens (q_st != 1), contiguous pixels (q_si == o_si == 1), ntok = F in {64, 96, 128}, any inner >= 1, rot
// and bias each null or not, heads x 32 channels.  fp32 operands, v_mfma_f32_32x32x2_f32, NB = F / 32 blocks of 32 frames.
//
// A workgroup owns NP adjacent pixels of one head (a group never straddles `outer`; the last group of a sample may be ragged:
// absent pixels are zero in LDS, no address is formed for them and their stores are skipped).  q' = rot(q scale), k' = rot(k),
// v (and dO) live in LDS as [d][frame] images of pitch F + 1 (conflict-free along either index), one image per pixel.
#include "sdc_common.h"
#include "sdc_attn_long.h"
#include "sdc_tattn_frames.h"

namespace {

constexpr int DH = 32;
constexpr float SCALE = 0.17677669529663687f;       // dim_head^-0.5
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float nfloat4 __attribute__((ext_vector_type(4)));

struct TfArgs {
    const float* qkv; const float* dout; const float* rot; const float* bias;
    float* out;                 // forward: out; backward: dqkv
    float* dbias_part;
    int inner, heads, gpo, ngrp, nslots, bias_al16;       // gpo = pixel groups per `outer`
    int64_t so, sc, st, oso, osc, ost;
};

// floats per pixel image: 32 rows of pitch F + 1, padded so that the NP pixels of a staging store (lanes = pixel fastest, then
// frame) land 64 / NP banks apart
__host__ __device__ constexpr int tf_img(int F, int NP) { return 32 * (F + 1) + 32 + 64 / NP; }

// the row a 32x32 accumulator register holds: lane (column = lane & 31, half lh = lane >> 5), register r
__device__ __forceinline__ int tf_row(int r, int lh) { return 8 * (r >> 2) + 4 * lh + (r & 3); }

// acc[kbk][r] += bias[head][query][kbk*32 + tf_row(r)] for this lane's query: four adjacent keys per (kbk, r >> 2)
template <int NB>
__device__ __forceinline__ void tf_add_bias_rows(f32x16 (&acc)[NB], const float* brow, int lh, int al16) {
#pragma unroll
    for (int kbk = 0; kbk < NB; ++kbk)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float* p = brow + kbk * 32 + 8 * g + 4 * lh;
            if (al16) {
                const nfloat4 b = *reinterpret_cast<const nfloat4*>(p);
                acc[kbk][4 * g] += b.x; acc[kbk][4 * g + 1] += b.y; acc[kbk][4 * g + 2] += b.z; acc[kbk][4 * g + 3] += b.w;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[kbk][4 * g + j] += p[j];
            }
        }
}

// ------------------------------------------------------------------------------------------------ forward
// 256 threads; wave w owns the pixels w*PPW .. w*PPW + PPW - 1 (PPW = NP / 4), so nothing below crosses waves but the staging.
//   1. stage q scale and k into the two image sets, rotate both in place (rot from global: L1-resident [F][16][2])
//   2. every wave lifts the B fragments of its q' blocks into registers (16 per 32-query block); v, requested during the rotary,
//      then takes the q images' place (the Q / V reuse of tattn_kernel: two image sets instead of three)
//   3. per (pixel, 32-query block): S^T[key][query] = K' Q'^T over the NB key blocks stays in registers (NB x 16 accumulators: a
//      query's scores sit in two lanes), + bias ([key][query] tiles read from global, four adjacent keys per load), exact softmax
//      over the row, then O[query][d] = P^T V with the P registers as the A operand as they stand
//   4. the wave's O tiles replace its own pixels' v images; the output leaves in pixel-contiguous runs
template <int NB, int NP>
__global__ __launch_bounds__(256) void tfr_fwd_kernel(const TfArgs a) {
    constexpr int F = NB * 32, P = F + 1, IMG = tf_img(F, NP), PPW = NP / 4, NIT = NP * F / 8, NTH = 256;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* const Ks = lds;                         // [NP][IMG]
    float* const QV = lds + NP * IMG;              // q', then v, then O
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lh = lane >> 5;
    const int head = blockIdx.x % a.heads, grp = blockIdx.x / a.heads;
    const int o = grp / a.gpo, i0 = (grp - o * a.gpo) * NP;
    const int npx = a.inner - i0 < NP ? a.inner - i0 : NP;
    const float* qb = a.qkv + o * a.so + i0 + (int64_t)(head * DH) * a.sc;
    const float* kb = qb + (int64_t)(a.heads * DH) * a.sc;
    const float* vb = kb + (int64_t)(a.heads * DH) * a.sc;
    float* ob = a.out + o * a.oso + i0 + (int64_t)(head * DH) * a.osc;

    // element e = tid + 256 it -> (pixel = e % NP, frame = (e / NP) % F, d = e / (NP F))
#pragma unroll 8
    for (int it = 0; it < NIT; ++it) {
        const int e = tid + it * NTH;
        const int hw = e % NP, f = (e / NP) % F, d = e / (NP * F);
        float qv = 0.f, kv = 0.f;
        if (hw < npx) {
            const int64_t g = (int64_t)d * a.sc + (int64_t)f * a.st + hw;
            qv = qb[g] * SCALE;
            kv = kb[g];
        }
        Ks[hw * IMG + d * P + f] = kv;
        QV[hw * IMG + d * P + f] = qv;
    }
    float vreg[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int e = tid + it * NTH;
        const int hw = e % NP, f = (e / NP) % F, d = e / (NP * F);
        vreg[it] = hw < npx ? vb[(int64_t)d * a.sc + (int64_t)f * a.st + hw] : 0.f;
    }
    __syncthreads();
    if (a.rot) {
        // rotate (d = 2m, 2m+1) pairs of q and k in place; angle = frame * freq[m]
        for (int e = tid; e < NP * 16 * F; e += NTH) {
            const int f = e % F, m = (e / F) & 15, hw = e / (F * 16);
            const float c = a.rot[(f * 16 + m) * 2], sn = a.rot[(f * 16 + m) * 2 + 1];
            const int l0 = hw * IMG + (2 * m) * P + f, l1 = l0 + P;
            float x0 = Ks[l0], x1 = Ks[l1];
            Ks[l0] = x0 * c - x1 * sn; Ks[l1] = x1 * c + x0 * sn;
            x0 = QV[l0]; x1 = QV[l1];
            QV[l0] = x0 * c - x1 * sn; QV[l1] = x1 * c + x0 * sn;
        }
        __syncthreads();
    }
    // B fragments of Q'^T: B[d = 2s + lh][query = l31] of block qbk of pixel wave*PPW + u
    float qf[PPW * NB][16];
#pragma unroll
    for (int u = 0; u < PPW; ++u)
#pragma unroll
        for (int qbk = 0; qbk < NB; ++qbk)
#pragma unroll
            for (int s = 0; s < 16; ++s) qf[u * NB + qbk][s] = QV[(wave * PPW + u) * IMG + (2 * s + lh) * P + qbk * 32 + l31];
    __syncthreads();                                   // every wave has its q' fragments: v takes the images
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int e = tid + it * NTH;
        const int hw = e % NP, f = (e / NP) % F, d = e / (NP * F);
        QV[hw * IMG + d * P + f] = vreg[it];
    }
    __syncthreads();

#pragma unroll
    for (int u = 0; u < PPW; ++u) {
        const int px = wave * PPW + u;
        const float* Ki = Ks + px * IMG;
        float* Vi = QV + px * IMG;
        f32x16 oacc[NB];
#pragma unroll
        for (int qbk = 0; qbk < NB; ++qbk) {
            // (an offset the compiler cannot see through keeps the K / V fragment reads inside this block instead of hoisted
            // out of the unrolled loops and spilled, as in attn256_kernel)
            int koff = lh * P + l31, voff = l31 * P + 4 * lh;
            asm volatile("" : "+v"(koff), "+v"(voff));
            f32x16 sc[NB];
#pragma unroll
            for (int kbk = 0; kbk < NB; ++kbk) {
#pragma unroll
                for (int r = 0; r < 16; ++r) sc[kbk][r] = 0.f;
#pragma unroll
                for (int s = 0; s < 16; ++s)           // A[key = l31][d = 2s + lh]
                    sc[kbk] = __builtin_amdgcn_mfma_f32_32x32x2f32(Ki[koff + (2 * s) * P + kbk * 32], qf[u * NB + qbk][s], sc[kbk], 0, 0, 0);
            }
            // lane (query = l31, half lh) holds keys kbk*32 + tf_row(r)
            if (a.bias) tf_add_bias_rows<NB>(sc, a.bias + ((int64_t)head * F + qbk * 32 + l31) * F, lh, a.bias_al16);
            float mx = -INFINITY;
#pragma unroll
            for (int kbk = 0; kbk < NB; ++kbk)
#pragma unroll
                for (int r = 0; r < 16; ++r) mx = fmaxf(mx, sc[kbk][r]);
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            float sum = 0.f;
#pragma unroll
            for (int kbk = 0; kbk < NB; ++kbk)
#pragma unroll
                for (int r = 0; r < 16; ++r) { sc[kbk][r] = sdc::softmax_exp(sc[kbk][r] - mx); sum += sc[kbk][r]; }
            sum += __shfl_xor(sum, 32, 64);
            const float inv = 1.0f / sum;
#pragma unroll
            for (int kbk = 0; kbk < NB; ++kbk)
#pragma unroll
                for (int r = 0; r < 16; ++r) sc[kbk][r] *= inv;
            // O[query][d] = sum_key P[query][key] V[key][d]: A = P registers (k-step r of block kbk), B[key][d = l31]
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
            for (int kbk = 0; kbk < NB; ++kbk)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(sc[kbk][r], Vi[voff + kbk * 32 + (r & 3) + 8 * (r >> 2)], acc, 0, 0, 0);
            oacc[qbk] = acc;
        }
        // this pixel's v image is read by this wave alone: its O tiles take its place.  lane (d = l31) holds queries tf_row(r)
#pragma unroll
        for (int qbk = 0; qbk < NB; ++qbk)
#pragma unroll
            for (int r = 0; r < 16; ++r) Vi[l31 * P + qbk * 32 + tf_row(r, lh)] = oacc[qbk][r];
    }
    __syncthreads();
#pragma unroll 8
    for (int it = 0; it < NIT; ++it) {
        const int e = tid + it * NTH;
        const int hw = e % NP, f = (e / NP) % F, d = e / (NP * F);
        if (hw < npx) ob[(int64_t)d * a.osc + (int64_t)f * a.ost + hw] = QV[hw * IMG + d * P + f];
    }
}

// ------------------------------------------------------------------------------------------------ backward
// The products of tattn_bwd_kernel in its two orientations, over NB blocks.  64 NB G threads: wave w is bound to the frame block
// b = w % NB and to the pixel lane g = w / NB, and walks the pixels g, g + G, ... of the group.  Per pixel:
//   orientation 1 (lanes = queries of block b): S^T = K' Q'^T and dP^T = V dO^T over the NB key blocks -> row maximum, 1 / row
//       sum and D (to LDS), dS^T in registers (added to this wave's bias-gradient registers) -> dQ' = dS K'
//   orientation 2 (lanes = keys of block b):    S = Q' K'^T and dP = dO V^T over the NB query blocks -> P, dS from the statistics
//       -> dK' = dS^T Q', dV = P^T dO
// then dq', dk' are un-rotated and the three gradient tiles replace the block's part of the q, k, v images, which leave in
// pixel-contiguous runs.  No atomics, one owner per output element; workgroups walk pixel groups in a fixed assignment (slot,
// slot + nslots, ...) and the bias gradient leaves as one partial table per slot.
template <int NB, int NP, int G>
__global__ __launch_bounds__(64 * NB * G) void tfr_bwd_kernel(const TfArgs a) {
    constexpr int F = NB * 32, P = F + 1, IMG = tf_img(F, NP), NTH = 64 * NB * G, TOT = 32 * F * NP;
    static_assert(NP % G == 0, "every wave walks the same number of pixels");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* const img = lds;                            // [4 tensors][NP][IMG]: q', k', v, dO
    float* const stat = lds + 4 * NP * IMG;            // [NP][3][F]: row max, 1 / row sum, D
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lh = lane >> 5;
    const int blk = wave % NB, g = wave / NB;
    const int head = blockIdx.x % a.heads, slot = blockIdx.x / a.heads;
    auto IMGP = [&](int t, int px) -> float* { return img + (t * NP + px) * IMG; };
    f32x16 dbacc[NB];                                  // dS^T[key = kbk*32 + tf_row(r)][query = blk*32 + l31] over this wave's pixels
#pragma unroll
    for (int kbk = 0; kbk < NB; ++kbk)
#pragma unroll
        for (int r = 0; r < 16; ++r) dbacc[kbk][r] = 0.f;

    for (int grp = slot; grp < a.ngrp; grp += a.nslots) {
        const int o = grp / a.gpo, i0 = (grp - o * a.gpo) * NP;
        const int npx = a.inner - i0 < NP ? a.inner - i0 : NP;
        const float* qb = a.qkv + o * a.so + i0 + (int64_t)(head * DH) * a.sc;
        const float* kb = qb + (int64_t)(a.heads * DH) * a.sc;
        const float* vb = kb + (int64_t)(a.heads * DH) * a.sc;
        const float* gb = a.dout + o * a.oso + i0 + (int64_t)(head * DH) * a.osc;
        __syncthreads();                                   // the previous group's stores have read the images
        // ---- stage q (scaled), k, v, dO: element e -> (pixel = e % NP, frame = (e / NP) % F, d = e / (NP F))
#pragma unroll 4
        for (int e = tid; e < TOT; e += NTH) {
            const int hw = e % NP, f = (e / NP) % F, d = e / (NP * F);
            float qv = 0.f, kv = 0.f, vv = 0.f, gv = 0.f;
            if (hw < npx) {
                const int64_t gi = (int64_t)d * a.sc + (int64_t)f * a.st + hw;
                qv = qb[gi] * SCALE;
                kv = kb[gi];
                vv = vb[gi];
                gv = gb[(int64_t)d * a.osc + (int64_t)f * a.ost + hw];
            }
            const int li = d * P + f;
            IMGP(0, hw)[li] = qv; IMGP(1, hw)[li] = kv; IMGP(2, hw)[li] = vv; IMGP(3, hw)[li] = gv;
        }
        __syncthreads();
        if (a.rot) {
            for (int e = tid; e < NP * 16 * F; e += NTH) {
                const int f = e % F, m = (e / F) & 15, px = e / (F * 16);
                const float c = a.rot[(f * 16 + m) * 2], sn = a.rot[(f * 16 + m) * 2 + 1];
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    float* p0 = IMGP(t, px) + (2 * m) * P + f;
                    const float x0 = p0[0], x1 = p0[P];
                    p0[0] = x0 * c - x1 * sn;
                    p0[P] = x1 * c + x0 * sn;
                }
            }
            __syncthreads();
        }
        for (int p0 = 0; p0 < NP; p0 += G) {
            const int px = p0 + g;
            float* Qi = IMGP(0, px);
            float* Ki = IMGP(1, px);
            float* Vi = IMGP(2, px);
            float* Gi = IMGP(3, px);
            float* const st_m = stat + px * 3 * F, * const st_l = st_m + F, * const st_d = st_m + 2 * F;
            int foff = lh * P + l31, roff = l31 * P + 4 * lh;      // fragment offsets the compiler cannot see through (no hoisting)
            asm volatile("" : "+v"(foff), "+v"(roff));
            f32x16 dq;
            {
                // orientation 1: lanes = queries of block blk.  dP^T is formed twice, one key block at a time (once for D, once for
                // dS): holding its NB tiles next to S^T's and the bias gradient's does not fit the register file without scratch
                f32x16 sT[NB];
#pragma unroll
                for (int kbk = 0; kbk < NB; ++kbk) {
                    asm volatile("" : "+v"(foff));         // (one key block's fragments at a time: see above)
#pragma unroll
                    for (int r = 0; r < 16; ++r) sT[kbk][r] = 0.f;
#pragma unroll
                    for (int s2 = 0; s2 < 16; ++s2)
                        sT[kbk] = __builtin_amdgcn_mfma_f32_32x32x2f32(Ki[foff + (2 * s2) * P + kbk * 32], Qi[foff + (2 * s2) * P + blk * 32], sT[kbk], 0, 0, 0);
                }
                if (a.bias) {
                    int boff = (blk * 32 + l31) * F;       // (fenced like the fragment offsets: the bias loads stay here)
                    asm volatile("" : "+v"(boff));
                    tf_add_bias_rows<NB>(sT, a.bias + (int64_t)head * F * F + boff, lh, a.bias_al16);
                }
                float mx = -INFINITY;
#pragma unroll
                for (int kbk = 0; kbk < NB; ++kbk)
#pragma unroll
                    for (int r = 0; r < 16; ++r) mx = fmaxf(mx, sT[kbk][r]);
                mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
                float sum = 0.f;
#pragma unroll
                for (int kbk = 0; kbk < NB; ++kbk)
#pragma unroll
                    for (int r = 0; r < 16; ++r) { sT[kbk][r] = sdc::softmax_exp(sT[kbk][r] - mx); sum += sT[kbk][r]; }
                sum += __shfl_xor(sum, 32, 64);
                const float inv = 1.0f / sum;
                float D = 0.f;
#pragma unroll
                for (int kbk = 0; kbk < NB; ++kbk) {
                    asm volatile("" : "+v"(foff));
                    f32x16 dpT;
#pragma unroll
                    for (int r = 0; r < 16; ++r) dpT[r] = 0.f;
#pragma unroll
                    for (int s2 = 0; s2 < 16; ++s2)
                        dpT = __builtin_amdgcn_mfma_f32_32x32x2f32(Vi[foff + (2 * s2) * P + kbk * 32], Gi[foff + (2 * s2) * P + blk * 32], dpT, 0, 0, 0);
#pragma unroll
                    for (int r = 0; r < 16; ++r) { sT[kbk][r] *= inv; D += sT[kbk][r] * dpT[r]; }
                }
                D += __shfl_xor(D, 32, 64);
                if (lh == 0) { st_m[blk * 32 + l31] = mx; st_l[blk * 32 + l31] = inv; st_d[blk * 32 + l31] = D; }
                // dQ'[q][d] = sum_key dS[q][key] K'[key][d]: A = dS^T registers, B[key][d = l31]
#pragma unroll
                for (int r = 0; r < 16; ++r) dq[r] = 0.f;
#pragma unroll
                for (int kbk = 0; kbk < NB; ++kbk) {
                    asm volatile("" : "+v"(foff), "+v"(roff));
                    f32x16 dpT;
#pragma unroll
                    for (int r = 0; r < 16; ++r) dpT[r] = 0.f;
#pragma unroll
                    for (int s2 = 0; s2 < 16; ++s2)
                        dpT = __builtin_amdgcn_mfma_f32_32x32x2f32(Vi[foff + (2 * s2) * P + kbk * 32], Gi[foff + (2 * s2) * P + blk * 32], dpT, 0, 0, 0);
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float ds = sT[kbk][r] * (dpT[r] - D);                  // dS^T[key][query]
                        dbacc[kbk][r] += ds;
                        dq = __builtin_amdgcn_mfma_f32_32x32x2f32(ds, Ki[roff + kbk * 32 + (r & 3) + 8 * (r >> 2)], dq, 0, 0, 0);
                    }
                }
            }
            __syncthreads();                               // the statistics of every query block of these pixels are in LDS
            f32x16 dk, dv;
#pragma unroll
            for (int r = 0; r < 16; ++r) { dk[r] = 0.f; dv[r] = 0.f; }
            // orientation 2: lanes = keys of block blk, rows = queries qb2*32 + tf_row(r); one query block at a time, so only two
            // accumulator tiles are live next to dk and dv
            const float* bcol = a.bias ? a.bias + (int64_t)head * F * F + blk * 32 + l31 : nullptr;
#pragma unroll
            for (int qb2 = 0; qb2 < NB; ++qb2) {
                f32x16 sN, dpN;
                int boff = qb2 * 32 * F;
                asm volatile("" : "+v"(foff), "+v"(roff), "+v"(boff));
#pragma unroll
                for (int r = 0; r < 16; ++r) { sN[r] = 0.f; dpN[r] = 0.f; }
#pragma unroll
                for (int s2 = 0; s2 < 16; ++s2) {
                    const int lq = foff + (2 * s2) * P + qb2 * 32, lk = foff + (2 * s2) * P + blk * 32;
                    sN = __builtin_amdgcn_mfma_f32_32x32x2f32(Qi[lq], Ki[lk], sN, 0, 0, 0);
                    dpN = __builtin_amdgcn_mfma_f32_32x32x2f32(Gi[lq], Vi[lk], dpN, 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int q = qb2 * 32 + tf_row(r, lh);
                    const float b = bcol ? bcol[boff + tf_row(r, lh) * F] : 0.f;
                    const float p = sdc::softmax_exp(sN[r] + b - st_m[q]) * st_l[q];
                    sN[r] = p;                                    // P[q][key]
                    dpN[r] = p * (dpN[r] - st_d[q]);              // dS[q][key]
                }
                // dK'[key][d] += sum_q dS[q][key] Q'[q][d],  dV[key][d] += sum_q P[q][key] dO[q][d]
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int li = roff + qb2 * 32 + (r & 3) + 8 * (r >> 2);
                    dk = __builtin_amdgcn_mfma_f32_32x32x2f32(dpN[r], Qi[li], dk, 0, 0, 0);
                    dv = __builtin_amdgcn_mfma_f32_32x32x2f32(sN[r], Gi[li], dv, 0, 0, 0);
                }
            }
            __syncthreads();                               // every wave is done reading these pixels' images
            // transposed rotation of dq', dk' (pairs = adjacent lanes d, d ^ 1), the scale of q; the tiles replace block blk of the images
            int m = l31 >> 1;
            asm volatile("" : "+v"(m));
            const bool odd = l31 & 1;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int f = blk * 32 + tf_row(r, lh);
                float c = 1.0f, sn = 0.0f;
                if (a.rot) { c = a.rot[(f * 16 + m) * 2]; sn = a.rot[(f * 16 + m) * 2 + 1]; }
                const float pq = __shfl_xor(dq[r], 1, 64), pk = __shfl_xor(dk[r], 1, 64);
                const float rq = dq[r] * c + (odd ? -pq : pq) * sn;
                const float rk = dk[r] * c + (odd ? -pk : pk) * sn;
                Qi[l31 * P + f] = rq * SCALE;
                Ki[l31 * P + f] = rk;
                Vi[l31 * P + f] = dv[r];
            }
        }
        __syncthreads();
        // ---- gradients back to the channel-major tensor
        float* dqb = a.out + o * a.so + i0 + (int64_t)(head * DH) * a.sc;
        float* dkb = dqb + (int64_t)(a.heads * DH) * a.sc;
        float* dvb = dkb + (int64_t)(a.heads * DH) * a.sc;
#pragma unroll 4
        for (int e = tid; e < TOT; e += NTH) {
            const int hw = e % NP, f = (e / NP) % F, d = e / (NP * F);
            if (hw < npx) {
                const int64_t gi = (int64_t)d * a.sc + (int64_t)f * a.st + hw;
                const int li = d * P + f;
                dqb[gi] = IMGP(0, hw)[li];
                dkb[gi] = IMGP(1, hw)[li];
                dvb[gi] = IMGP(2, hw)[li];
            }
        }
    }
    if (a.dbias_part) {
        __syncthreads();
        if (G > 1) {
            // the pixel lanes of one frame block meet in a fixed order: lane g = 1 parks its registers, lane 0 adds them
            float* tmp = lds + blk * (NB * 16 * 64);       // [NB blocks][NB*16 registers][64 lanes], the images are dead
            if (g == 1) {
#pragma unroll
                for (int kbk = 0; kbk < NB; ++kbk)
#pragma unroll
                    for (int r = 0; r < 16; ++r) tmp[(kbk * 16 + r) * 64 + lane] = dbacc[kbk][r];
            }
            __syncthreads();
            if (g == 0) {
#pragma unroll
                for (int kbk = 0; kbk < NB; ++kbk)
#pragma unroll
                    for (int r = 0; r < 16; ++r) dbacc[kbk][r] += tmp[(kbk * 16 + r) * 64 + lane];
            }
        }
        if (g == 0) {
            float* out = a.dbias_part + (((int64_t)slot * a.heads + head) * F + blk * 32 + l31) * F;      // row of this lane's query
#pragma unroll
            for (int kbk = 0; kbk < NB; ++kbk)
#pragma unroll
                for (int r = 0; r < 16; ++r) out[kbk * 32 + tf_row(r, lh)] = dbacc[kbk][r];
        }
    }
}

// LDS footprints (bytes), all <= 160 KB = 163840:
//   forward   2 image sets x NP x tf_img(F, NP) floats:   F = 64, NP = 8: 2 x 8 x 2120 x 4 = 135680
//                                                         F = 96, NP = 4: 2 x 4 x 3152 x 4 = 100864
//                                                         F = 128, NP = 4: 2 x 4 x 4176 x 4 = 133632
//   backward  4 image sets x NP x tf_img + NP x 3 x F:    F = 64, NP = 4: (16 x 2128 + 768) x 4 = 139264
//                                                         F = 96, NP = 2: (8 x 3168 + 576) x 4 = 103680
//                                                         F = 128, NP = 2: (8 x 4192 + 768) x 4 = 137216
//   (four images of a pixel at 128 frames are 66 KB: two pixels are what fits, in one kernel -- no split into two launches)
constexpr size_t tf_fwd_lds(int F, int NP) { return sizeof(float) * (size_t)(2 * NP * tf_img(F, NP)); }
constexpr size_t tf_bwd_lds(int F, int NP) { return sizeof(float) * (size_t)(4 * NP * tf_img(F, NP) + NP * 3 * F); }
static_assert(tf_fwd_lds(64, 8) <= 160 * 1024 && tf_fwd_lds(96, 4) <= 160 * 1024 && tf_fwd_lds(128, 4) <= 160 * 1024, "forward LDS");
static_assert(tf_bwd_lds(64, 4) <= 160 * 1024 && tf_bwd_lds(96, 2) <= 160 * 1024 && tf_bwd_lds(128, 2) <= 160 * 1024, "backward LDS");
static_assert(2 * 2 * 16 * 64 <= 16 * tf_img(64, 4), "the G = 2 bias-gradient exchange fits the dead images");

constexpr int tf_fwd_np(int ntok) { return ntok == 64 ? 8 : 4; }
constexpr int tf_bwd_np(int ntok) { return ntok == 64 ? 4 : 2; }

template <int NB, int NP>
int launch_fwd(const TfArgs& a, unsigned grid, void* stream) {
    static std::atomic<uint64_t> attr{0};
    SDC_LDS_OPTIN(attr, (tfr_fwd_kernel<NB, NP>), 160 * 1024, "sdc_attn[frames]");
    hipLaunchKernelGGL((tfr_fwd_kernel<NB, NP>), dim3(grid), dim3(256), tf_fwd_lds(NB * 32, NP), sdc::as_stream(stream), a);
    return sdc::check_launch("sdc_attn[frames]");
}

template <int NB, int NP, int G>
int launch_bwd(const TfArgs& a, unsigned grid, void* stream) {
    static std::atomic<uint64_t> attr{0};
    SDC_LDS_OPTIN(attr, (tfr_bwd_kernel<NB, NP, G>), 160 * 1024, "sdc_attn_bwd[frames]");
    hipLaunchKernelGGL((tfr_bwd_kernel<NB, NP, G>), dim3(grid), dim3(64 * NB * G), tf_bwd_lds(NB * 32, NP), sdc::as_stream(stream), a);
    return sdc::check_launch("sdc_attn_bwd[frames]");
}

// The forward's speed table (profiles/tattn_frames.log): a shape goes to the frames kernel only where its measured range lies
// wholly below attn_kernel's on the same box.  Keyed on ntok and the per-sample inner alone.  Every shape measured -- 64 and 128
// frames at inner 4096 / 1024 / 256 -- does, by 1.6 x to 2.7 x, so the table has no exception today; smaller inner (the 16- and
// 4-pixel levels of a dim-8 net) and 96 frames were not timed and follow their neighbours.
bool frames_fwd_faster(int ntok, int inner) {
    (void)ntok; (void)inner;
    return true;
}

}  // namespace

namespace sdc {

int tattn_frames(const float* qkv, float* out, const float* rot, const float* bias, int outer, int inner, int heads, int ntok,
                 int64_t q_so, int64_t q_sc, int64_t q_st, int64_t o_so, int64_t o_sc, int64_t o_st, void* stream) {
    TfArgs a{};
    a.qkv = qkv; a.out = out; a.rot = rot; a.bias = bias;
    a.inner = inner; a.heads = heads;
    a.so = q_so; a.sc = q_sc; a.st = q_st; a.oso = o_so; a.osc = o_sc; a.ost = o_st;
    a.bias_al16 = reinterpret_cast<uintptr_t>(bias) % 16 == 0;
    const int np = tf_fwd_np(ntok);
    a.gpo = (inner + np - 1) / np;
    const int64_t nwg = (int64_t)outer * a.gpo * heads;
    SDC_REQUIRE(nwg < (1ll << 31), SDC_EINVAL, "sdc_attn: outer * ceil(inner / %d) * heads must be < 2^31", np);
    a.ngrp = outer * a.gpo;
    if (ntok == 64) return launch_fwd<2, 8>(a, (unsigned)nwg, stream);
    if (ntok == 96) return launch_fwd<3, 4>(a, (unsigned)nwg, stream);
    return launch_fwd<4, 4>(a, (unsigned)nwg, stream);
}

size_t tattn_frames_bwd_bytes(int heads, int ntok) { return (size_t)TATTN_FRAMES_SLOTS * heads * ntok * ntok * sizeof(float); }

int tattn_frames_bwd(const float* qkv, const float* dout, const float* rot, const float* bias, float* dqkv, float* dbias_part,
                     int* nslots, int outer, int inner, int heads, int ntok, int64_t q_so, int64_t q_sc, int64_t q_st,
                     int64_t o_so, int64_t o_sc, int64_t o_st, void* stream) {
    TfArgs a{};
    a.qkv = qkv; a.dout = dout; a.out = dqkv; a.rot = rot; a.bias = bias; a.dbias_part = dbias_part;
    a.inner = inner; a.heads = heads;
    a.so = q_so; a.sc = q_sc; a.st = q_st; a.oso = o_so; a.osc = o_sc; a.ost = o_st;
    a.bias_al16 = reinterpret_cast<uintptr_t>(bias) % 16 == 0;
    const int np = tf_bwd_np(ntok);
    a.gpo = (inner + np - 1) / np;
    const int64_t ngrp = (int64_t)outer * a.gpo;
    SDC_REQUIRE(ngrp < (1ll << 31), SDC_EINVAL, "sdc_attn_bwd: outer * ceil(inner / %d) must be < 2^31", np);
    a.ngrp = (int)ngrp;
    a.nslots = a.ngrp < TATTN_FRAMES_SLOTS ? a.ngrp : TATTN_FRAMES_SLOTS;
    *nslots = a.nslots;
    const unsigned grid = (unsigned)(a.nslots * heads);
    if (ntok == 64) return launch_bwd<2, 4, 2>(a, grid, stream);
    if (ntok == 96) return launch_bwd<3, 2, 1>(a, grid, stream);
    return launch_bwd<4, 2, 1>(a, grid, stream);
}

}  // namespace sdc

// The one routing predicate of sdc_attn / sdc_attn_bwd: host arithmetic on the shape and strides alone (no device, no pointer, no
// `outer`).  0 generic, 1 32-frame MFMA, 2 256-token MFMA, 3 streaming, 4 frames; SDC_EINVAL with the entry point's message
// for a call it refuses.  Route 2 is reported for every shape in attn256_kernel's domain: whether the operands are 16-byte
// aligned is not a property of the shape, and a call that is not falls back to route 0 inside sdc_attn.
extern "C" int sdc_attn_route(int inner, int ntok, int64_t q_si, int64_t q_st, int64_t o_si, int64_t o_st, int has_rot, int has_bias,
                              int want_dbias, int backward) {
    const char* who = backward ? "sdc_attn_bwd" : "sdc_attn";
    SDC_REQUIRE(inner > 0 && ntok > 0, SDC_EINVAL, "%s: bad shape (ntok=%d)", who, ntok);
    const bool tok_contig = q_st == 1;
    if (ntok > 256) {
        if (backward)
            SDC_REQUIRE(!has_rot && !has_bias && !want_dbias && q_st == 1 && o_st == 1 && ntok <= sdc::ATTN_LONG_MAX, SDC_EINVAL,
                        "sdc_attn_bwd: bad shape (ntok=%d): more than 256 tokens need rot == bias == dbias == null, contiguous tokens "
                        "(q_st == o_st == 1) and ntok <= %d", ntok, sdc::ATTN_LONG_MAX);
        else
            SDC_REQUIRE(!has_rot && !has_bias && q_st == 1 && o_st == 1 && ntok <= sdc::ATTN_LONG_MAX, SDC_EINVAL,
                        "sdc_attn: bad shape (ntok=%d): more than 256 tokens need rot == bias == null, contiguous tokens (q_st == o_st == 1) "
                        "and ntok <= %d", ntok, sdc::ATTN_LONG_MAX);
        return 3;
    }
    // the frames domain; frame stride x ntok x 4 bytes < 2^32 for both tensors, the 32-frame kernel's lane-offset rule
    const bool frames = !tok_contig && sdc::tattn_frames_ntok(ntok) && q_si == 1 && o_si == 1 && q_st > 0 && o_st > 0 &&
                        q_st <= ((1ll << 30) - 1) / ntok && o_st <= ((1ll << 30) - 1) / ntok;
    if (backward) {
        SDC_REQUIRE(!(has_bias && want_dbias) || ntok <= 32 || frames, SDC_EINVAL,
                    "sdc_attn_bwd: the bias gradient is built for ntok <= 32, or 64, 96 or 128 frames with contiguous pixels, and needs the workspace");
        if (frames) return 4;
        if (!tok_contig && ntok == 32 && inner % 8 == 0 && q_si == 1 && o_si == 1) return 1;
        return 0;
    }
    if (frames && frames_fwd_faster(ntok, inner)) return 4;
    if (!tok_contig && ntok == 32 && inner % 8 == 0 && q_si == 1 && o_si == 1 && q_st > 0 && o_st > 0 && q_st < (1ll << 24) && o_st < (1ll << 24))
        return 1;
    if (tok_contig && ntok == 256 && !has_rot && !has_bias && o_st == 1) return 2;
    return 0;
}
