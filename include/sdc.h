/*
 * libsdc_hip.so -- C ABI of the MI355X (gfx950) SafeDiffCon sampler kernels.
 *
 * Drop-in boundary: the reference has no native code on the
 * sampling path -- every stage is a torch.nn op inside
 *   1D/model/diffusion.py      GaussianDiffusion.p_sample_loop / p_sample
 *   tokamak/model/diffusion.py (same)
 *   2d/ddpm/diffusion_2d.py    GaussianDiffusion.p_sample_loop / p_sample
 * and the three U-Nets (1D/model/unet.py, tokamak/model/unet.py,
 * 2d/video_diffusion_pytorch/video_diffusion_pytorch_conv3d.py).  Each entry
 * point below replaces one *stage* of that path and cites the reference lines
 * whose arithmetic it implements.  The binding a reference maintainer adds is a
 * ctypes stub; safediffcon_amd/_lib.py is that stub.
 *
 * Conventions
 *  - plain pointers + sizes, no torch types; all tensors fp32 in device memory
 *    owned by the caller; the library never allocates, frees or retains them
 *    (except inside an explicit graph object, whose lifetime the caller ties
 *    to the buffers it captured).
 *  - every call is asynchronous on `stream` (a hipStream_t passed as void*);
 *    no hidden synchronisation, no host reads of device scalars.  The current
 *    diffusion timestep is a device-resident int (`t_dev`) so that one captured
 *    hipGraph replays for all 1000 steps.
 *  - return 0 on success, negative SDC_E* otherwise; text via sdc_last_error().
 *  - activation layout: (B, C, D, H, W) addressed through explicit element
 *    strides, so Conv1d (D=H=1), Conv2d (D=1), Conv3d and the smoke tensor's
 *    frame-major (B,F,C,H,W) storage all go through the same kernels.
 */
#ifndef SDC_H
#define SDC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SDC_OK 0
#define SDC_EINVAL (-1)      /* bad shape / unsupported configuration */
#define SDC_EALIGN (-2)      /* misaligned pointer */
#define SDC_EHIP (-3)        /* HIP runtime error (launch, capture, ...) */
#define SDC_ENULL (-4)       /* required pointer is null */

int sdc_version(void);
/* copies the calling thread's last error message; returns its length */
int sdc_last_error(char* buf, size_t cap);

/* ------------------------------------------------------------------ conv */
/* Implicit-GEMM N-d convolution on fp32 MFMA (v_mfma_f32_32x32x2_f32), gather
 * straight from the strided input(s):
 *   y[b,co,o] = bias[co] + sum_{tap,ci} Wp[tap*Cin+ci][co] * xcat[b,ci, o*stride - pad + tap] (+ residual[b,co,o])
 * xcat = channel-concat of x0 (Cin0 ch) and x1 (Cin1 ch) -- replaces torch.cat
 * before the up-path ResnetBlocks (1D/model/unet.py:414-418, conv3d.py:553,560).
 * `up` = virtual nearest-neighbour upsample of the input (nn.Upsample(2) + conv,
 * 1D/model/unet.py:24-37); up_mode 1 = zero insertion (ConvTranspose3d as a conv
 * over the zero-stuffed input with flipped taps, conv3d.py:159-160).
 * Replaces: every nn.Conv1d/2d/3d, nn.Linear and nn.ConvTranspose3d on the path
 * (1D/model/unet.py:132-134,161-163,189-197,232-236,326,345,370,378;
 *  conv3d.py:159-163,192,218,239-240,291-292,395,471).
 * Output size per axis: (i*u + 2p - k)/s + 1 (i -> (i-1)*u+1 for zero insertion); up to k-1 more positions are
 * accepted and read implicit zeros past the far edge (one-sided padding), fewer compute a prefix.
 * Wp is the caller-repacked weight [K = taps*Cin][Cout] (row-major, Cout fastest).
 */
typedef struct SdcConvDesc {
    int32_t B, Cin0, Cin1, Cout;
    int32_t iD, iH, iW;          /* stored input spatial size */
    int32_t oD, oH, oW;          /* output spatial size */
    int32_t kD, kH, kW;
    int32_t sD, sH, sW;          /* stride */
    int32_t pD, pH, pW;          /* padding, in the (virtually upsampled) input space */
    int32_t uD, uH, uW;          /* virtual input upsample factor, 1 or 2 */
    int32_t up_mode;             /* 0 nearest, 1 zero-insert */
    int32_t precision;           /* conv algorithm and layout of the wp buffer (0, 2, 3, 4 and 5 are fp32 end to end and differ by
                                    rounding order only; the drop-in nets use 4; 6 and 7 round the 3-tap convs' operands to fp16):
                                    0 = fp32 MFMA, direct implicit GEMM everywhere (k-ordered fp32 FMA chains); wp = Wp
                                    2 = fp32 MFMA, Winograd F(2,3) along W on the 3-wide stride-1 convs (2/3 of the matrix
                                        work); wp = Wp followed, when kW == 3, by the transformed taps
                                        Wg[(kd*kH + kh)*4 + xi][Cin][Cout]  (G g, G = [[1,0,0],[.5,.5,.5],[.5,-.5,.5],[0,0,1]],
                                        formed in fp64, rounded once); convs the kernel does not cover run the direct kernels
                                    3 = as 2, plus Winograd F(2x2,3x3) over (H, W) for the 3x3 / 3x3x3 stride-1 pad-1 convs over
                                        whole contiguous rows of 16 / 32 / 64 / 128 columns (4/9 of the matrix work): when
                                        kH == kW == 3 the buffer is Wp | Wg | Wg2 with Wg2[kd][ci][co][j*4 + xi] =
                                        sum_{kh,kw} G[j][kh] G[xi][kw] w[co][ci][kd][kh][kw]; other tap shapes: layout of 2.
                                        Shapes the F(2x2,3x3) kernel does not take fall back to 2's kernels on the same buffer.
                                    4 = as 3, plus Winograd F(2x2x2,3x3x3) over (D, H, W) for the 3x3x3 stride-1 pad-1 convs with
                                        an even depth, rows of 16 / 32 / 64 columns and Cout % 64 == 0 (8/27 of the matrix work):
                                        when kD == kH == kW == 3 the buffer is Wp | Wg | Wg2 | Wg3 with Wg3[jd][ci][co][j*4 + xi]
                                        = sum_{kd,kh,kw} G[jd][kd] G[j][kh] G[xi][kw] w[co][ci][kd][kh][kw]; other tap shapes:
                                        layout of 3.  y is used as scratch for partial plane sums while the kernel runs (it
                                        must not alias an input).  Shapes it does not take fall back to 3's kernels.
                                    5 = as 4, plus Winograd F(4,3) along W for the 1-D convs (kD == kH == 1, rows of whole quads,
                                        Cout >= 128; half of the matrix work): such a conv's buffer is Wp | Wg | Wg43 with
                                        Wg43[xi][Cin][Cout], xi < 6, = G43 g (rows (1/4,0,0), (-1/6,-1/6,-1/6), (-1/6,1/6,-1/6),
                                        (1/24,1/12,1/6), (1/24,-1/12,1/6), (0,0,1)).  Opt-in, not the nets' default: on MI355X it is
                                        no faster than 2's kernel (the transform is not hidden behind the MFMAs it saves) and
                                        rounds three times coarser (~3e-6 of the output scale).
                                    6 = as 4, plus fp16 operands with fp32 accumulation (conv_f16_kernel, v_mfma_f32_32x32x16_f16:
                                        activations rounded to fp16 RNE as they are staged, fp32 in HBM) for the 1x1x3 / 1x3x3 /
                                        3x3x3 stride-1 pad-1 convs over rows of 16 / 32 / 64 / 128 columns that its measured dispatch
                                        table lists (csrc/sdc_conv_f16.hip f16_faster, DESIGN.md section 11: every 3x3x3 conv, the 3x3
                                        convs over rows of 64 / 16 and of 32 from 32768 outputs per sample, the 1x3 convs from 32768
                                        outputs per sample; keyed on per-sample sizes, so a sample's bits do not depend on its batch).
                                        Opt-in, samplers only.  For those tap shapes the buffer is 4's buffer, zero-padded to a multiple
                                        of 4 floats (16 bytes), followed by Wh[tap][ci / 32][co][ci % 32] = (fp16, RNE) w[co][ci][tap],
                                        Cin zero-padded to whole chunks of 32 (taps * ceil(Cin / 32) * 32 * Cout / 2 floats: +8 % on a
                                        3x3x3 buffer, +12 % on a 3x3 one, +21 % on a 1x3 one, stored for every such conv, including those
                                        the table leaves on 4's kernels); other tap shapes: layout of 4.  Every other conv, and
                                        sdc_conv_splitk, runs 4's kernels on the buffer's precision-4 prefix.  The GroupNorm sums of
                                        sdc_conv_gn are fused where S % 256 == 0 or whole samples of 64 / 128 positions share a tile.
                                    7 = test and measurement hook, not a user mode: 6 without the dispatch table (every conv the fp16
                                        kernel covers), the same buffer.
                                    (8 is a packing code only, sdc_pack_conv_weight: the fine-tuning layout, read with precision 6 / 7)
                                    Rounding of 6 / 7: fp16 x fp16 products are exact in fp32, so the result is an fp64 conv of the
                                    rounded operands up to fp32 summation order (~2e-4 of the output rms from the operand rounding;
                                    ~1e-6 eps-MSE on the nets).
                                    (1 was a split-bf16 mode in rounds 1-2; removed) */
    int64_t x0s[5], x1s[5], ys[5], rs[5];   /* element strides (b,c,d,h,w) */
} SdcConvDesc;

int sdc_conv(const SdcConvDesc* d, const float* x0, const float* x1, const float* wp, const float* bias,
             const float* residual, float* y, void* stream);

/* sdc_conv for grids that leave most of the chip idle (the fine-tuning step, SURVEY 8f: batch 64 puts the deep 3x3 convs of the
 * Burgers net on 32-128 workgroups for 256 CUs; the samplers' small-batch plan, SURVEY 8e: an 8-way shard of the 1-D configs leaves
 * 16-32 trajectories per GPU): the input channels of an F(2x2,3x3) conv, of a single-tap-row F(2,3) conv (Conv1d k3, with or
 * without the nearest x2 upsampling folded into its gather), or the (tap, channel) walk of a direct-form conv on its smallest tile
 * (1x1, strided, sub-pixel), are split over up to 8 workgroups per output tile, the partial outputs
 * go to `work` (sdc_conv_splitk_bytes(d) bytes, 16-byte aligned; 0 = this conv is not split: the call is then exactly sdc_conv) and
 * are summed in split order -- deterministic, but the split depends on the batch, so a sample's rounding depends on the batch it
 * rides in: the samplers use sdc_conv only unless the caller opts in (net.split_small_grids).  No fused residual.  Precision 6 / 7:
 * precision 4's split kernels on the buffer's precision-4 prefix (fp32; the fp16 kernel never splits K). */
size_t sdc_conv_splitk_bytes(const SdcConvDesc* d);
int sdc_conv_splitk(const SdcConvDesc* d, const float* x0, const float* x1, const float* wp, const float* bias, float* y,
                    float* work, size_t work_bytes, void* stream);

/* Host-side query (measurement tooling, launches nothing): which kernel template instance sdc_conv would run for this
 * descriptor, and the share of the direct-form multiply-adds 2*B*P*Cout*Cin*taps that it issues on the matrix cores
 * (1 for the direct kernels and conv_f16_kernel, 2/3 for Winograd F(2,3) along W, 4/9 for F(2x2,3x3), 8/27 for F(2x2x2,3x3x3)). */
int sdc_conv_describe(const SdcConvDesc* d, char* name, size_t cap, double* mfma_share);

/* Conv + GroupNorm statistics of its output in one pass (the Block.proj -> Block.norm pair, 1D/model/unet.py:132-141,
 * conv3d.py:192-198): the conv epilogue leaves fp64 (sum, sum of squares) pairs per (sample, group, part) in `parts`
 * (B * G * nparts pairs) and sdc_gn_finalize turns them into the {mean, rstd} table sdc_gn_apply reads -- y is not read
 * again for the statistics.  sdc_conv_gnparts is a host-side query: nparts for this descriptor, or 0 when the fused form
 * does not cover it (then run sdc_conv + sdc_gn_stats).  Covered: the precision-2 / 3 / 4 Winograd convs whose tile grid
 * lines up with the samples and groups. */
int sdc_conv_gnparts(const SdcConvDesc* d, int G);
int sdc_conv_gn(const SdcConvDesc* d, const float* x0, const float* x1, const float* wp, const float* bias,
                const float* residual, float* y, double* parts, int G, void* stream);

/* ------------------------------------------------------------- group norm */
/* nn.GroupNorm(G, C, eps=1e-5) statistics over contiguous (B, C, S) data:
 * stats[(b*G+g)*2 + {0,1}] = {mean, rstd}, accumulated in fp64.
 * 1D/model/unet.py:135,140 ; conv3d.py:193,198. */
int sdc_gn_stats(const float* x, float* stats, int B, int C, int G, int64_t S, float eps, void* stream);
/* bytes the caller must allocate for `stats` (mean/rstd pairs + fp64 partial-sum scratch) */
size_t sdc_gn_stats_bytes(int B, int G);
/* stats from the partial sums of sdc_conv_gn: n_per_group = (C / G) * S elements per (sample, group) */
int sdc_gn_finalize(const double* parts, float* stats, int B, int G, int nparts, int64_t n_per_group, float eps, void* stream);

/* y = SiLU( ((x-mean)*rstd*gamma[c]+beta[c]) * (scale+1) + shift ) (+ residual)
 * Block.forward + the ResnetBlock residual add: 1D/model/unet.py:138-147,180 ; conv3d.py:196-204,230.
 * scale/shift come from a time-conditioning table ss (nullable):
 *   row = (t_dev ? *t_dev : 0) * ss_t_stride + b * ss_b_stride
 *   scale = ss[row + ss_off + c], shift = ss[row + ss_off + C + c]
 * (ResnetBlock.mlp output chunked in two, 1D/model/unet.py:169-175). */
int sdc_gn_apply(const float* x, const float* stats, const float* gamma, const float* beta, const float* ss,
                 const int32_t* t_dev, int64_t ss_t_stride, int64_t ss_b_stride, int64_t ss_off,
                 const float* residual, float* y, int B, int C, int G, int64_t S, void* stream);

/* GroupNorm statistics + apply in ONE launch for small groups (sdc_gn_fused_ok: (C/G)*S <= 32768, whatever the batch): the deep levels
 * of Unet2D / Unet1D, 1D/model/unet.py:128-147.  Arguments as sdc_gn_apply (fp64 statistics like sdc_gn_stats). */
int sdc_gn_fused_ok(int B, int C, int G, int64_t S);
int sdc_gn_fused(const float* x, const float* gamma, const float* beta, const float* ss, const int32_t* t_dev,
                 int64_t ss_t_stride, int64_t ss_b_stride, int64_t ss_off, const float* residual, float* y, int B, int C, int G,
                 int64_t S, float eps, void* stream);

/* GroupNorm apply + SiLU (+ residual) of the LAST ResnetBlock inside the 1x1(x1) output conv that is its only reader
 * (2d/video_diffusion_pytorch/video_diffusion_pytorch_conv3d.py:468-471 `final_conv`, 1D/model/unet.py:376-378,
 * tokamak/model/unet.py:355-357): y[b, o, pos] = bias[o] + sum_c w[o][c] * (SiLU((h[b, c, pos] - mean) * rstd * gamma[c] + beta[c]) +
 * residual[b, c, pos]) in one streaming pass -- the normalised tensor is never written.  h / residual contiguous (B, C, S), 16-byte
 * aligned; stats from sdc_gn_stats / sdc_gn_finalize; w = the nn.Conv weight (Cout, C) as it lies, Cout <= 16; y through strides:
 * element (b, o, s) at b * ys0 + o * ys1 + (s / plane) * ys2 + s % plane, plane = H * W (the smoke net writes eps frame-major);
 * plane and the strides multiples of 4 floats.  HBM-bound: 4 * (2 C + Cout) bytes per position. */
int sdc_gn_pointwise_out(const float* h, const float* stats, const float* gamma, const float* beta, const float* residual,
                         const float* w, const float* bias, float* y, int B, int C, int G, int Cout, int64_t S, int64_t plane,
                         int64_t ys0, int64_t ys1, int64_t ys2, void* stream);

/* ------------------------------------------------------- channel norms */
/* mode 0: channel LayerNorm, gain only, (x-mean)*rsqrt(var+eps)*g   1D/model/unet.py:53-63, conv3d.py:165-174
 * mode 1: RMSNorm  x / max(||x||_2,1e-12) * g * sqrt(C)            tokamak/model/unet.py:45-51
 * over contiguous (B, C, S); optional residual add (Residual(...) wrapper, unet.py:16-22). */
int sdc_chan_norm(const float* x, const float* g, const float* residual, float* y, int B, int C, int64_t S,
                  int mode, float eps, void* stream);

/* ---------------------------------------------------- linear attention */
/* LinearAttention / SpatialLinearAttention core, heads x 32:
 *   ctx[d,e] = sum_n softmax_n(k)[d,n] v[e,n] ; out[e,n] = sum_d ctx[d,e] softmax_d(q)[d,n]*scale
 * 1D/model/unet.py:203-221 ; conv3d.py:246-256.
 * qkv is (outer, 3*heads*32, inner, n) through strides: element(outer o, channel c, inner i, token n) at
 *   o*so + c*sc + i*si + n  (tokens contiguous).  out uses the same scheme with heads*32 channels.
 * ctx is workspace of outer*inner*heads*32*32 floats. */
int sdc_linattn(const float* qkv, float* ctx, float* out, int outer, int inner, int heads, int64_t n,
                int64_t q_so, int64_t q_sc, int64_t q_si, int64_t o_so, int64_t o_sc, int64_t o_si, void* stream);

/* Fused LinearAttention block, dim C in {64, 128}, heads 4 x 32, tokens contiguous, n % 64 == 0:
 *   y = x + post( Wo . LA(pre(x)) + bo )
 * i.e. Residual(PreNorm(dim, LinearAttention(dim))) in one call: 1D/model/unet.py:64-71,182-222,341-342;
 * tokamak/model/unet.py:186-222; conv3d.py:176-184,232-258 (SpatialLinearAttention, post_mode -1).
 * pre_mode / post_mode: 0 channel LayerNorm (gain only), 1 RMSNorm, post_mode -1 = none.
 * wqkv = packed 1x1 weight [C][384] (q | k | v), wo = packed [128][C], bo = [C] or null.
 * x and y share the layout element(o, c, i, tok) at o*so + c*sc + i*si + tok.  `work` holds
 * sdc_linattn_block_bytes(...) bytes of scratch.  Three launches: x is read three times, y written once. */
size_t sdc_linattn_block_bytes(int outer, int inner, int C, int64_t n);
int sdc_linattn_block(const float* x, const float* g_pre, const float* wqkv, const float* wo, const float* bo,
                      const float* g_post, float* work, float* y, int outer, int inner, int C, int64_t n,
                      int64_t so, int64_t sc, int64_t si, int pre_mode, int post_mode, float eps, void* stream);
/* The same block reading the RAW output of the producing conv: the ResnetBlock's second GroupNorm + SiLU (+ the residual
 * branch) -- conv3d.py:189-230 block2 / res_conv, consumed only by the attention block that follows (conv3d.py:537-545:
 * block2 -> spatial_attn -> temporal_attn -> skip) -- is applied while pass 1 loads its tiles, instead of in a separate
 * sdc_gn_apply pass:  h = SiLU(x_raw * rstd gamma + (beta - mean rstd gamma)) + residual; pass 1 leaves h in y, where pass 2
 * reads it tile by tile before overwriting it (y must not alias x_raw or the residual).
 * gn_stats = (mean, rstd) per (outer index, group) as sdc_gn_finalize / sdc_gn_stats write them; gn_residual has x_raw's
 * strides or is null.  Same arithmetic as sdc_gn_apply followed by sdc_linattn_block. */
int sdc_linattn_block_gn(const float* x_raw, const float* gn_stats, const float* gn_gamma, const float* gn_beta, int gn_G,
                         const float* gn_residual, const float* g_pre, const float* wqkv, const float* wo, const float* bo,
                         const float* g_post, float* work, float* y, int outer, int inner, int C, int64_t n,
                         int64_t so, int64_t sc, int64_t si, int pre_mode, int post_mode, float eps, void* stream);
/* The two entries above with the kernels chosen by hand (csrc/sdc_lablock_x3.hip): the same arguments with
 * `impl` in front of the stream.  impl 0: every product on the fp32 matrix pipe.  impl 1: the two products with a weight operand,
 * K^T = xn^T Wk^T of pass 1 and Q = Wq xn of pass 2, on the bf16 pipe from exact three-way bf16 splits of both operands (six terms, fp32
 * accumulation: an fp32-grade result in another rounding order); the weights are split inside the kernels from the same packed wqkv,
 * `work` and sdc_linattn_block_bytes are unchanged; everything else -- norms, softmaxes, M^T += xn p, la_blk_mid, y = T q, the residual
 * -- is impl 0's code in impl 0's order.  A non-finite x gives NaN where impl 0 may give an infinity.  Any other impl: SDC_EINVAL,
 * like a bad shape, before any launch.
 * sdc_linattn_block_x3_ok(C, n): 1 at the (C, tokens per sequence) -- never the batch -- where impl 1 measured faster by the
 * per-launch rule; sdc_linattn_block / sdc_linattn_block_gn are the _sel entries with impl = sdc_linattn_block_x3_ok(C, n). */
int sdc_linattn_block_sel(const float* x, const float* g_pre, const float* wqkv, const float* wo, const float* bo,
                          const float* g_post, float* work, float* y, int outer, int inner, int C, int64_t n,
                          int64_t so, int64_t sc, int64_t si, int pre_mode, int post_mode, float eps, int impl, void* stream);
int sdc_linattn_block_gn_sel(const float* x_raw, const float* gn_stats, const float* gn_gamma, const float* gn_beta, int gn_G,
                             const float* gn_residual, const float* g_pre, const float* wqkv, const float* wo, const float* bo,
                             const float* g_post, float* work, float* y, int outer, int inner, int C, int64_t n,
                             int64_t so, int64_t sc, int64_t si, int pre_mode, int post_mode, float eps, int impl, void* stream);
int sdc_linattn_block_x3_ok(int C, int64_t n);

/* The same block with fp16 operands and fp32 accumulation (net.linattn_f16, opt-in, samplers only; DESIGN.md section 20;
 * csrc/sdc_lablock_f16.hip).  A switch of its own: sdc_linattn_block, sdc_linattn_block_gn and their buffers are untouched.  The same
 * three launches, shape domain, strides, token splits and GroupNorm-on-load form.  Rounded once to fp16 (nearest even) as operands of
 * v_mfma_f32_32x32x16_f16, and nothing else: xn, Wq and Wk (at pack time), the un-normalised probabilities p of the softmax over
 * tokens, T = Wo ctx (per sequence), q after its softmax and scale.  fp32: both channel norms, the GroupNorm-on-load arithmetic and
 * the stored h, maxima, exponents, row sums, the split merge, ctx (on the fp32 packed wqkv and wo), every accumulator, the residual
 * add.  p = exp2(k log2e - ceil(m log2e)) with m the running maximum: every rescale factor is an exact power of two, so the rounding
 * of p depends neither on the tile order nor on the split count.  An operand beyond 65504 (T has no bound) becomes infinite.
 *
 * Weight buffer (sdc_pack_linattn_f16_bytes(C) = 512 C bytes, 16-byte aligned; 0 for another C), from the unpacked 1x1 weight to_qkv
 * Wqkv (384, C) -- rows mat * 128 + head * 32 + d, mat = 0 q, 1 k.  Every operand fetch of a lane (l31 = lane & 31, lh = lane >> 5) is
 * one contiguous 16-byte read of 8 fp16 values j = 0 .. 7:
 *   Wh[mat][head][s][lane][j]       = Wqkv[mat * 128 + head * 32 + l31][16 s + 8 lh + j]       mat < 2, head < 4, s < C / 16
 * (256 C values: the q fragments of the four heads, then the k fragments).  to_out Wo (C, 128) is part of the call for symmetry with
 * sdc_pack_tattn_f16 and must not be null, but is not read: T is formed in fp32 from the fp32 packed wo and rounded per sequence.
 * sdc_pack_linattn_f16 writes the buffer on the device, one launch on `stream` (SDC_ENULL for a null pointer, SDC_EINVAL for another
 * C, SDC_EALIGN for a misaligned dst).
 *
 * Scratch (sdc_linattn_block_f16_bytes, 16-byte aligned): the fp32 partials of sdc_linattn_block, then per sequence the fp16 K fragments
 *   Tf[rt][s][lane][j]              = T[32 rt + l31][32 (s >> 1) + row(8 (s & 1) + j, lh)]      rt < C / 32, s < 8
 * with row(r, lh) = (r & 3) + 8 (r >> 2) + 4 lh, the accumulator row that register r of a 32x32 MFMA result holds on half-wave lh: the
 * kernel's q operand arrives in that order.
 *
 * sdc_linattn_block_f16 / sdc_linattn_block_gn_f16: arguments, strides and checks of sdc_linattn_block / sdc_linattn_block_gn with wpk
 * behind (wqkv, wo), which stay the fp32 packed [C][384] / [128][C] weights.  SDC_ENULL for a null pointer, SDC_EINVAL for a bad shape or
 * mode, SDC_EALIGN for a wpk or work that is not 16-byte aligned, all before any launch.  No atomics, fixed accumulation order; a
 * sample's output does not depend on the batch.
 * sdc_linattn_block_f16_ok: 1 where net.linattn_f16 routes a fused site of width C and n tokens per sequence (never the batch) to
 * these entries: every covered (C, n). */
size_t sdc_pack_linattn_f16_bytes(int C);
int sdc_pack_linattn_f16(const float* wqkv, const float* wo, int C, void* dst, void* stream);
size_t sdc_linattn_block_f16_bytes(int outer, int inner, int C, int64_t n);
int sdc_linattn_block_f16(const float* x, const float* g_pre, const float* wqkv, const float* wo, const void* wpk, const float* bo,
                          const float* g_post, void* work, float* y, int outer, int inner, int C, int64_t n,
                          int64_t so, int64_t sc, int64_t si, int pre_mode, int post_mode, float eps, void* stream);
int sdc_linattn_block_gn_f16(const float* x_raw, const float* gn_stats, const float* gn_gamma, const float* gn_beta, int gn_G,
                             const float* gn_residual, const float* g_pre, const float* wqkv, const float* wo, const void* wpk,
                             const float* bo, const float* g_post, void* work, float* y, int outer, int inner, int C, int64_t n,
                             int64_t so, int64_t sc, int64_t si, int pre_mode, int post_mode, float eps, void* stream);
int sdc_linattn_block_f16_ok(int C, int64_t n);

/* Fused temporal-attention block of the smoke U-Net, dim 64, 32 frames, heads 4 x 32:
 *   y = x + Wo . softmax( rot(s Wq xn) rot(Wk xn)^T + relpos ) (Wv xn),  xn = channel LayerNorm(x) * gamma
 * Residual(PreNorm(dim, EinopsToAndFrom(Attention))): conv3d.py:165-184,262-275,277-353,383,402-405.
 * wqkv = packed [64][384] (bias-free Linear), wo = packed [128][64]; rot = [32][16][2] (cos, sin) or null,
 * bias = [heads][query][key] or null.  Element (o, c, pixel i, frame f) of x and y at o*so + c*sc + f*st + i;
 * inner = pixels per outer index, a multiple of 8.
 * wqkv and wo must be 16-byte aligned, rot 8-byte aligned (vector loads); SDC_EINVAL otherwise. */
int sdc_tattn_block(const float* x, const float* g_pre, const float* wqkv, const float* wo, const float* rot,
                    const float* bias, float* y, int outer, int inner, int C, int ntok, int64_t so, int64_t sc,
                    int64_t st, float eps, void* stream);

/* The same block with fp16 operands and fp32 accumulation (net.attn_f16, opt-in, samplers only; DESIGN.md section 16;
 * csrc/sdc_tablock_f16.hip).  A switch of its own: sdc_tattn_block and its buffers are untouched.  fp32: LayerNorm, rotary, bias,
 * softmax (maximum, exponent, row sum, division), every accumulator, the residual add.  Rounded once to fp16 (nearest even) as
 * operands of v_mfma_f32_32x32x16_f16: xn, the weights (at pack time), q and k after the rotary (unscaled), v, the un-normalised
 * probabilities exp(s - max), O after the division by the row sum.  An operand beyond 65504 becomes infinite.
 *
 * Weight buffer (sdc_pack_tattn_f16_bytes() = 65536 bytes, 16-byte aligned), from the nn.Linear weights to_qkv Wqkv (384, 64)
 * -- rows mat * 128 + head * 32 + d, mat = 0 q, 1 k, 2 v -- and to_out Wo (64, 128).  Every operand fetch of a lane (l31 = lane & 31,
 * lh = lane >> 5) is one contiguous 16-byte read of 8 fp16 values j = 0 .. 7:
 *   Wh[head][mat][s][lane][j]       = Wqkv[mat * 128 + head * 32 + l31][16 s + 8 lh + j]           s < 4   (24576 values), then
 *   Wh'[head][i][s][lane][j]        = Wo[32 i + l31][head * 32 + row(8 s + j, lh)]                 i < 2, s < 2   (8192 values)
 * with row(r, lh) = (r & 3) + 8 (r >> 2) + 4 lh, the accumulator row that register r of a 32x32 MFMA result holds on half-wave lh:
 * the kernel's O^T operand arrives in that order.
 * sdc_pack_tattn_f16 writes the buffer on the device, one launch on `stream` (SDC_ENULL for a null pointer, SDC_EALIGN for a
 * misaligned dst).
 *
 * sdc_tattn_block_f16: arguments, strides, tables and checks of sdc_tattn_block with wpk in place of (wqkv, wo); SDC_ENULL for a
 * null x, g_pre, wpk or y, SDC_EINVAL for another shape, SDC_EALIGN for a wpk that is not 16-byte aligned, all before any launch.
 * No atomics, fixed accumulation order; a sample's output does not depend on the batch. */
size_t sdc_pack_tattn_f16_bytes(void);
int sdc_pack_tattn_f16(const float* wqkv, const float* wo, void* dst, void* stream);
int sdc_tattn_block_f16(const float* x, const float* g_pre, const void* wpk, const float* rot, const float* bias, float* y,
                        int outer, int inner, int C, int ntok, int64_t so, int64_t sc, int64_t st, float eps, void* stream);

/* The same block with its weight products -- the q / k / v projections and the out-projection -- formed on the bf16 matrix pipe
 * (v_mfma_f32_32x32x16_bf16) from exact three-way bf16 operand splits, fp32 accumulation (net.attn_split, samplers only, precision 4
 * and 5; csrc/sdc_tablock_x3.hip).  x = h + m + l with round-to-nearest-even bf16 pieces and exact fp32 residuals;
 * a product is the six terms a3 b1 + a2 b2 + a1 b3 + a2 b1 + a1 b2 + a1 b1, the small ones first: an fp32-grade result in another
 * rounding order.  Split: the weights (at pack time), xn (once per tile), O after the softmax normalisation.  fp32 with
 * sdc_tattn_block's instructions and order: LayerNorm, rotary, bias, the score product, softmax, the O = V P product, every
 * accumulator, the residual add.  A non-finite x gives NaN where sdc_tattn_block may give an infinity.
 *
 * Weight buffer (sdc_pack_tattn_x3_bytes() = 196608 bytes, 16-byte aligned), from the unpacked nn.Linear weights to_qkv (384, 64) and
 * to_out (64, 128): Wb[head][piece][e], e < 8192, piece 0 / 1 / 2 = h / m / l -- one head's three pieces are one contiguous run of 48 KB.
 * Position e of a head is sdc_pack_tattn_f16's fragment order restricted to that head:
 *   e = ((mat * 4 + s) * 64 + lane) * 8 + j          <- Wqkv[mat * 128 + head * 32 + l31][16 s + 8 lh + j]     mat < 3, s < 4, then
 *   e = 6144 + ((i * 2 + s) * 64 + lane) * 8 + j     <- Wo[32 i + l31][head * 32 + row(8 s + j, lh)]           i < 2, s < 2.
 * sdc_pack_tattn_x3 writes the buffer on the device, one launch on `stream` (SDC_ENULL for a null pointer, SDC_EALIGN for a
 * misaligned dst).
 *
 * sdc_tattn_block_x3: arguments, strides, tables, checks and error codes of sdc_tattn_block_f16, all before any launch.  No atomics,
 * fixed accumulation order; a sample's output does not depend on the batch.
 * sdc_tattn_block_x3_ok: 1 where the routing table of net.attn_split lists the site -- (C, frames, inner = H * W), never B: the sizes
 * at which the kernel measured faster than sdc_tattn_block in every repeat.
 *
 * sdc_tattn_block_x3_sel: the same arguments plus `impl` in front of the stream.  0 = every wave runs a head between the same two
 * barriers; 1 = waves 4 - 7, the second wave of every SIMD, run half a head behind the first four ("The skewed
 * form").  Same arithmetic, same bits.  Any other impl is SDC_EINVAL before any launch.
 * sdc_tattn_block_x3_impl(C, frames, inner): the measured table of impl -- never keyed on B --: 1 at the sizes where impl 1 beat impl 0
 * in every repeat at the bench batch, 0 everywhere else.  sdc_tattn_block_x3 is the _sel entry with that answer. */
size_t sdc_pack_tattn_x3_bytes(void);
int sdc_pack_tattn_x3(const float* wqkv, const float* wo, void* dst, void* stream);
int sdc_tattn_block_x3(const float* x, const float* g_pre, const void* wpk, const float* rot, const float* bias, float* y,
                       int outer, int inner, int C, int ntok, int64_t so, int64_t sc, int64_t st, float eps, void* stream);
int sdc_tattn_block_x3_ok(int C, int ntok, int inner);
int sdc_tattn_block_x3_sel(const float* x, const float* g_pre, const void* wpk, const float* rot, const float* bias, float* y,
                           int outer, int inner, int C, int ntok, int64_t so, int64_t sc, int64_t st, float eps, int impl, void* stream);
int sdc_tattn_block_x3_impl(int C, int ntok, int inner);

/* ------------------------------------------------------- softmax attention */
/* Attention core (heads x 32): out = softmax(q*scale . k^T + bias) v, optional rotary on q,k.
 * 1D/model/unet.py:247-251 ; conv3d.py:313-353 (focus_present_mask all-False).
 * Sequences are indexed (outer, inner); element (o, c, i, tok) at o*so + c*sc + i*si + tok*st.
 * rot: [ntok][16][2] cos/sin table or null; bias: [heads][ntok][ntok] or null.
 * Two domains.  ntok <= 256: everything above, any strides.  256 < ntok <= 4096: the streaming kernel
 * (csrc/sdc_attn_long.hip) -- rot and bias null, tokens contiguous in qkv and out (q_st == o_st == 1).  Its address
 * arithmetic is 64-bit; the 32-bit quantities are the token index and the grid outer*inner*heads*ceil(ntok/128) (checked
 * per call), so the cap is not an arithmetic limit: 4096 is the largest size held against the fp64 reference.  Anything
 * else past 256 tokens is SDC_EINVAL before any launch.  The kernel is chosen by sdc_attn_route below: by ntok, the strides
 * and the per-sample inner alone, never by outer.  Temporal attention (frame-strided tokens, q_si == o_si == 1) runs on the
 * matrix cores at 32 frames (inner % 8 == 0) and at 64, 96 and 128 frames (any inner >= 1; csrc/sdc_tattn_frames.hip). */
int sdc_attn(const float* qkv, float* out, const float* rot, const float* bias, int outer, int inner, int heads,
             int ntok, int64_t q_so, int64_t q_sc, int64_t q_si, int64_t q_st,
             int64_t o_so, int64_t o_sc, int64_t o_si, int64_t o_st, void* stream);

/* The routing predicate sdc_attn (backward == 0) and sdc_attn_bwd (backward != 0) both dispatch through: host arithmetic on the
 * shape and the strides, no device, no pointer, independent of outer and heads.  has_rot / has_bias: rot / bias non-null;
 * want_dbias: dbias non-null (backward only).  Returns 0 generic kernel, 1 32-frame MFMA, 2 256-token MFMA, 3 streaming
 * (ntok > 256), 4 the 64 / 96 / 128-frame MFMA kernels (frame-strided tokens q_st != 1, q_si == o_si == 1, frame stride x ntok x 4
 * bytes < 2^32 in qkv and out), or SDC_EINVAL with the entry point's own message for a call the entry point refuses.
 * Route 2 is reported for every shape in the 256-token kernel's domain; sdc_attn falls back to route 0 at run time where qkv
 * or its strides are not 16-byte aligned, which is no property of the shape.  The backward has no route 2. */
int sdc_attn_route(int inner, int ntok, int64_t q_si, int64_t q_st, int64_t o_si, int64_t o_st, int has_rot, int has_bias,
                   int want_dbias, int backward);

/* ------------------------------------------------------------ elementwise */
/* kind 0: SiLU, 1: exact (erf) GELU -- time_mlp / ResnetBlock.mlp (unet.py:152-155,310-315) */
int sdc_act(const float* x, float* y, int64_t n, int kind, void* stream);

/* ----------------------------------------------------- fused DDPM update */
/* One reverse step for every element, fused with guidance and the conditioning writes:
 *   x0  = a x - b eps ; eps' = eps + k g(x0) ; x0' = clamp(a x - b eps', -1, 1)
 *   x-  = c1 x0' + c2 x + sigma z ; then re-impose the conditions (unless last step for burgers/tokamak)
 * p_sample / p_mean_variance / model_predictions / q_posterior:
 *   1D/model/diffusion.py:217-306, tokamak/model/diffusion.py:201-266, 2d/ddpm/diffusion_2d.py:242-285;
 * conditioning writes 1D/model/diffusion.py:336-366,380-394, tokamak/...:295-308,330-336, 2d/...:297-301,310-312.
 * coef: [T][8] floats {a, b, c1, c2, sigma(0 at t=0), k(J_scheduler), 0, 0}; t_dev: device timestep.
 * noise: explicit z tensors [n_draw][numel] (parity mode) indexed by *draw_dev, or null -> Philox4x32-10
 * normal draws keyed by (seed, *draw_dev, element).  gscal: per-sample guidance scalars from sdc_guide_reduce.
 */
#define SDC_MODEL_BURGERS 0
#define SDC_MODEL_TOKAMAK 1
#define SDC_MODEL_SMOKE 2

typedef struct SdcStepDesc {
    int32_t model;               /* SDC_MODEL_* */
    int32_t B;
    int32_t d0, d1, d2, d3;      /* per-sample dims: burgers (C,H,W,1) ; tokamak (C,L,1,1) ; smoke (F,C,H,W) */
    int32_t guide;               /* 0 none, 1 built-in closed form, 2 external g tensor */
    int32_t clip;                /* clip_denoised */
    int32_t impose;              /* 1: apply conditioning writes to the output; 2 (smoke): control channels only */
    int32_t cond_idx;            /* burgers: condition_idx (10); tokamak: nt (122) */
    int32_t pad_zero;            /* burgers/tokamak: !train_on_padded_locations */
    int32_t use_max;             /* burgers: 0 mean-mode (use_max_safety=True), 1 amax mode */
    int32_t has_wgt;             /* burgers: w_groundtruth given ; smoke: control given */
    int32_t skip_draws;          /* noise draws consumed per step beyond the one used (calibration branch: 1) */
    int32_t ddim;                /* 1: DDIM update (ddim_sample, 1D/model/diffusion.py:451-555, 2d/...:324-404): x0 always
                                    clipped, guidance on the clipped x0, eps re-derived, coef rows = {a, b, sqrt(a_next), c,
                                    sigma, k, last} indexed by step number */
    uint64_t seed;
} SdcStepDesc;

/* gpar: device float[8] of guidance constants (kept on the device so a captured graph survives a new
 * conformal quantile Q):  burgers {w_score, u_bound^2, Q, 10}; tokamak {w_obj, w_safe, guidance_scaler,
 * safety_threshold, Q}; smoke {w_safe, safe_bound, Q, standard_fixed_ratio}.
 * sdc_guide_reduce: per-sample hinge derivative + arg-extremum of the safety functional evaluated on
 * x0 = a x - b eps (clipped to [-1, 1] when ddim)  -> gscal[4*B] = {active, arg, extremum, 1/ties}
 * (1D/utils/guidance.py:58-77, tokamak/utils/guidance.py:32-56, tokamak/utils/metrics.py:144-151, 2d/inference_2d.py:173-186).
 *   active   = d/ds max(s, 0) at the hinge argument s: 1 for s > 0, 0 for s < 0 and 1/2 at s == 0 exactly (what the
 *              backward of torch.maximum(s, 0) passes at a tie)
 *   arg      = flat per-sample index of the first element attaining the amax / amin (int bits), 0 in the mean modes
 *   extremum = that amax / amin value ; 1/ties = one over the number of elements attaining it (amax / amin backward
 *              splits the gradient evenly between tied elements) */
int sdc_guide_reduce(const SdcStepDesc* d, const float* x, const float* eps, const float* coef, const int32_t* t_dev,
                     const float* gpar, float* gscal, void* stream);
/* guide: 0 none | 1 built-in closed-form gradient (needs gpar, gscal[, target]) | 2 external gradient tensor gext
 * | 3 write x0 = a x - b eps to x0out only (so a caller-supplied nablaJ callable can be evaluated on it). */
int sdc_step_update(const SdcStepDesc* d, const float* x, const float* eps, const float* gext, const float* coef,
                    const int32_t* t_dev, const int32_t* draw_dev, const float* noise, int64_t noise_stride,
                    const float* gpar, const float* gscal, const float* target, const float* c0, const float* c1,
                    const float* c2, float* xout, float* x0out, void* stream);
/* conditioning writes only (initial x_T).  Validates like sdc_step_update with impose set, before any launch: c0 always;
 * c1 unless the model is smoke (SDC_ENULL); the tensor behind has_wgt (burgers/tokamak c2, smoke c1; SDC_ENULL);
 * d->impose == 2 (control channels only) for smoke alone (SDC_EINVAL). */
int sdc_impose(const SdcStepDesc* d, float* x, const float* c0, const float* c1, const float* c2, void* stream);
/* x = N(0,1) from the same Philox stream (draw index *draw_dev), then (*draw_dev)++ handled by sdc_advance */
int sdc_randn(float* x, int64_t n, uint64_t seed, const int32_t* draw_dev, void* stream);
/* *t_dev += dt ; *draw_dev += ddraw   (one thread; keeps the step counter on the device for graph replay) */
int sdc_advance(int32_t* t_dev, int dt, int32_t* draw_dev, int ddraw, void* stream);

/* DDIM: ++*idx_dev ; *t_dev = ttab[*idx_dev] (the strided timestep list lives on the device) ; *draw_dev += ddraw */
int sdc_advance_table(int32_t* idx_dev, int32_t* t_dev, const int32_t* ttab, int32_t* draw_dev, int ddraw, void* stream);

/* ------------------------------------------------------------- conformal */
/* per-sample conformal score |f(pred) - f(truth)| and weight exp(-J(truth)):
 * 1D/inference/conformal.py:68-85 + guidance.py:9-46 ; tokamak/inference/conformal.py:79-109 ;
 * 2d/inference_2d.py:83-92,139-144.  Uses SdcStepDesc for model + constants. */
int sdc_conformal_score(const SdcStepDesc* d, const float* pred, const float* truth, const float* target,
                        const float* gpar, float* score, float* weight, void* stream);

/* --------------------------------------------------- evaluation rollout */
/* Explicit finite-difference Burgers' solver used to score a sampled control:
 * burgers_numeric_solve_free, 1D/data/generate_burgers.py:207-299, called by control_trajectories,
 * 1D/utils/metrics.py:42-65.  u0 (N,s), f (N,Nt,s) -> traj (N,Nt+1,s); `steps` Euler steps of size dt, the force row
 * advances and a snapshot is recorded every `record_every` steps; coef_transport = 1/(2 dx), d0..d2 = visc*[1,-2,1]/dx^2
 * (all rounded to fp32 by the caller exactly as the reference's FloatTensor(...) does).
 * Step counts the reference's loop fails on are defined here: when record_every does not divide `steps` into Nt intervals, the
 * steps past Nt * record_every run with zero force and at most Nt snapshots are recorded (rows never recorded stay unwritten);
 * record_every <= 0 (the reference's steps < Nt, a modulo by zero) is SDC_EINVAL.  s > 8190 (two (s+2)-float rows exceed 64 KiB
 * of LDS) is SDC_EINVAL.  All checks come before any launch.  The Python drop-in solvers.burgers_numeric_solve_free does not
 * rely on the guards: it raises the reference's IndexError / ZeroDivisionError for those step counts before calling this. */
int sdc_burgers_rollout(const float* u0, const float* f, float* traj, int N, int s, int Nt, int steps, int record_every,
                        float dt, float coef_transport, float d0, float d1, float d2, void* stream);

/* ------------------------------------------------- backward (fine-tuning path) */
/* The VJP kernels of the fine-tuning loss: p_losses + loss.backward() through the U-Nets,
 * 1D/model/diffusion.py:638-733, 2d/ddpm/diffusion_2d.py:434-452 (callers 1D/inference/inference_ft.py:183-187,
 * tokamak/inference/pipeline.py:238-263, 2d/inference_2d.py:267-279).  Conv DATA gradients have no entry point of their
 * own: they are convolutions with flipped / transposed taps and run on sdc_conv with re-packed weights. */

/* Weight (and bias) gradient of nn.Conv1d/2d/3d, nn.Linear and nn.ConvTranspose3d:
 *   dw[m][n][kd][kh][kw] = sum_{b, od, oh, ow} G[b][m][od][oh][ow] * X[b][n][(od sD - pD + kd) / uD][...][(ow sW - pW + kw) / uW]
 * (terms outside X are zero; uD/uH/uW in {1,2} = nearest upsampling of X folded into the read, nn.Upsample + conv).
 * For a conv  y = conv(x, w): G = dL/dy (M = Cout), X = x (N = Cin) -> dw in nn.Conv layout (Cout, Cin, k...).
 * For a transposed conv y = convT(x, w): G = x (M = Cin), X = dL/dy (N = Cout), s/p of the layer -> nn.ConvTranspose layout.
 * dbias[m] = sum G[b][m][...] or null.  (kW, sW) in {(1,1),(3,1),(7,1),(4,2),(2,2)}; rows are walked in chunks of 16 positions.
 * fp32 MFMA; the positions are split over workgroups and summed in a fixed order (deterministic). */
typedef struct SdcWgradDesc {
    int32_t B, M, N;
    int32_t oD, oH, oW;          /* positions of G */
    int32_t iD, iH, iW;          /* stored size of X */
    int32_t kD, kH, kW;
    int32_t sD, sH, sW;
    int32_t pD, pH, pW;
    int32_t uD, uH, uW;
    int32_t precision;           /* sdc_conv_wgrad: unread (0); sdc_conv_wgrad_f16: 6 or 7, below */
    int64_t gs[5], xs[5];        /* element strides (b, c, d, h, w) of G and X */
} SdcWgradDesc;
size_t sdc_conv_wgrad_bytes(const SdcWgradDesc* d);
int sdc_conv_wgrad(const SdcWgradDesc* d, const float* g, const float* x, float* dw, float* dbias, void* work,
                   size_t work_bytes, void* stream);

/* Fine-tuning with fp16 operands (net.train_precision 6 / 7, opt-in).  For the stride-1 pad-1 3-tap convs
 * (1x1x3, 1x3x3, 3x3x3) the three directions run on the fp16 matrix pipe with fp32 accumulation:
 *   forward         sdc_conv at SdcConvDesc.precision 6 / 7 on a precision-8 buffer (below), as the samplers do;
 *   data gradient   sdc_conv_dgrad_f16 on the precision-8 buffer of the data-gradient weight (flip = 1);
 *   weight gradient sdc_conv_wgrad_f16.
 * The loss gradient G of a conv (per-element ~1e-7 for a mean loss: below fp16's normal range) is scaled per tensor by 2^e before it
 * is rounded and the results by 2^-e (both exact); e is computed on the device, so a step stays capturable and never syncs.
 *
 * sdc_f16_grad_exponent: e[0] = e such that max|G| 2^e lies in [2^14, 2^15), 0 when max|G| is 0 or not finite (inf / NaN then
 * reach dx / dw unchanged), clamped to [-126, 126].  G is (B, C, D, H, W) through strides[5] (elements); e holds SDC_F16_EXP_INTS
 * int32 of device memory (e[1 ...]: scratch).  Two launches. */
#define SDC_F16_EXP_INTS 1025
int sdc_f16_grad_exponent(const float* g, int B, int C, int D, int H, int W, const int64_t* strides, int32_t* e, void* stream);

/* Data gradient dx = conv(g, flipped w): the descriptor of that conv (Cin0 = channels of g, Cout = channels of dx, pad k - 1 - p),
 * precision 6 (dispatch table of sdc_conv) or 7 (every covered conv), wp a precision-8 flip = 1 buffer.  Where sdc_conv would run
 * conv_f16_kernel, g is multiplied by 2^e[0] as it is rounded and the accumulators by 2^-e[0]; elsewhere exactly sdc_conv (e unread). */
int sdc_conv_dgrad_f16(const SdcConvDesc* d, const float* g, const float* wp, const int32_t* e, float* dx, void* stream);

/* Weight gradient of sdc_conv_wgrad with fp16 operands: dw = 2^-e sum fp16(2^e G) fp16(X), fp32 accumulation, positions split over
 * workgroups and summed in a fixed order (deterministic, no atomics); dbias = fp32 sum of the unscaled G (fixed order).  d.precision
 * 6: wgrad_f16_kernel where its measured dispatch table (csrc/sdc_wgrad_f16.hip wf_faster, keyed on per-sample sizes) has it ahead
 * of sdc_conv_wgrad; 7: every covered descriptor (1x1x3 / 1x3x3 / 3x3x3 taps, stride 1, pad 1, rows of 16 / 32 / 64 / 128 positions,
 * whole rows per 128-position stage).  Other descriptors: exactly sdc_conv_wgrad (e unread).  work: sdc_conv_wgrad_f16_bytes(d)
 * bytes.  sdc_conv_wgrad_describe names the kernel a descriptor runs (host only, launches nothing). */
size_t sdc_conv_wgrad_f16_bytes(const SdcWgradDesc* d);
int sdc_conv_wgrad_f16(const SdcWgradDesc* d, const float* g, const float* x, const int32_t* e, float* dw, float* dbias, void* work,
                       size_t work_bytes, void* stream);
int sdc_conv_wgrad_describe(const SdcWgradDesc* d, char* name, size_t cap);

/* The 7-tap stem convs with fp16 operands and fp32 accumulation (net.stem_f16, opt-in, samplers only; DESIGN.md section 13;
 * csrc/sdc_conv_stem_f16.hip).  A switch of its own beside SdcConvDesc.precision: sdc_conv, its dispatch and every layout above are
 * untouched; the caller asks sdc_conv_stem_f16_ok and, where it says 1, calls sdc_conv_stem_f16 on the stem's own fp16 buffer.
 *
 * sdc_conv_stem_f16_ok: 1 when conv_stem_f16_kernel covers the descriptor, else 0.  Host only, launches nothing, reads the
 * descriptor alone and never keys on B (a sample's bits do not depend on its batch).  Covered: kW = 7 with (kD, kH) = (1, 1), (1, 7)
 * or (7, 7); stride 1, no upsampling; pad 3 along every 7-tap axis and 0 along every 1-tap axis, output size = input size;
 * Cin0 <= 8, Cin1 = 0; Cout % 64 == 0; rows of oW = 16, 32, 64 or 128 columns; dense input and output rows (x0s[4] == ys[4] == 1, every
 * other stride free).  d->precision, d->x1s and d->rs are unread: no second input, no fused residual.
 *
 * Buffer layout (sdc_pack_stem_f16_bytes(...) bytes, 16-byte aligned; 0 for other taps or Cin > 8).  With NS = ceil(7 kH / 2):
 *     Wh[kd][s][co][8 h + ci] = (fp16, RNE) w[co][ci][kd][kh][kw],   kh * 7 + kw = 2 s + h,   kd < kD, s < NS, h < 2, ci < 8,
 * zero for ci >= Cin and for the one tap 2 s + h = 7 kH past the end: a 16-deep MFMA step s covers two adjacent taps of the
 * (kh, kw) walk, eight channels each (kD * NS * Cout * 16 halves: 350 KB for the smoke stem, Cout 64).
 * sdc_pack_stem_f16 writes it on the device from the nn.Conv weight w (Cout, Cin, kD, kH, kW), one launch on `stream`.
 *
 * sdc_conv_stem_f16: y = conv(x, w) + bias (bias may be null), asynchronous on `stream`.  SDC_ENULL for a null d, x, wh or y and
 * SDC_EINVAL (with a message) for a descriptor sdc_conv_stem_f16_ok rejects, both before any launch; SDC_EALIGN for a misaligned wh.
 * Rounding: fp16 x fp16 products are exact in fp32, so the result is an fp64 conv of the rounded operands up to fp32 summation
 * order.  Fixed k order, no K split, no atomics: deterministic. */
int sdc_conv_stem_f16_ok(const SdcConvDesc* d);
size_t sdc_pack_stem_f16_bytes(int Cout, int Cin, int kD, int kH, int kW);
int sdc_pack_stem_f16(const float* w, void* out, int Cout, int Cin, int kD, int kH, int kW, void* stream);
int sdc_conv_stem_f16(const SdcConvDesc* d, const float* x, const void* wh, const float* bias, float* y, void* stream);

/* The same stem convs as exact three-way bf16 operand splits on the bf16 matrix pipe (net.stem_split, the nets' default at precision
 * >= 4, samplers only; csrc/sdc_conv_stem_x3.hip): fp32 inputs, fp32 accumulation, fp32 outputs.  Every fp32
 * operand is the exact sum of three bf16 pieces, x = h + m + l with h = bf16(x), m = bf16(x - h), l = bf16(x - h - m) (RNE), and a
 * product is formed as a3 b1 + a2 b2 + a1 b3 + a2 b1 + a1 b2 + a1 b1 (a = weight, b = activation; six v_mfma_f32_32x32x16_bf16, smallest
 * terms first); the three dropped terms are below 2^-24 |a b|, half an ulp of the product.  An fp32-grade result in another rounding
 * order, not a reduced precision.  Like stem_f16 a switch of its own beside SdcConvDesc.precision: sdc_conv, its dispatch and every
 * layout above are untouched; the caller asks sdc_conv_stem_x3_ok and, where it says 1, calls sdc_conv_stem_x3 on the stem's own buffer.
 *
 * sdc_conv_stem_x3_ok: 1 where the caller should route the stem here: the predicate of sdc_conv_stem_f16_ok (one function) less the
 * shapes that did not measure faster than sdc_conv -- the kD = 1 stems (1x1x7 and 1x7x7 taps), so today kD = kH = kW = 7 only.
 * sdc_conv_stem_x3 itself accepts every descriptor of sdc_conv_stem_f16_ok (SDC_EINVAL for the others).
 *
 * Buffer layout (sdc_pack_stem_x3_bytes(...) = 3 * sdc_pack_stem_f16_bytes(...) bytes, 16-byte aligned): three planes
 *     Wb[piece][kd][s][co][8 h + ci],   piece = 0 (h), 1 (m), 2 (l) of w[co][ci][kd][kh][kw],   kh * 7 + kw = 2 s + h,
 * each with the layout of Wh above in bf16, zeros where Wh has zeros; the three planes sum to the fp32 weight bit for bit.
 * sdc_pack_stem_x3 writes it on the device, one launch on `stream`.
 *
 * sdc_conv_stem_x3: y = conv(x, w) + bias (bias may be null), asynchronous on `stream`; errors as sdc_conv_stem_f16.  The activations
 * are split as they are staged.  Fixed k order, no K split, no atomics: deterministic, and a sample's bits do not depend on its batch.
 * Scaling x by a power of two scales y - bias exactly (short of overflow / underflow).  Non-finite inputs: the residuals of an
 * infinite x are inf - inf = NaN, so y is NaN where sdc_conv gives an infinity. */
int sdc_conv_stem_x3_ok(const SdcConvDesc* d);
size_t sdc_pack_stem_x3_bytes(int Cout, int Cin, int kD, int kH, int kW);
int sdc_pack_stem_x3(const float* w, void* out, int Cout, int Cin, int kD, int kH, int kW, void* stream);
int sdc_conv_stem_x3(const SdcConvDesc* d, const float* x, const void* wb, const float* bias, float* y, void* stream);

/* The strided (1,4,4)/(1,2,2) convs, the 1x2x2 sub-pixel convs of the transposed convs and the 1x1x1 convs as exact three-way bf16 operand
 * splits on the bf16 matrix pipe (net.gemm_split, default on at precision >= 4, samplers only; DESIGN.md section 15;
 * csrc/sdc_conv_gemm_x3.hip): the arithmetic of sdc_conv_stem_x3 -- fp32 inputs, fp32 accumulation, fp32 outputs, six
 * v_mfma_f32_32x32x16_bf16 per product, fixed k order, no K split, no atomics.  A switch of its own beside SdcConvDesc.precision:
 * sdc_conv, its dispatch and every layout above are untouched; the caller asks sdc_conv_gemm_x3_ok and, where it says 1, calls
 * sdc_conv_gemm_x3 on the conv's own buffer.
 *
 * Covered: kD = 1, one input tensor (Cin1 == 0), no residual (rs all zero), no upsampling, Cout % 64 == 0, rows of 16 / 32 / 64 / 128
 * output columns, and one of
 *   taps (1,4,4), stride (1,2,2), pad (0,1,1), input twice the output along H and W, Cin % 16 == 0;
 *   taps (1,2,2), stride 1, pad (0, pH, pW) with pH, pW in {0, 1}, output size = input size, Cin % 32 == 0 (y is usually a parity view
 *     y[:, :, :, 1 - pH :: 2, 1 - pW :: 2] of a transposed conv's output: every stride of y is free);
 *   taps 1x1x1, stride 1, Cin % 64 == 0;
 * with a tile's input rows within 160 KB of LDS.  There is no form with a second input, a residual, GroupNorm sums or upsampling.
 *
 * sdc_conv_gemm_x3_ok: 1 where the caller should route the conv here: covered AND measured faster than sdc_conv at precision 4 on the
 * same buffers (the table in csrc/sdc_conv_gemm_x3.hip).  Host only, launches nothing, reads the descriptor only, keyed on per-sample
 * sizes and never on B: a sample's bits do not depend on its batch.  sdc_conv_gemm_x3 itself accepts every covered descriptor
 * (tests, measurement) and returns SDC_EINVAL for the others.
 *
 * Buffer layout (sdc_pack_gemm_x3_bytes(Cout, Cin, kH, kW) = 3 * kH * kW * Cin * Cout * 2 bytes, 16-byte aligned; 0 for other taps or
 * channel counts): three bf16 planes, the exact split h = bf16(w), m = bf16(w - h), l = bf16(w - h - m) (RNE), each
 * Wb[m tile = co / 64][stage][step = block * taps + tap][co % 64][ci % 16] with ci = (stage * NCB + block) * 16 + ci % 16 and
 * NCB = 1 (4x4 taps), 2 (2x2) or 4 (1x1) channel blocks of 16 per stage: the steps of a stage are one contiguous run per tile.
 * sdc_pack_gemm_x3 writes it on the device, one launch on `stream`, from the conv's Wp[tap * Cin + ci][co] (the precision-0 layout of
 * sdc_conv; for a sub-pixel conv the merged sub-filter of its parity).
 *
 * sdc_conv_gemm_x3: y = conv(x, w) + bias (bias may be null), asynchronous on `stream`.  SDC_ENULL for a null d, x, wb or y,
 * SDC_EINVAL for a descriptor that is not covered, both before any launch; SDC_EALIGN for a misaligned wb. */
int sdc_conv_gemm_x3_ok(const SdcConvDesc* d);
size_t sdc_pack_gemm_x3_bytes(int Cout, int Cin, int kH, int kW);
int sdc_pack_gemm_x3(const float* wp, void* out, int Cout, int Cin, int kH, int kW, void* stream);
int sdc_conv_gemm_x3(const SdcConvDesc* d, const float* x, const void* wb, const float* bias, float* y, void* stream);

/* The 1x1x1 stride-1 convs over a dense layout as exact three-way bf16 operand splits with the weights resident in LDS (DESIGN.md
 * section 23; csrc/sdc_conv_pw_x3.hip): the arithmetic of sdc_conv_stem_x3 and sdc_conv_gemm_x3 -- fp32 inputs, fp32 accumulation, fp32
 * outputs, six v_mfma_f32_32x32x16_bf16 per product, the five small terms in accumulators of their own, fixed k order, no K split, no
 * atomics.  NOT a switch and no buffer of its own: wp is the conv's ordinary packed Wp[ci][co] (any precision's buffer starts with it),
 * split by every workgroup as it starts.  sdc_conv itself takes this kernel for the shapes sdc_conv_pw_x3_ok lists (route(), after the
 * split-K decision) at precision 0 and >= 4; at precision 2 and 3 it keeps the literal fp32 kernels.  A 1x1x1 conv has one weight
 * layout, and every plan records it with the lowest layout code, precision 0, whatever the plan's own precision: 0 cannot be told from
 * 4 in such a descriptor, so the listed per-sample shapes run here wherever sdc_conv is called on them -- sampler plans of every
 * precision, forward_train's forward --: fp32-grade arithmetic in another rounding order, like the Winograd modes.
 *
 * Covered: 1x1x1 taps, stride 1, no padding or upsampling, output size = input size; positions of a sample contiguous in x0, x1, y and
 * the residual (strides (., ., H W, W, 1)), D H W a multiple of 4 and at least 128; sample and channel strides multiples of 4, every
 * pointer 16-byte aligned; Cin0 and Cin1 multiples of 16 with Cin0 + Cin1 a multiple of 32 from 64 on; Cout a multiple of 64 or 96; and
 * the three bf16 images of a block of output channels -- the widest of 128, 96 and 64 that divides Cout -- within 160 KB of LDS:
 * Cin0 + Cin1 <= 256 (128 for the 128-wide block).  Optional second
 * channel-concatenated input, bias and residual: y = (conv(x0 | x1, w) + bias) + residual.
 *
 * sdc_conv_pw_x3_ok: 1 where sdc_conv routes the conv here: covered AND measured faster than the fp32 kernel on the same buffers (the
 * table in csrc/sdc_conv.hip).  Host only, launches nothing, reads the descriptor only (16-byte aligned operands assumed, a residual
 * where rs[1] != 0), keyed on Cin0, Cin1, Cout and the per-sample volume and never on B: a sample's bits do not depend on its batch.
 * sdc_conv_pw_x3: the direct launch for every covered descriptor, listed or not (tests, measurement), asynchronous on `stream`, nothing
 * allocated.  SDC_ENULL for a null d, x0, wp or y, SDC_EINVAL for a descriptor or operands outside the coverage, both before any
 * launch. */
int sdc_conv_pw_x3_ok(const SdcConvDesc* d);
int sdc_conv_pw_x3(const SdcConvDesc* d, const float* x0, const float* x1, const float* wp, const float* bias, const float* residual,
                   float* y, void* stream);

/* The 3x3x3 stride-1 convs over rows of 16 as Winograd F(2x2x2,3x3x3) with the Cin products formed from exact three-way bf16 operand
 * splits on the bf16 matrix pipe (net.wino_split, samplers only; csrc/sdc_conv_wino_x3.hip): precision 4's
 * algorithm -- the same transforms, passes, folds into the plane pair, bias and GroupNorm epilogue -- with the arithmetic of
 * sdc_conv_stem_x3: fp32 inputs, fp32 accumulation, fp32 outputs, six v_mfma_f32_32x32x16_bf16 per product (smallest terms first, one
 * accumulator), fixed k order, no K split, no atomics.  The operands that are split are the transformed ones: V = B^T d B comes out of
 * the fp32 transform with precision 4's bits and is split as it is staged; U3 is split at pack time.  A switch of its own beside
 * SdcConvDesc.precision (which these entry points do not read): sdc_conv, its dispatch and every layout above are untouched.
 *
 * Covered: what conv_wg3_kernel takes at precision 4 -- 3x3x3 taps, stride 1, pad 1, no upsampling, output size = input size, an even
 * depth, oH % 16 == 0, Cout % 64 == 0, contiguous input rows, 8-byte aligned rows of y, no residual (rs all zero), one or two
 * (channel-concatenated) inputs -- with oW == 16 and Cin0 % 16 == 0 and Cin1 % 16 == 0.
 *
 * sdc_conv_wino3_x3_ok: 1 where the caller should route the conv here: covered AND measured faster than sdc_conv at precision 4 on the
 * same buffers (the table in csrc/sdc_conv_wino_x3.hip).  Host only, launches nothing, reads the descriptor only, keyed on per-sample
 * sizes and never on B.  sdc_conv_wino3_x3 itself accepts every covered descriptor (tests, measurement) and returns SDC_EINVAL for the
 * others.
 *
 * Buffer layout (sdc_pack_wino3_x3_bytes(Cout, Cin) = 3 * 64 * Cin * Cout * 2 bytes, Cin = Cin0 + Cin1, 16-byte aligned; 0 unless
 * Cout % 64 == 0 and Cin % 16 == 0): three bf16 planes, the exact split h = bf16(u), m = bf16(u - h), l = bf16(u - h - m) (RNE) of
 * u = U3[jd][ci][co][j * 4 + xi], each Wb[co / 64][jd][stage = ci / 16][j][xi][co % 64][(ci % 16) ^ 8 ((co >> 3) & 1)]: the four
 * components of a transformed row j of a stage are one contiguous run of 8 KB per plane, and the two channel octets of a row swap
 * places in rows 8-15 of every 16 (the kernel's fragment reads then cover all LDS banks).  sdc_pack_wino3_x3 writes it on the device, one launch on `stream`, from
 * the conv's precision-4 buffer wp (sdc_pack_conv_weight at precision 4; U3 is its last part).
 *
 * sdc_conv_wino3_x3: y = conv(cat(x, x1), w) + bias (x1, bias may be null), asynchronous on `stream`; y is scratch while the kernel
 * runs.  gn_parts non-null: the GroupNorm partial sums of sdc_conv_gn for gn_groups groups -- the same table, sized with
 * sdc_conv_gnparts of the conv at precision 4 -- are written as well; SDC_EINVAL where that says 0.  SDC_ENULL for a null d, x, wb or y
 * (or x1 with Cin1 > 0), SDC_EINVAL for a descriptor that is not covered, both before any launch; SDC_EALIGN for a wb that is not
 * 16-byte aligned or an x, x1 or y that is not 8-byte aligned.  Non-finite inputs: the residuals of the split of an infinite value are
 * inf - inf = NaN, and a plane or row that is clipped away enters as 0 * x: y is NaN where sdc_conv gives an infinity. */
int sdc_conv_wino3_x3_ok(const SdcConvDesc* d);
size_t sdc_pack_wino3_x3_bytes(int Cout, int Cin);
int sdc_pack_wino3_x3(const float* wp, void* out, int Cout, int Cin, void* stream);
int sdc_conv_wino3_x3(const SdcConvDesc* d, const float* x, const float* x1, const void* wb, const float* bias, float* y,
                      double* gn_parts, int gn_groups, void* stream);

/* Backward of sdc_gn_apply (GroupNorm -> (scale+1, shift) -> SiLU; Block, conv3d.py:189-204, 1D/model/unet.py:128-147):
 * h = the conv output the forward normalised (contiguous (B,C,S)), stats from the forward, ss = per-sample rows
 * [scale (C) | shift (C)] at ss + b*ss_b_stride or null.  rows: sdc_gn_silu_bwd_floats(B, C, G, S) floats, 8-byte aligned.  Writes
 * gh = dL/dh and rows[b][c] = (A1, A2) with
 * A1 = sum_S gy silu'(v), A2 = sum_S gy silu'(v) xhat, and -- when dgamma / dbeta (C floats each) are given --
 * dgamma[c] = sum_b (1+scale) A2, dbeta[c] = sum_b (1+scale) A1 and, when dss (contiguous (B, 2C)) is given too,
 * dss[b] = [gamma A2 + beta A1 | A1], the gradient of the ss rows.  (The residual the forward added passes gy through.) */
size_t sdc_gn_silu_bwd_floats(int B, int C, int G, int64_t S);
int sdc_gn_silu_bwd(const float* h, const float* gy, const float* stats, const float* gamma, const float* beta,
                    const float* ss, int64_t ss_b_stride, float* rows, float* gh, float* dgamma, float* dbeta, float* dss,
                    int B, int C, int G, int64_t S, void* stream);

/* Backward of sdc_chan_norm (mode 0 channel LayerNorm, 1 RMSNorm): gx, and partial sums of the gain gradient.
 * gpart = sdc_chan_norm_bwd_bytes(B, C, S) bytes of scratch: [C][sdc_chan_norm_bwd_parts(B, S)] partials (the caller sums the
 * last axis) followed by the kernel's per-position (mean, scale) table. */
size_t sdc_chan_norm_bwd_parts(int B, int64_t S);
size_t sdc_chan_norm_bwd_bytes(int B, int C, int64_t S);
int sdc_chan_norm_bwd(const float* x, const float* gy, const float* g, float* gx, float* gpart, int B, int C, int64_t S,
                      int mode, float eps, void* stream);

/* Kernel layout of an nn.Conv weight w (Cout, Cin, kD, kH, kW) for SdcConvDesc.precision (0, 2 ... 7) in one launch: Wp followed
 * by the Winograd taps the precision / tap shape call for (layouts: SdcConvDesc.precision above), transformed taps summed in fp64
 * and rounded once.  flip != 0 packs the DATA-GRADIENT weight of the same conv instead (channels transposed, taps flipped; then the
 * arguments Cout / Cin are those of the packed weight, i.e. swapped; not with precision 6 / 7, whose fp16 tail -- a second launch,
 * RNE -- only the samplers read).  precision 8 = the fine-tuning layout of precisions 6 / 7: precision 6's buffer (the precision-4
 * sections, then for the 1x1x3 / 1x3x3 / 3x3x3 taps the fp16 tail) written by the one launch, flip allowed (the tail then holds the
 * flipped, transposed taps); sdc_conv reads it with SdcConvDesc.precision 6 or 7.  out holds sdc_pack_conv_weight_floats(...) floats. */
size_t sdc_pack_conv_weight_floats(int Cout, int Cin, int kD, int kH, int kW, int precision);
int sdc_pack_conv_weight(const float* w, float* out, int Cout, int Cin, int kD, int kH, int kW, int precision, int flip, void* stream);

/* The same packing for MANY weights in one launch (a fine-tuning step re-packs every conv of the net, twice: forward and
 * data-gradient form -- reference callers 1D/inference/inference_ft.py:183-226, 2d/inference_2d.py:267-279 step the optimiser
 * between forwards).  The caller fills w, out, Cout, Cin, kD, kH, kW, precision, flip of every item (meaning as in
 * sdc_pack_conv_weight; out holds sdc_pack_conv_weight_floats(...) floats); sdc_pack_batch_plan (host only, no GPU call)
 * fills the remaining fields and returns the launch size; the caller copies the table to device memory once and calls
 * sdc_pack_batch_run(table_dev, ...) whenever the weights changed.  Results are those of sdc_pack_conv_weight bit for bit.
 * Precisions 0, 2 ... 5 and the fine-tuning layout 8 (the sampler-only 6 / 7: SDC_EINVAL). */
typedef struct SdcPackItem {
    const float* w;
    float* out;
    int Cout, Cin, kD, kH, kW, precision, flip;
    int co_sh, ci_sh, grid_x, grid_y, block0;     /* filled by sdc_pack_batch_plan */
    unsigned tap_magic;
    int64_t n[5];
} SdcPackItem;
int sdc_pack_batch_plan(SdcPackItem* items, int n, int* total_blocks, int* lds_bytes);
int sdc_pack_batch_run(const SdcPackItem* items_dev, int n, int total_blocks, int lds_bytes, void* stream);

/* Backward of the attention cores (same tensor conventions as sdc_attn / sdc_linattn: q, k, v = channel ranges of qkv, the
 * gradients dqkv in the same layout; dout = dL/dout in the layout of `out`).
 * sdc_attn_bwd: dbias (heads, ntok, ntok) = sum over sequences of dS, or null.  The bias gradient is built for ntok <= 32 and for
 * route 4 of sdc_attn_route (64, 96 or 128 frames with contiguous pixels): the temporal attention's relative-position bias,
 * conv3d.py:74-112; anywhere else a non-null dbias is SDC_EINVAL before any launch.  work = sdc_attn_bwd_bytes(...) bytes when
 * dbias is requested, and only then: it holds one partial table per workgroup slot, summed in a fixed order (no atomics).
 * sdc_attn_bwd_bytes: 1024 slots x heads x ntok^2 floats, except at ntok 64 / 96 / 128: 256 slots (67 MB instead of 268 MB at
 * 128 frames and 4 heads).
 * 256 < ntok <= 4096 (the domain of sdc_attn above, dbias null): work is REQUIRED -- two floats per (sequence, head, token),
 * the row statistics the gradient recomputes the probabilities from; nothing ntok x ntok is stored, no atomics. */
size_t sdc_attn_bwd_bytes(int outer, int inner, int heads, int ntok);
int sdc_attn_bwd(const float* qkv, const float* dout, const float* rot, const float* bias, float* dqkv, float* dbias, void* work,
                 int outer, int inner, int heads, int ntok, int64_t q_so, int64_t q_sc, int64_t q_si, int64_t q_st,
                 int64_t o_so, int64_t o_sc, int64_t o_si, int64_t o_st, void* stream);

/* Backward of sdc_tattn_block for fine-tuning (net.train_fuse_attn; csrc/sdc_tablock_bwd.hip): from x and dy
 * alone -- xn, q/k/v, P, O and every gradient of an intermediate are recomputed on chip, nothing full-size is written but dx.
 * x, g_pre, wqkv (packed [64][384]), wo (packed [128][64]), rot, bias, the strides and the supported domain (C = 64, 32 frames,
 * inner a multiple of 8, one outer index below 4 GB) are sdc_tattn_block's; dy and dx are addressed as x.
 *   dx    = dy + J^T dy (the residual branch included)        dg [64]
 *   dwqkv, dwo: the layouts of wqkv and wo                     dbias [4][32][32]: required exactly when bias is given, ignored otherwise
 * Outputs are overwritten, not accumulated.  dx must not alias x or dy (x is read again after dx of a neighbouring tile is written).
 * work = sdc_tattn_block_bwd_bytes(outer, inner) bytes: one table of parameter-gradient partial sums per workgroup, summed in a
 * fixed order (deterministic, no atomics); its content before the call does not matter.  The size is an upper bound that needs no
 * device query and stops growing at 256 pixel groups.
 * Checked before any launch or device query: SDC_ENULL for a null x, g_pre, wqkv, wo, dy, dx, dg, dwqkv, dwo or work, and for bias
 * without dbias; SDC_EINVAL for an unsupported shape, a wqkv / wo not 16-byte or a rot not 8-byte aligned. */
size_t sdc_tattn_block_bwd_bytes(int outer, int inner);
int sdc_tattn_block_bwd(const float* x, const float* g_pre, const float* wqkv, const float* wo, const float* rot, const float* bias,
                        const float* dy, float* dx, float* dg, float* dwqkv, float* dwo, float* dbias, void* work,
                        int outer, int inner, int C, int ntok, int64_t so, int64_t sc, int64_t st, float eps, void* stream);

/* Backward of sdc_linattn_block_sel(..., impl = 0) for fine-tuning (net.train_fuse_linattn; DESIGN.md section 25;
 * csrc/sdc_lablock_bwd.hip), SpatialLinearAttention form only: pre_mode 0 (channel LayerNorm), post_mode -1 (no post norm).  From x
 * and dy alone -- xn, Q, K, the two softmaxes, dQ, dK and dxn are recomputed tile by tile on chip (V is never formed per token);
 * nothing of size C x tokens is written but dx.  x, g_pre, wqkv (packed [C][384]), wo (packed [128][C]), the strides and the domain
 * (C in {64, 128}, n % 64 == 0, outer * inner < 65536, sc < 2^27) are sdc_linattn_block's; dy and dx are addressed as x.
 *   dx    = dy + J^T dy (the residual branch included)        dg [C]
 *   dwqkv, dwo: the layouts of wqkv and wo                     dbo [C]: required exactly when bo is given, not written otherwise
 *                                                              (bo is only tested for null)
 * Outputs are overwritten, not accumulated.  dx must not alias x or dy (x and dy are read twice).
 * work = sdc_linattn_block_bwd_bytes(outer, inner, C, n) bytes; its content before the call does not matter.  It holds the small
 * per-sequence tables and the parameter-gradient partial sums of S = min(128, 256 / splits) sequence slots (splits = 1 .. 8, a
 * function of n): sequences are worked in chunks of at most S and the chunks' tables are added in a fixed order (deterministic, no
 * atomics; the token splits depend on n only, so a sequence's dx does not depend on what shares the call).  The size needs no
 * device query and stops growing at outer * inner = S; it is at most 256 (514 C + 256) + 128 (768 C + 4480) + 256 C floats (62 MB at
 * C = 64, 121 MB at C = 128).
 * Checked before any launch or device query, each with its own message: SDC_ENULL for a null x, g_pre, wqkv, wo, dy, dx, dg, dwqkv,
 * dwo or work, and for bo without dbo; SDC_EINVAL for a norm mode other than (0, -1), C not in {64, 128}, n % 64 != 0,
 * outer * inner >= 65536, sc >= 2^27, a wqkv / wo not 16-byte aligned, or dx aliasing x or dy. */
size_t sdc_linattn_block_bwd_bytes(int outer, int inner, int C, int64_t n);
int sdc_linattn_block_bwd(const float* x, const float* g_pre, const float* wqkv, const float* wo, const float* bo, const float* dy,
                          float* dx, float* dg, float* dwqkv, float* dwo, float* dbo, void* work, int outer, int inner, int C,
                          int64_t n, int64_t so, int64_t sc, int64_t si, int pre_mode, int post_mode, float eps, void* stream);

/* The same for the post-norm form of the 1-D nets (LinearAttention of Unet2D / Unet1D): the backward of
 * sdc_linattn_block_sel(..., impl = 0) with pre_mode in {0, 1} and post_mode in {0, 1} (0 channel LayerNorm, 1 RMSNorm; all four
 * combinations),
 *   y = x + N_post(Wo LA(N_pre(x)) + bo) g_post.
 * Arguments, addressing, domain and contract are sdc_linattn_block_bwd's, plus g_post [C] and dg_post [C] (always required).  The
 * post norm's backward turns every dy tile into dz = dL/d(Wo LA + bo) in the first sweep, which leaves it in dx's memory at the
 * tile's own address; the second sweep reads it there before it overwrites the tile with dx (one owner per tile) -- still nothing
 * of size C x tokens is written but dx.  At RMSNorm's clamp (||.|| <= 1e-12) the gradients are sdc_chan_norm_bwd's.
 * work = sdc_linattn_block_post_bwd_bytes(outer, inner, C, n) bytes: sdc_linattn_block_bwd's tables plus T with its channel axis
 * contiguous and the dg_post partials per sequence slot; no device query, stops growing at outer * inner = S; at most
 * 256 (515 C + 256) + 128 (896 C + 4480) + 256 C floats (66 MB at C = 64, 129 MB at C = 128).
 * Checked before any launch or device query, each with its own message: SDC_ENULL for a null x, g_pre, wqkv, wo, g_post, dy, dx,
 * dg_pre, dwqkv, dwo, dg_post or work, and for bo without dbo; SDC_EINVAL for pre_mode not in {0, 1}, post_mode not in {0, 1}
 * (-1 is sdc_linattn_block_bwd's form and the message says so), C not in {64, 128}, n % 64 != 0, outer * inner >= 65536,
 * sc >= 2^27, wqkv or wo not 16-byte aligned, dx aliasing x or dy. */
size_t sdc_linattn_block_post_bwd_bytes(int outer, int inner, int C, int64_t n);
int sdc_linattn_block_post_bwd(const float* x, const float* g_pre, const float* wqkv, const float* wo, const float* bo,
                               const float* g_post, const float* dy,
                               float* dx, float* dg_pre, float* dwqkv, float* dwo, float* dbo, float* dg_post, void* work,
                               int outer, int inner, int C, int64_t n, int64_t so, int64_t sc, int64_t si,
                               int pre_mode, int post_mode, float eps, void* stream);
size_t sdc_linattn_bwd_bytes(int outer, int inner, int heads, int64_t n);      /* scratch of sdc_linattn_bwd */
int sdc_linattn_bwd(const float* qkv, const float* dout, float* dqkv, void* work, int outer, int inner, int heads, int64_t n,
                    int64_t q_so, int64_t q_sc, int64_t q_si, int64_t o_so, int64_t o_sc, int64_t o_si, void* stream);

/* gx = gy * f'(x): kind 0 SiLU, 1 GELU (exact erf) -- time_mlp, 1D/model/unet.py:300-305 */
int sdc_act_bwd(const float* x, const float* gy, float* gx, int64_t n, int kind, void* stream);

/* VJP of nearest-neighbour upsampling by (fh, fw) in {1,2}^2 over the last two axes: gx (rows,H,W) from g (rows,H*fh,W*fw) */
int sdc_sumpool2(const float* g, float* gx, int64_t rows, int H, int W, int fh, int fw, void* stream);

/* ------------------------------------------------- nn.Linear over a batch of rows (fine-tuning path) */
/* The time MLP and the ResnetBlocks' scale/shift MLPs (1D/model/unet.py:300-305, :158-162; tokamak/model/unet.py likewise;
 * 2d/video_diffusion_pytorch/video_diffusion_pytorch_conv3d.py:212-216, :399-404) run forward and backward in every fine-tuning
 * step (the samplers read them from a per-timestep table).  w is the nn.Linear weight [M][K] as torch stores it; rows of x / y /
 * gy / gx may be strided (strides in floats).  K, M and the strides must be multiples of 4 and the pointers 16-byte aligned
 * (SDC_EINVAL otherwise: the caller then uses sdc_conv / sdc_conv_wgrad, which take any shape).  Fixed summation order, no atomics.
 *   sdc_linear        y[r][m]  = bias[m] + sum_k x[r][k] w[m][k]          (bias may be null)
 *   sdc_linear_dgrad  gx[r][k] = sum_m gy[r][m] w[m][k]
 *   sdc_linear_wgrad  gw[m][k] = sum_r gy[r][m] x[r][k],  gbias[m] = sum_r gy[r][m]   (gbias may be null; gw contiguous [M][K]) */
int sdc_linear(const float* x, const float* w, const float* bias, float* y, int rows, int K, int M, int64_t x_stride,
               int64_t y_stride, void* stream);
int sdc_linear_dgrad(const float* gy, const float* w, float* gx, int rows, int K, int M, int64_t gy_stride, int64_t gx_stride,
                     void* stream);
int sdc_linear_wgrad(const float* gy, const float* x, float* gw, float* gbias, int rows, int K, int M, int64_t gy_stride,
                     int64_t x_stride, void* stream);

/* ------------------------------------------------- weight content stamp */
/* out_dev[0] = order-independent 64-bit checksum over n device spans of 32-bit words (span index, word index and bits all
 * enter it).  The host wrapper stamps a plan's packed weights with it: `p.data.lerp_()` / `p.data = ...` (the reference's EMA
 * updates, 2d/video_diffusion_pytorch/video_diffusion_pytorch_conv3d.py:121-124; ema_pytorch in 1D/model/trainer.py,
 * tokamak/model/trainer.py) change the parameters without moving any autograd version counter.  spans_dev, out_dev: device memory. */
typedef struct {
    const void* ptr;          /* 4-byte aligned device address */
    int64_t nwords;           /* 32-bit words */
} SdcSpan;
int sdc_checksum_spans(const SdcSpan* spans_dev, int n, uint64_t* out_dev, void* stream);

/* ------------------------------------------------- fine-tuning optimizer step (clip + SGD / Adam / AdamW + EMA) */
/* The tail of the reference's fine-tuning iteration (1D/inference/inference_ft.py:189-226, 2d/inference_2d.py:261-281):
 * clip_grad_norm_ -> optimizer.step() -> ema.update(), over EVERY parameter of a net in one streaming pass.
 *
 * The caller fills p, g, m, v, ema, n of every item (fp32, n elements each; v null for SGD, ema null without an EMA twin; m, v
 * and ema are caller-owned and start at zero); sdc_optim_plan (host only, no GPU call) cuts the items into chunks of *chunk
 * elements, fills chunk0 (the prefix a workgroup searches to find the item of its chunk) and returns the chunk size, the
 * chunk count and the launch grid (4096 elements; grid = min(total_chunks, 2048), the chunks are grid-strided).  The caller copies the table to device memory and
 * calls sdc_optim_step(kind, table_dev, ...) per iteration; work holds sdc_optim_bytes(total_chunks) bytes.
 * Errors of the plan: SDC_ENULL for a null p, g or m, or a null v under Adam / AdamW; SDC_EALIGN for a pointer that is not
 * 4-byte aligned; SDC_EINVAL for n <= 0 or an unknown kind.  16-byte aligned items take 16-byte loads and stores.
 *
 * hp_dev: SDC_OPT_HP_COUNT doubles in device memory (indices below).  state_dev: one SdcOptState in device memory, zeroed by
 * the caller before the first step.  Everything the step decides -- learning rate, step count, bias corrections, the every-N-th
 * EMA update, the non-finite skip -- is read from these two, so a captured replay follows the caller's changes of hp_dev.
 *
 * One step (t = state.step + 1; element arithmetic in fp32: each a * b + c below is one fused multiply-add, every other operation
 * is rounded once, nothing else is contracted; sqrt and the division are correctly rounded):
 *   norm   = sqrt(sum over all items of g^2), per-chunk partial sums in fp64 summed in a fixed order (bit-identical from run
 *            to run); coef = min(1, max_grad_norm / (norm + 1e-6)) (torch.nn.utils.clip_grad_norm_); gc = g * coef.
 *            g ITSELF IS NOT REWRITTEN.  Without SDC_OPT_CLIP coef = 1, and without SDC_OPT_SKIP_NONFINITE as well the norm is
 *            not computed (state.grad_norm keeps its value).
 *   SDC_OPT_SKIP_NONFINITE: a NaN / Inf norm leaves p, m, v, ema and state.step untouched (state.applied = 0).
 *   kind SDC_OPT_SGD    g' = gc + wd p;  m = momentum m + g';  p -= lr m          (dampening 0, no Nesterov)
 *   kind SDC_OPT_ADAM   g' = gc + wd p;  m += (1 - b1)(g' - m);  v = b2 v + (1 - b2) g'^2;
 *                       p -= (lr / bc1) * (m / (sqrt(v) / sqrt(bc2) + eps)),  bc = 1 - b^t in fp64
 *   kind SDC_OPT_ADAMW  p *= 1 - lr wd first, g' = gc, then as Adam
 *   EMA (items with ema): when t % ema_update_every == 0: t <= ema_update_after_step ? ema = p : ema += (1 - ema_beta)(p - ema)
 *            with the updated p; on other steps ema is not touched. */
#define SDC_OPT_SGD 0
#define SDC_OPT_ADAM 1
#define SDC_OPT_ADAMW 2
#define SDC_OPT_CLIP 1
#define SDC_OPT_SKIP_NONFINITE 2
#define SDC_OPT_HP_LR 0
#define SDC_OPT_HP_BETA1 1              /* momentum for SGD */
#define SDC_OPT_HP_BETA2 2
#define SDC_OPT_HP_EPS 3
#define SDC_OPT_HP_WEIGHT_DECAY 4
#define SDC_OPT_HP_MAX_GRAD_NORM 5
#define SDC_OPT_HP_EMA_BETA 6
#define SDC_OPT_HP_EMA_UPDATE_EVERY 7   /* whole numbers stored as doubles; < 1 means never */
#define SDC_OPT_HP_EMA_UPDATE_AFTER_STEP 8
#define SDC_OPT_HP_COUNT 9
typedef struct SdcOptItem {
    float* p;
    const float* g;
    float* m;
    float* v;
    float* ema;
    int64_t n;
    int64_t chunk0;           /* filled by sdc_optim_plan: chunks of the items before this one */
} SdcOptItem;
typedef struct SdcOptState {
    int64_t step;             /* steps applied so far */
    float grad_norm;          /* total gradient 2-norm of the last step that computed it */
    float clip_coef;          /* the coefficient the last step multiplied the gradients by */
    int applied;              /* 0: the last step was skipped (SDC_OPT_SKIP_NONFINITE) */
    int ema_mode;             /* last step: 0 EMA untouched, 1 copied, 2 moving average */
} SdcOptState;
int sdc_optim_plan(SdcOptItem* items, int n, int kind, int* chunk, int* total_chunks, int* grid);
size_t sdc_optim_bytes(int total_chunks);
int sdc_optim_step(int kind, const SdcOptItem* items_dev, int n, int chunk, int total_chunks, int grid, const double* hp_dev,
                   SdcOptState* state_dev, void* work, int flags, void* stream);

/* ----------------------------------------------------------------- graphs */
int sdc_graph_begin(void* stream);
int sdc_graph_end(void* stream, void** graph_exec);
int sdc_graph_launch(void* graph_exec, void* stream);
int sdc_graph_destroy(void* graph_exec);

/* ------------------------------------------------------ timing (bench only) */
int sdc_event_create(void** ev);
int sdc_event_record(void* ev, void* stream);
int sdc_event_elapsed_ms(void* ev0, void* ev1, float* ms);   /* synchronises on ev1 */
int sdc_event_destroy(void* ev);

/* ---- Tokamak score check: the KSTAR surrogate rollout (tokamak/kstar_solver.py:163-428 KSTARSolver.control / predict_0d /
 * simulate; the Keras networks of tokamak/common/model_structure.py:69-152; called per sample by control_trajectories,
 * tokamak/utils/metrics.py:60-85).  Replaces the 122 x B serial single-sample Keras predict() calls with one launch. */
#define SDC_KSTAR_SEQ 10      /* window rows (seq_len, kstar_solver.py:34) */
#define SDC_KSTAR_NIN 18      /* window columns: 4 fed-back outputs + 13 inputs + year */
#define SDC_KSTAR_UNITS 100   /* LSTM units of kstar_v220505 (model_structure.py:108) */
typedef struct {
    int nlayers;              /* BatchNormalization -> Dense blocks (Dropout is the identity at inference) */
    int width[7];             /* width[0] inputs ... width[nlayers] outputs, each <= 256 */
    int act[6];               /* per block: 0 linear, 1 sigmoid */
    const float* params;      /* per network, per block: inv[in], off[in] (BatchNorm folded: x*inv + off), kernel[in][out], bias[out] */
    int64_t stride;           /* floats between consecutive networks of an ensemble */
} SdcKstarMlp;
typedef struct {
    int n_lstm, n_bpw;        /* networks averaged (the reference's n_model_box, kstar_solver.py:156-162) */
    const float* lstm;        /* per network: bn0 inv, off [18]; K0 [18][400]; R0 [100][400]; b0 [400]; bn1 inv, off [100];
                                 K1 [100][400]; R1 [100][400]; b1 [400]   (Keras gate order i, f, c, o) */
    int64_t lstm_stride;      /* floats between networks, >= sdc_kstar_lstm_floats() */
    SdcKstarMlp head;         /* 100 -> ... -> 4 after the second LSTM (BatchNorm, Dense(50, sigmoid), BatchNorm, Dense(4)) */
    SdcKstarMlp steady;       /* kstar_nn, 17 -> 4: the steady-state first row */
    SdcKstarMlp bpw;          /* bpw_nn, 8 -> 2: (beta_p, W_mhd) */
    double lstm_ystd[4], lstm_ymean[4], nn_ystd[4], nn_ymean[4], bpw_ystd[2], bpw_ymean[2];
    double scale;             /* 10 ** np.log10(1000) as the host evaluates it (f2i / i2f, kstar_solver.py:35,107-113) */
    double inputs0[15];       /* i2f(f2i(input_init)), kstar_solver.py:84,150-152 */
    double low_action[9], high_action[9];
    double year_in;
} SdcKstarModel;
size_t sdc_kstar_lstm_floats(void);
/* actions: element (b, t, i) at actions[b*act_b_stride + t*act_t_stride + i*act_c_stride], t < nsteps, i < 9 (so a (B, C, T)
 * sample tensor is read in place).  out (B, nsteps + 1, 8) fp64 rows [bn, bp, h89, h98, q95, q0, li, wmhd]; work: 4 doubles. */
int sdc_kstar_rollout(const SdcKstarModel* m, const float* actions, int64_t act_b_stride, int64_t act_t_stride,
                      int64_t act_c_stride, double* out, double* work, int B, int nsteps, void* stream);

/* ---- Closed loop: the reference's trained real-time controller inside the rollout (KSTARDataGenerator.auto_control /
 * random_target_simulation, tokamak/kstar_data_generator_random_target.py:379-409,433-517; the actor is SB2_model.predict,
 * tokamak/common/model_structure.py:191-204, bavg = 0).  The action of step t depends on rows t-1 .. t-3, so the controller
 * runs in the kernel: per step it forms the observation (the last three (raw action, beta_p, q95, l_i) rows, oldest first,
 * then the target of the step), evaluates the actor in fp64 (normalise 2(obs - low)/(high - low) - 1, relu layers, tanh head,
 * 0.5 (high_a - low_a)(y + 1) + low_a; one thread per output column, k ascending) and hands the RAW output to the control /
 * predict_0d code of sdc_kstar_rollout -- the same device code, a compile-time variant of one kernel, with the same three
 * launch shapes; replaying a loop's quantised actuator values through sdc_kstar_rollout gives its rows bit for bit.
 * Like the rollout, parity with the TensorFlow surrogate is unpinned. */
typedef struct {
    int nlayers;            /* hidden relu layers, <= 4 */
    int width[6];           /* width[0] = 39 observation entries ... width[nlayers + 1] = 9 actuators, each <= 256 */
    const float* params;    /* device memory; per layer: kernel[in][out], bias[out]; the tanh head last */
    double low_state[39], high_state[39];   /* (LOW_ACTION + LOW_TARGET) * 3 + LOW_TARGET and its HIGH twin */
    double hist0[12];       /* the row every history slot starts with: LOW_ACTION + TARGET_INIT */
} SdcKstarPolicy;
/* targets (B, nsteps, 3) fp64 [beta_p, q95, l_i], finite (the caller checks: the reference's int(nan) raises).
 * rows (B, nsteps + 1, 8) as sdc_kstar_rollout's out (row 0: the steady-state network's); actions (B, nsteps, 9) the raw
 * policy outputs before the clip; inputs (B, nsteps + 1, 15) the quantised simulator inputs after each control(), row 0 =
 * inputs0; work: 4 doubles.  A policy with width[0] != 39, an output width other than 9, more than 4 hidden layers or a
 * width outside 1..256 returns SDC_EINVAL and launches nothing. */
int sdc_kstar_closed_loop(const SdcKstarModel* m, const SdcKstarPolicy* p, const double* targets, double* rows, double* actions,
                          double* inputs, double* work, int B, int nsteps, void* stream);

/* ---- Smoke score check: the fluid rollout behind InferencePipeline.multi_evaluate (2d/inference_2d.py:389-447 ->
 * 2d/dataset/apps/evaluate_solver.py:209-350 `solver`: per step get_envolve :82-111 = control ring + last interior velocity ->
 * divergence_free (phi/flow.py:317-326: float64 CG of phi/solver/base.py:63-103 on the matrix of phi/solver/sparse.py:27-77)
 * -> three semi-Lagrangian advections (phi/math/nd.py:407-428) -> bucket book-keeping :262-336).  Replaces one Python process
 * per sample with one launch: one 512-thread workgroup per sample, the 127 x 127 pressure problem on chip for the whole rollout.
 *   c1, c2          controls (B, nt, nx, nx) fp32: element (b, f, y, x) at [b*ctrl_b_stride + f*ctrl_f_stride + y*nx + x]
 *                   (so the channel slices pred[:, :, 3] / pred[:, :, 4] of a (B, nt, 7, nx, nx) sample are read in place)
 *   init_density    (B, nx, nx) fp32, batch stride dens_b_stride; init_velocity (128, 128, 2) fp32 staggered, batch stride
 *                   vel_b_stride (0 = one field for all samples, init_velocity_ evaluate_solver.py:77-79)
 *   fluid_mask      (127, 127) bytes, 1 = fluid / 0 = obstacle (build_obstacles_pi_128, evaluate_solver.py:29-60)
 *   bucket_labels, safe_labels   (128, 128) bytes: 0 = none, k = absorbing area k - 1 of get_bucket_mask / get_bucket_mask_safe
 *                   (evaluate_solver.py:114-178; areas must not overlap); n_buckets in [2, 8], n_safe in [1, 8]
 *   out             (B, nt, 7, nx, nx) fp64 = multi_evaluate's solver_out: density, velocity x, y, control x, y, smoke_out
 *                   record, safe record; out_zero (B, nt, nx, nx) fp64 = `zero_densitys`, may be null
 *   work            sdc_smoke_rollout_workspace_bytes(B) bytes, 16-byte aligned
 *   nx divides 128, nt divides per_timelength (256); ring_lo/ring_hi = 16/112: the interior the controls do not reach;
 *   accuracy / max_iterations = 1e-8 / 500 (evaluate_solver.py:108, phi/solver/sparse.py:88). */
size_t sdc_smoke_rollout_workspace_bytes(int B);
int sdc_smoke_rollout(const float* c1, const float* c2, int64_t ctrl_b_stride, int64_t ctrl_f_stride,
                      const float* init_density, int64_t dens_b_stride, const float* init_velocity, int64_t vel_b_stride,
                      const unsigned char* fluid_mask, const unsigned char* bucket_labels, const unsigned char* safe_labels,
                      int n_buckets, int n_safe, double* out, double* out_zero, void* work, size_t work_bytes, int B, int nt,
                      int nx, int per_timelength, int ring_lo, int ring_hi, double accuracy, int max_iterations, void* stream);

/* Smoke data generator (2d/dataset/apps/a_gen_dataset_128.py `loop_write`): the same fluid step as sdc_smoke_rollout, one
 * workgroup per trajectory, with the loop closed inside the kernel -- on frame f = 1 .. T the velocity outside [16:112, 16:112]
 * is the previous frame's projected velocity plus the ring field of the frame (or, on the frames the schedule marks absolute,
 * the ring field itself); interior cells keep the previous velocity.  Where the ring numbers come from is the caller's business.
 *   ring            (B, T, 128, 128, 2) fp64, batch / frame strides in elements (both even), a frame dense; only cells outside
 *                   [16:112, 16:112] are read; 16-byte aligned
 *   start_yx        (B, 2) int32: the 10 x 10 square of ones on the 127 x 127 density grid starts at (y0, x0)
 *   schedule        (B, T) bytes, entry f - 1 for frame f: bit 0 = 1 the ring field is the value / 0 it is added to the previous
 *                   velocity; bits 1-2 = 0 no book-keeping, 1 book-keeping then record, 2 record then book-keeping (a frame is
 *                   recorded when f % rs == 0, whatever these bits say, so every output element is written)
 *   map_index       (B) int32 into label_maps (n_maps, 128, 128) bytes: 0 = none, k = absorbing area k - 1, areas must not
 *                   overlap; map_buckets = HOST array of n_maps bucket counts, each in [2, 8]; n_maps in [1, 4]
 *   fluid_mask      (127, 127) bytes as for sdc_smoke_rollout; initial_vy: the initial velocity is (0, initial_vy) everywhere
 *   outputs, fp64, n = T / rs + 1 recorded frames (frame 0 = the initial state), L = 128 / ss cells sub-sampled [::ss]:
 *     density (B, n, L, L) (ss = 1: the 127 x 127 field inside a zero 128 x 128 frame), density_zero the same for the copy the
 *     book-keeping empties (may be null), velocity and control (B, n, L, L, 2) (16-byte aligned; a control frame is the ring
 *     value before the velocity mask, zero inside, of frame f = rec * rs + 1; the last one stays zero as in the reference),
 *     smoke (B, n, smoke_cols): the cumulative amounts of the sample's nb areas, the emptied field's sum at column nb, zeros
 *     after it; smoke_cols in [max bucket count + 1, 16]
 *   work            sdc_smoke_datagen_workspace_bytes(B) bytes, 16-byte aligned
 * T a multiple of rs, ss divides 128; accuracy / max_iterations as for sdc_smoke_rollout.  SDC_ENULL / SDC_EINVAL / SDC_EALIGN
 * before any launch.  A sample's result depends on neither its batch nor its block index. */
size_t sdc_smoke_datagen_workspace_bytes(int B);
int sdc_smoke_datagen(const double* ring, int64_t ring_b_stride, int64_t ring_f_stride, const int32_t* start_yx,
                      const unsigned char* schedule, const int32_t* map_index, const unsigned char* label_maps,
                      const int32_t* map_buckets, int n_maps, const unsigned char* fluid_mask, double initial_vy,
                      double* density, double* density_zero, double* velocity, double* control, double* smoke, int smoke_cols,
                      void* work, size_t work_bytes, int B, int T, int rs, int ss, double accuracy, int max_iterations,
                      void* stream);

/* --------------------------------------------------- Burgers data generator */
/* What 1D/data/generate_burgers.py does to make the 1-D Burgers task's training data (csrc/sdc_burgers_gen.hip).
 *
 * sdc_burgers_rollout_wave: the Euler rollout of sdc_burgers_rollout -- the same expressions in the same order, FMA contraction
 * off, fp32 denormals kept, so the same bits -- with one wave per trajectory and the state in registers: lane l owns the
 * K = ceil(s / 64) cells [l K, l K + K), K in {1, 2, 4, 8}, so s <= 512 (more is SDC_EINVAL); no LDS, no barrier.  Cells >= s and the
 * two neighbours outside the wave are the Dirichlet ghosts, +0.0f on every step.
 *   u0 (Nu0, s) contiguous; force value of trajectory n, interval t, cell c: f[fi * f_sn + t * f_st + c] (element strides >= 0;
 *   f_st = 0: one force row for every interval, the reference's mode='const'); traj (N, Nt + 1, s) contiguous, row 0 = u0.
 *   pair_mode 0: ui = fi = n, needs Nu0 == Nf == N (burgers_numeric_solve_free);
 *   pair_mode 1: ui = n / Nf, fi = n % Nf, needs N == Nu0 * Nf (burgers_numeric_solve: every u0 against every f).
 *   Nt intervals of `rec` steps each (rec <= 0 is SDC_EINVAL); dt, coef_transport, d0..d2 as for sdc_burgers_rollout.
 *   waves_per_block: 0 = the library's choice (4), else 1 .. 16; waves share nothing, so it changes no result.
 * SDC_ENULL / SDC_EINVAL before any launch, the output untouched. */
int sdc_burgers_rollout_wave(const float* u0, const float* f, float* traj, int N, int Nu0, int Nf, int s, int Nt, int rec,
                             int64_t f_sn, int64_t f_st, int pair_mode, float dt, float coef_transport, float d0, float d1, float d2,
                             int waves_per_block, void* stream);

/* sdc_burgers_synth: the initial states and forces of make_data_varying_f / make_data (generate_burgers.py:302-418) from their drawn
 * parameters, evaluated in float64 in the reference's operation order (contraction off) and rounded once to fp32.
 *   upar (Nu0, 6) fp64 {loc1, amp1, sig1, loc2, amp2, sig2}; fpar (Nf, 8, 5) fp64 {amp, xloc, xsig, tloc, tsig} per term (amp with
 *   its randint factor, the sigmas with their 0.5, multiplied on the host); x (s), ts (Nt) the fp32 grids; mask (s) fp32 or null.
 *   e(d, sig) = exp((-0.5 (d d)) / (sig sig));  u0 = amp1 e(x - loc1, sig1) + amp2 e(x - loc2, sig2);
 *   term_k = (amp_k (e(x - xloc_k, xsig_k) [mask])) (comp e(ts - tloc_k, tsig_k)), f = ((term_0 + term_1) + ...) + term_7 -> fp32,
 *   then, if alpha != 1, min(max(f alpha, -10), 10) in fp32.  ts == null: make_data's form, term_k = amp_k e(...), Nt must be 1.
 *   u0 (Nu0, s) fp32 and f (Nf, Nt, s) fp32; either may be null (skipped, with its parameters), not both. */
int sdc_burgers_synth(const double* upar, const double* fpar, const float* x, const float* ts, const float* mask, double comp,
                      float alpha, float* u0, float* f, int Nu0, int Nf, int s, int Nt, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SDC_H */
