/*
 * udaseg.h -- C-ABI of libudaseg_hip.so: the MI355X (gfx950) kernels behind the segmentation /
 * domain-adaptation training hot path of bempt/uda_aerial_semantic_segmentation_research.
 *
 * The reference has no FFI layer: its boundary is the torch.nn.Module / callable protocol its trainers
 * use.  Each entry point below therefore names the reference call it replaces (file:line
 * under the reference tree); the Python side (uda_aerial_semantic_segmentation_research_amd/) mirrors the
 * reference's classes on top of these symbols via ctypes.  INTEGRATION.md shows the binding.
 *
 * Conventions
 *  - plain pointers + sizes only; every pointer is DEVICE memory owned by the caller (PyTorch);
 *    the library allocates nothing and never synchronises the host;
 *  - `stream` is a hipStream_t passed as void* (0 = default stream); all launches are asynchronous;
 *  - activations are NHWC fp32 with a channel count that is a multiple of 4 (images are padded 3->4,
 *    logits 23->24 by udaseg_nchw_to_nhwc / the head conv); conv weights are OHWI [co][kh][kw][ci];
 *  - return 0 on success, a negative UDASEG_E_* otherwise; udaseg_last_error() gives the message
 *    (thread-local).  No C++ exception crosses the boundary.
 */
#ifndef UDASEG_H
#define UDASEG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UDASEG_OK 0
#define UDASEG_E_BADARG (-1)
#define UDASEG_E_UNSUPPORTED (-2)
#define UDASEG_E_WORKSPACE (-3)
#define UDASEG_E_HIP (-4)

#define UDASEG_ACT_NONE 0
#define UDASEG_ACT_LEAKY 1 /* y = x > 0 ? x : slope * x ; slope 0 => ReLU */

int udaseg_version(void);
/* Runtime switches for cross-checks and tuning: ONE table (csrc/api.hip).  Every key has a default that an environment variable
 * may supply (read once, at first use); udaseg_set_option(key, value) overrides it for the process (value -1: back to the default),
 * udaseg_get_option reads the effective value, udaseg_option_name gives the key's environment variable, udaseg_option_epoch counts
 * the overrides made so far (callers that cache routing answers compare it).  Both gather loops accumulate in the same order:
 * forward and data-gradient results are bit-identical between GENERIC_GATHER 0 and 1. */
#define UDASEG_OPT_GENERIC_GATHER 0        /* UDASEG_IGEMM_GENERIC: 1: the implicit-GEMM kernels keep their generic gather loop (cross-check of the uniform-tap loop); setting this key also sets WGRAD_GENERIC */
#define UDASEG_OPT_F32_SPLIT 1             /* UDASEG_F32_SPLIT: 0: the SHARED-SOURCE fp32 kernels (udaseg_conv2d_fwd / _dgrad / _wgrad) stay on the fp32 matrix pipe */
#define UDASEG_OPT_WGRAD_GENERIC 2         /* UDASEG_WGRAD_GENERIC: 1: the split-K weight gradients keep their generic gather loop */
#define UDASEG_OPT_F32_HALO 3              /* UDASEG_F32_SPLIT: 0: the halo-resident three-term kernels (udaseg_conv2d_*_f32x3, _up_, _n16_) report 'not supported' (A/B: everything on the fp32 pipe) */
#define UDASEG_OPT_F3_CFG 4                /* UDASEG_F3_CFG: conv_halo_f32x3.hip: one tile configuration 1..12 for every launch (udaseg_f32x3_force_config) */
#define UDASEG_OPT_F3_WS 5                 /* UDASEG_F3_WS: 0: the one-role forward kernel everywhere (A/B of the wave-specialised form) */
#define UDASEG_OPT_F3_SIGNS 6              /* UDASEG_F3_SIGNS: 0: no + - - + sign pattern in the split kernels and their packers (bias measurements) */
#define UDASEG_OPT_IGEMM_TILE 7            /* UDASEG_IGEMM_TILE: conv_igemm.hip: 1 (128x128) | 2 (128x64) | 3 (64x64) | 4 (128x32) for every launch */
#define UDASEG_OPT_IGEMM_X3 8              /* UDASEG_IGEMM_X3: three-term mode of the shared implicit GEMM: 0 off | 1 (64x64 tile) | 2 (128x64) | 3 (128x128) */
#define UDASEG_OPT_NO_FOLD 9               /* UDASEG_NO_FOLD: 1: no pixel folding of the <= 32-channel bf16 layers */
#define UDASEG_OPT_WGRAD_X3_BLOCKS 10       /* UDASEG_WGRAD_X3_BLOCKS: blocks of a conv_wgrad_x3_kernel launch */
#define UDASEG_OPT_WGRAD_BLOCKS 11          /* UDASEG_WGRAD_BLOCKS: blocks of a split-K weight-gradient launch (0: 3072 fp32 / the bf16 rules) */
#define UDASEG_OPT_WGRAD_NO_XCD 12          /* UDASEG_WGRAD_NO_XCD: 1: no XCD-aware block order in the bf16 split-K weight gradient */
#define UDASEG_OPT_WGRAD_X3 13              /* UDASEG_WGRAD_X3: 0: conv_wgrad_x3_kernel off (shared-source weight gradients on the fp32 pipe) */
#define UDASEG_OPT_NO_WGRAD_HALO 14         /* UDASEG_NO_WGRAD_HALO: 1: the per-tap split-K weight gradients everywhere */
#define UDASEG_OPT_WGRAD_F3_BLOCKS 15       /* UDASEG_WGRAD_F3_BLOCKS: blocks of an fp32 halo weight-gradient launch */
#define UDASEG_OPT_WGRAD_HALO_BLOCKS 16     /* UDASEG_WGRAD_HALO_BLOCKS: blocks of a bf16 halo weight-gradient launch */
#define UDASEG_OPT_WGRAD_DEEP_BLOCKS 17     /* UDASEG_WGRAD_DEEP_BLOCKS: blocks of the 16-pixel-wide halo weight gradients (0: 128 fp32 / 256 bf16) */
#define UDASEG_OPT_WGRAD_DB 18              /* UDASEG_WGRAD_DB: 0: the single-buffer 4-row form of the 64 x 64 fp32 halo weight gradient */
#define UDASEG_OPT_REDUCE_BLOCKS 19         /* UDASEG_REDUCE_BLOCKS: cap on the blocks of the BatchNorm reduction kernels (0: 512) */
#define UDASEG_OPT_BN_APPLY_PT 20           /* UDASEG_BN_APPLY_PT: vectors per thread of the BatchNorm apply kernels */
#define UDASEG_OPT_GEMM_1X1_TILE 21         /* UDASEG_GEMM_1X1_TILE: conv1x1_gemm_bf16_kernel: 128 | 256 pixel tiles for every launch */
#define UDASEG_OPT_GEMM_1X1 22              /* UDASEG_GEMM_1X1: 0: r50's 1x1 projections never take the small-GEMM kernel */
#define UDASEG_OPT_GEMM_1X1_MAXM 23         /* UDASEG_GEMM_1X1_MAXM: most pixels of a launch the small-GEMM kernel takes */
#define UDASEG_OPT_NO_STREAM 24             /* UDASEG_NO_STREAM: 1: 1x1 layers stay on the tile kernel */
#define UDASEG_OPT_HALO_CFG 25              /* UDASEG_HALO_CFG: conv_halo_bf16.hip: one configuration for every launch */
#define UDASEG_OPT_NO_HALO 26               /* UDASEG_NO_HALO: 1: every bf16 layer on the shared implicit-GEMM source */
#define UDASEG_OPT_NO_HALO_S2 27            /* UDASEG_NO_HALO_S2: 1: the discriminator's 4x4 / stride 2 layers on the shared source */
#define UDASEG_OPT_HALO_W16 28              /* UDASEG_HALO_W16: tile for widths 16 divides and 32 does not: 0 | 4 | 5 | 6 */
#define UDASEG_OPT_HALO_DEEP 29             /* UDASEG_HALO_DEEP: 0: no 8 x 16-pixel tile for deep low-resolution layers */
#define UDASEG_OPT_HALO_S2_CK 30            /* UDASEG_HALO_S2_CK: channels per staged chunk of the 4x4 / stride 2 halo form: 32 | 64 */
#define UDASEG_OPT_UP_CFG 31                /* UDASEG_UP_CFG: conv_up_f32x3.hip: one tile configuration 1..8 for every launch (udaseg_up_f32x3_force_config) */
#define UDASEG_OPT_WGRAD_UP_BLOCKS 32       /* UDASEG_WGRAD_UP_BLOCKS: blocks of a conv_wgrad_up_kernel launch (0: 96; udaseg_wgrad_up_set_blocks) */
#define UDASEG_OPT_WGRAD_PAIR 33            /* UDASEG_WGRAD_PAIR: fp32 weight gradients of 16-channel inputs on the pair-packed halo kernel: bit 0 the 16 -> 16 layers, bit 1 those of 24 / 32 produced channels, bit 2 the up-sampled 32 -> 16 layer without a skip half; 0: all on conv3x3_small_wgrad_kernel */
#define UDASEG_OPT_WGRAD_PAIR_BLOCKS 34     /* UDASEG_WGRAD_PAIR_BLOCKS: blocks of a pair-packed halo weight-gradient launch (0: 120) */
#define UDASEG_OPT_STEM_WGRAD_BN 35        /* UDASEG_STEM_WGRAD_BN: 0: udaseg_conv_stem_wgrad_bn_ok answers no (the stem's BatchNorm apply pass + split-K weight gradient, A/B) */
#define UDASEG_OPT_STEM_WGRAD_BLOCKS 36    /* UDASEG_STEM_WGRAD_BLOCKS: cap on the blocks of a conv_small_ci_wgrad_kernel launch (0: one per CU; udaseg_stem_wgrad_set_blocks) */
#define UDASEG_OPT_COUNT 37
int udaseg_set_option(int key, int value);
int udaseg_get_option(int key);
int udaseg_option_count(void);
const char* udaseg_option_name(int key);
int udaseg_option_epoch(void);
const char* udaseg_last_error(void);
/* number of HIP devices visible to the library (0 on a CPU-only box; never initialises a context) */
int udaseg_device_count(void);
/* Host-side helpers of the launch plan (no reference counterpart: what `torch.zeros` / `stream.wait_stream` do for the reference's
 * eager ops, at a tenth of their host cost -- BASELINE cfg 3 is bound by the host's launch rate).  udaseg_memset_async: byte fill of
 * a device buffer in stream order; udaseg_stream_wait: `waiter` waits for everything enqueued on `signal` so far. */
int udaseg_memset_async(void* ptr, int value, size_t bytes, void* stream);
int udaseg_stream_wait(void* waiter_stream, void* signal_stream);

/* Geometry of one 2-D convolution, NHWC. hi/wi/ci: input; ho/wo/co: output; square stride, symmetric pad.
 * ci and co are the PHYSICAL channel counts (multiples of 4). */
typedef struct {
  int n, hi, wi, ci;
  int ho, wo, co;
  int kh, kw, stride, pad;
} udaseg_conv_desc;

/* ---- convolutions: torch.nn.functional.conv2d reached through smp.Unet.forward (reference
 *      src/models/train.py:341, src/models/adversarial_trainer.py:104) and DomainDiscriminator.forward
 *      (src/models/discriminator.py:54).  Implicit GEMM on v_mfma_f32_32x32x2_f32 (exact fp32). ---- */

/* y[n,ho,wo,co] (+)= conv(x, w) + bias, then optional activation. bias may be NULL. */
int udaseg_conv2d_fwd(const udaseg_conv_desc* d, const float* x, const float* w, const float* bias, float* y,
                      int act, float slope, int accumulate, void* stream);
/* y = conv(x, w) + bias AND the training-mode BatchNorm statistics of y in the same pass: stats[R][2][co] f64 (sum, sum of
 * squares; R = udaseg_bn_replicas(), caller-zeroed) -- exactly what udaseg_bn_stats(y) would add, without re-reading y. */
int udaseg_conv2d_fwd_bnstats(const udaseg_conv_desc* d, const float* x, const float* w, const float* bias, float* y,
                              double* stats, void* stream);
/* Inference form: y = act(conv(x, w) + bias + residual) in one kernel (bias, residual optional).  With udaseg_bn_fold this
 * is the whole conv+BN(+add)+ReLU block of an eval-mode forward (reference validate(): src/models/train.py:391-438). */
int udaseg_conv2d_fwd_fused(const udaseg_conv_desc* d, const float* x, const float* w, const float* bias,
                            const float* residual, float* y, int act, float slope, void* stream);
/* bf16 storage variants (BASELINE configs 3 and 5): x, w, residual, y are bf16 (channel counts multiples of 8), accumulation,
 * bias and BatchNorm statistics fp32/f64; v_mfma_f32_32x32x16_bf16.  out_f32 != 0 writes y as fp32 (segmentation logits).
 * stats may be NULL. */
int udaseg_conv2d_fwd_bf16(const udaseg_conv_desc* d, const void* x, const void* w, const float* bias, const void* residual,
                           void* y, int out_f32, int act, float slope, double* stats, void* stream);
int udaseg_conv2d_dgrad_bf16(const udaseg_conv_desc* d, const void* dy, const void* w_t, void* dx, int accumulate,
                             void* stream);
/* dw (fp32 master gradient) from bf16 x and dy */
int udaseg_conv2d_wgrad_bf16(const udaseg_conv_desc* d, const void* x, const void* dy, float* dw, int accumulate, void* stream);
/* dx[n,hi,wi,ci] (+)= conv_transpose(dy, w).  w_t is the dgrad packing [ci][kh][kw][co] made by
 * udaseg_pack_dgrad_weights.  Autograd of the convs above: loss.backward() at train.py:343. */
int udaseg_conv2d_dgrad(const udaseg_conv_desc* d, const float* dy, const float* w_t, float* dx, int accumulate,
                        void* stream);
/* dx = conv_transpose(dy, w) AND, in the same pass, the two reductions of the BatchNorm backward of the layer in front of this
 * convolution (the one whose output prev_y [n][hi][wi][ci] went through training-mode BN + activation to become this
 * convolution's input):  g = dx * act'(gamma*(prev_y-mean)*rstd + beta),  bsums[0][c] += sum g,  bsums[1][c] += sum g*xhat
 * -- exactly what udaseg_bn_bwd_reduce(dz = dx, z = NULL, y = prev_y, ...) adds, without re-reading dx (loss.backward(),
 * reference src/models/train.py:343).  Only for activations with a single consumer (dx is their complete gradient) and for
 * geometries udaseg_conv2d_dgrad_bnreduce_ok() accepts (whole tiles: stride 1, no K-slices, not the small-channel kernel). */
int udaseg_conv2d_dgrad_bnreduce_ok(const udaseg_conv_desc* d);
int udaseg_conv2d_dgrad_bnreduce(const udaseg_conv_desc* d, const float* dy, const float* w_t, float* dx, const float* prev_y,
                                 const float* save_mean, const float* save_rstd, const float* gamma, const float* beta, int act,
                                 float slope, double* bsums, void* stream);
/* bf16 storage: same reductions from the LDS-staged epilogue (g from the bf16-rounded gradient, as the stand-alone
   udaseg_bn_bwd_reduce_bf16 would read it back); any stride-1 geometry */
int udaseg_conv2d_dgrad_bnreduce_bf16_ok(const udaseg_conv_desc* d);
int udaseg_conv2d_dgrad_bnreduce_bf16(const udaseg_conv_desc* d, const void* dy, const void* w_t, void* dx, const void* prev_y,
                                      const float* save_mean, const float* save_rstd, const float* gamma, const float* beta,
                                      int act, float slope, double* bsums, void* stream);
/* dw[co][kh][kw][ci] (+)= sum over pixels of dy (x) x.  If !accumulate dw is overwritten.
 * Split-K partials are combined with fp32 atomics. */
int udaseg_conv2d_wgrad(const udaseg_conv_desc* d, const float* x, const float* dy, float* dw, int accumulate,
                        void* stream);
/* ---- fused decoder input: smp's DecoderBlock computes conv(cat([interpolate(a, 2, 'nearest'), skip], 1)) (reference model
 *      created at src/test_system.py:90-95; trace fixture: aten::upsample_nearest2d + aten::cat in front of every decoder
 *      conv1).  The concatenation is never materialised: the convolution reads a [n][hi/2][wi/2][ca] at (iy >> 1, ix >> 1)
 *      for its first ca input channels and skip [n][hi][wi][ci-ca] for the rest (skip == NULL when ca == ci).  d describes
 *      the convolution on the VIRTUAL input (ci = ca + cb, hi x wi = full resolution), stride 1.  Channel counts must be
 *      multiples of the K-tile (32 fp32 / 64 bf16) unless the small-channel kernel applies (ci <= 32, no skip). ---- */
int udaseg_conv2d_fwd_upcat(const udaseg_conv_desc* d, const float* a, const float* skip, int ca, const float* w,
                            const float* bias, float* y, int act, float slope, double* stats, void* stream);
int udaseg_conv2d_fwd_upcat_bf16(const udaseg_conv_desc* d, const void* a, const void* skip, int ca, const void* w,
                                 const float* bias, void* y, int act, float slope, double* stats, void* stream);
/* its data gradient, written straight into the two gradient tensors: dx_a [n][hi][wi][ca] = gradient of the UP-SAMPLED a
 * (the caller reduces it 2x2 with udaseg_upsample2x_concat_bwd, cb = 0), dx_b [n][hi][wi][ci-ca] = gradient of skip.
 * ca must be a multiple of 64. */
int udaseg_conv2d_dgrad_split(const udaseg_conv_desc* d, const float* dy, const float* w_t, float* dx_a, float* dx_b, int ca,
                              void* stream);
int udaseg_conv2d_dgrad_split_bf16(const udaseg_conv_desc* d, const void* dy, const void* w_t, void* dx_a, void* dx_b, int ca,
                                   void* stream);
/* and its weight gradient, one call per source: the columns (tap, c_off + c), c < src_c, of dw[co][kh*kw][d->ci] from the
 * source tensor src ([..][src_c] channels; up != 0: at half resolution behind the nearest x2 up-sampling).  accumulate must
 * be set unless the slice is the whole gradient (src_c == d->ci). */
int udaseg_conv2d_wgrad_part(const udaseg_conv_desc* d, const float* src, int src_c, int c_off, int up, const float* dy,
                             float* dw, int accumulate, void* stream);
int udaseg_conv2d_wgrad_part_bf16(const udaseg_conv_desc* d, const void* src, int src_c, int c_off, int up, const void* dy,
                                  float* dw, int accumulate, void* stream);
/* w[co][kh*kw][ci] -> w_t[ci][kh*kw][co] */
int udaseg_pack_dgrad_weights(const udaseg_conv_desc* d, const float* w, float* w_t, void* stream);
/* The same for every convolution of a network in one launch: table[i] = {src float-offset into arena, dst float-offset
 * into packed, co, kh*kw, ci} (int32, device memory). */
int udaseg_pack_dgrad_batched(const float* arena, float* packed, const int* table, int entries, void* stream);
/* Conv FLOPs (2*MAC) of one call, for roofline accounting. */
double udaseg_conv_flops(const udaseg_conv_desc* d);

/* ---- layout: the DataLoader hands NCHW images (train.py:337); kernels want NHWC with C%4==0 ---- */
/* x[n][c][h][w] -> y[n][h][w][cpad], channels c..cpad-1 zero-filled */
int udaseg_nchw_to_nhwc(const float* x, float* y, int n, int c, int h, int w, int cpad, void* stream);

/* most channels the BatchNorm kernels take (they keep per-channel coefficients in LDS, 64 KB at most for the bf16 backward) */
#define UDASEG_BN_MAX_C 4096                    /* every fp32 entry point; bf16 statistics, apply, reduce, channel_sum */
#define UDASEG_BN_BWD_APPLY_BF16_MAX_C 3272     /* udaseg_bn_bwd_apply_bf16: 20 bytes of LDS per channel */
#define UDASEG_BN_BWD_RECOMPUTE_BF16_MAX_C 2336 /* udaseg_bn_bwd_apply_recompute_bf16: 28 bytes of LDS per channel */

/* ---- batch norm (training mode) + activation: torch.nn.BatchNorm2d/ReLU/LeakyReLU inside smp.Unet and
 *      discriminator.py:21-33.  sums / bsums = [R][2][c] doubles (R = udaseg_bn_replicas() replicated accumulators of
 *      sum and sum of squares, spread to avoid same-address atomic serialisation), zeroed by the caller. ---- */
int udaseg_bn_replicas(void);
int udaseg_bn_stats(const float* y, int64_t pixels, int c, double* sums, void* stream);
/* the same for a bf16 tensor (channels a multiple of 8): behind the library GEMMs, which have no statistics epilogue */
int udaseg_bn_stats_bf16(const void* y, int64_t pixels, int c, double* sums, void* stream);
/* z = act(gamma*(y-mean)*rstd + beta (+ residual)); writes save_mean/save_rstd [c]; updates running stats
 * (momentum, unbiased variance) when running_mean != NULL.  residual may be NULL. */
int udaseg_bn_apply(const float* y, const double* sums, const float* gamma, const float* beta, const float* residual,
                    float* z, int64_t pixels, int c, float eps, float momentum, float* running_mean,
                    float* running_var, float* save_mean, float* save_rstd, int act, float slope, void* stream);
/* eval mode: z = act(gamma*(y-running_mean)/sqrt(running_var+eps) + beta (+ residual)) */
int udaseg_bn_apply_eval(const float* y, const float* gamma, const float* beta, const float* running_mean,
                         const float* running_var, const float* residual, float* z, int64_t pixels, int c, float eps,
                         int act, float slope, void* stream);
/* eval mode, folded into the preceding conv: w_folded[co][row_len] = w * gamma/sqrt(var+eps);
 * bias_folded[co] = beta + (bias - mean) * gamma/sqrt(var+eps).  bias may be NULL. */
int udaseg_bn_fold(const float* w, const float* bias, const float* gamma, const float* beta, const float* running_mean,
                   const float* running_var, float eps, int co, int row_len, float* w_folded, float* bias_folded, void* stream);
/* backward, pass 1: g = dz * act'(z); bsums[0][c] += sum g, bsums[1][c] += sum g*xhat (doubles, caller-zeroed).
 * z may be NULL when the layer had no residual input: the activation's argument is then re-evaluated from y, gamma and
 * beta (the same fused multiply-add as udaseg_bn_apply), which saves one pass over the activation; gamma / beta are only
 * read in that case. */
int udaseg_bn_bwd_reduce(const float* dz, const float* z, const float* y, const float* save_mean,
                         const float* save_rstd, const float* gamma, const float* beta, int64_t pixels, int c,
                         double* bsums, int act, float slope, void* stream);
/* backward, pass 2: dy (+)= gamma*rstd*(g - mean(g) - xhat*mean(g*xhat)); dres (+)= g if dres != NULL;
 * dgamma/dbeta (+)= from bsums.  z may be NULL as in pass 1 (then beta is read). */
int udaseg_bn_bwd_apply(const float* dz, const float* z, const float* y, const float* save_mean,
                        const float* save_rstd, const float* gamma, const float* beta, const double* bsums, float* dy,
                        float* dres, float* dgamma, float* dbeta, int64_t pixels, int c, int act, float slope,
                        int accumulate_dy, int accumulate_dres, int accumulate_param, void* stream);
/* plain activation backward for a conv+bias+act epilogue (discriminator layer 1): dy = dz * act'(z) */
int udaseg_act_bwd(const float* dz, const float* z, float* dy, int64_t count, int act, float slope, void* stream);
/* out[c] (+)= sum over pixels of x[p][c]  (bias gradients) */
int udaseg_channel_sum(const float* x, int64_t pixels, int c, float* out,
                       int accumulate, void* stream);
/* same, with the caller's scratch for the partial sums of large inputs (udaseg_channel_sum_scratch_bytes(c) bytes, owned by
   `stream` until the call's work has run); the plain form takes a stream-ordered allocation instead */
int udaseg_channel_sum_ws(const float* x, int64_t pixels, int c, float* out, int accumulate, float* scratch,
                          size_t scratch_bytes, void* stream);
size_t udaseg_channel_sum_scratch_bytes(int c);

/* ---- pooling / resize glue inside smp.Unet ---- */
/* max_pool2d(3, 2, 1): y[n,ho,wo,c], idx = argmax tap (0..8, first max in scan order) */
int udaseg_maxpool3x3s2_fwd(const float* x, float* y, uint8_t* idx, int n, int h, int w, int c, void* stream);
int udaseg_maxpool3x3s2_bwd(const float* dy, const uint8_t* idx, float* dx, int n, int h, int w, int c, int accumulate,
                            void* stream);
/* out[n,2h,2w,ca+cb] = cat(nearest_x2(a[n,h,w,ca]), skip[n,2h,2w,cb]); skip may be NULL (cb = 0) */
int udaseg_upsample2x_concat_fwd(const float* a, const float* skip, float* out, int n, int h, int w, int ca, int cb,
                                 void* stream);
/* da (+)= 2x2 sum of dout[..., :ca]; dskip (+)= dout[..., ca:] */
int udaseg_upsample2x_concat_bwd(const float* dout, float* da, float* dskip, int n, int h, int w, int ca, int cb,
                                 int accumulate_da, int accumulate_dskip, void* stream);

/* The decoder's alternate up-sampling mode (north_star: "bilinear-upsample + conv"; the reference's traced model uses nearest,
 * SURVEY F5): out = cat(interpolate(a, scale_factor=2, mode="bilinear", align_corners=False), skip) and its backward in
 * gather form.  a / skip / out / gradients are fp32 (channels % 4 == 0) or, with bf16 != 0, bf16 (channels % 8 == 0). */
int udaseg_upsample2x_bilinear_concat_fwd(const void* a, const void* skip, void* out, int n, int h, int w, int ca, int cb,
                                          int bf16, void* stream);
int udaseg_upsample2x_bilinear_concat_bwd(const void* dout, void* da, void* dskip, int n, int h, int w, int ca, int cb,
                                          int accumulate_da, int accumulate_dskip, int bf16, void* stream);

/* ---- per-pixel cross entropy: nn.CrossEntropyLoss() at train.py:208,342 (mean, no weights/ignore) ----
 * logits[p][ldc] with `classes` valid channels; target int64[p]; lse[p] saved for backward;
 * partials: scratch of udaseg_ce_partials() doubles; loss: 1 float. */
int udaseg_ce_partials(void);
int udaseg_ce_fwd(const float* logits, const int64_t* target, int64_t pixels, int classes, int ldc, float* lse,
                  double* partials, float* loss, void* stream);
/* dlogits[p][ldc] = (softmax - onehot) * (*grad_out) / pixels; pad channels written as 0.
 * Optional (ldc <= 32): colsum[ldc] = per-class sum of dlogits over all pixels (= the head conv's bias gradient, reference
 * src/models/train.py:343), produced in the same pass; colsum_partials = scratch of udaseg_ce_partials()*ldc floats. */
int udaseg_ce_bwd(const float* logits, const int64_t* target, const float* lse, const float* grad_out, int64_t pixels,
                  int classes, int ldc, float* dlogits, float* colsum_partials, float* colsum, void* stream);

/* round 5: both in ONE pass over the logits (ldc <= 32): loss as udaseg_ce_fwd leaves it (bit for bit), dlogits / colsum as
 * udaseg_ce_bwd leaves them for an upstream gradient of exactly 1 (bit for bit) -- what loss.backward() (train.py:343) passes.
 * udaseg_scale_unless_one(x, count, x2, count2, g): x[i] *= *g, x2[j] *= *g unless the DEVICE scalar *g is 1 (then the launch
 * returns at once): the backward of a loss whose gradient was made ahead of time (count % 4 == 0, count2 <= 256). */
int udaseg_ce_fwd_bwd(const float* logits, const int64_t* target, int64_t pixels, int classes, int ldc, double* partials, float* loss,
                      float* dlogits, float* colsum_partials, float* colsum, void* stream);
int udaseg_scale_unless_one(float* x, int64_t count, float* x2, int count2, const float* g, void* stream);

/* ---- cross entropy with options: torch.nn.functional.cross_entropy(weight, ignore_index, reduction, label_smoothing) ----
 * valid(p): target[p] != ignore_index (when has_ignore) and 0 <= target[p] < classes.  Departure from torch: an out-of-range
 * target that is not ignore_index raises no error (a launch that never synchronises cannot); it is void, and counted.
 *   l_p       = (1-eps)*w[t]*(-logp[t]) + (eps/classes)*(-sum_c w[c]*logp[c])  at a valid pixel, exactly 0 at a void one
 *   dl_p/dz_k = (1-eps)*w[t]*(P_k - [k==t]) + (eps/classes)*(P_k*sum_c w[c] - w[k]), exactly 0 at a void pixel in all ldc lanes
 *   'sum' = sum_p l_p; 'mean' (mean != 0) = 'sum' / D, D = sum over valid p of w[t_p] (all void: NaN loss, zero gradient).
 * weight: `classes` floats or NULL (all 1); 0 <= eps <= 1; ignore_index: any int64; the plain udaseg_ce_* calls are untouched.
 *
 * udaseg_ce_target_stats reads ONLY the targets (8 B/pixel): denom[0] = D in f64 and stats[0..2] = {valid, void (== ignore_index),
 * invalid (out of range)} pixel counts, by fixed-order sums (same bits on every call); partials: 4*udaseg_ce_partials() doubles. */
int udaseg_ce_target_stats(const int64_t* target, const float* weight, int64_t pixels, int classes, int has_ignore,
                           int64_t ignore_index, double* partials, double* denom, int64_t* stats, void* stream);
/* ONE pass over the logits (ldc <= 32), as udaseg_ce_fwd_bwd: loss, dlogits for an upstream gradient of 1 -- already divided by
 * *denom when mean != 0 (denom may be NULL otherwise) -- and the optional column sums (the head conv's bias gradient). */
int udaseg_ce_opt_fwd_bwd(const float* logits, const int64_t* target, const float* weight, int64_t pixels, int classes, int ldc,
                          int has_ignore, int64_t ignore_index, float eps, int mean, const double* denom, double* partials,
                          float* loss, float* dlogits, float* colsum_partials, float* colsum, void* stream);
/* Two-pass route (no_grad forwards, ldc > 32, reduction 'none', a second backward): lse[p] saved (0 at void pixels);
 * loss (1 float, reduced) and / or loss_px[p] = l_p ('none'): at least one of the two. */
int udaseg_ce_opt_fwd(const float* logits, const int64_t* target, const float* weight, int64_t pixels, int classes, int ldc,
                      int has_ignore, int64_t ignore_index, float eps, int mean, const double* denom, float* lse, double* partials,
                      float* loss, float* loss_px, void* stream);
/* dlogits[p] = (*grad_out, NULL = 1) * (grad_px[p], NULL = 1: the per-pixel upstream gradient of 'none') * dl_p/dz (/ *denom when
 * mean != 0); column sums optional, ldc <= 32 only. */
int udaseg_ce_opt_bwd(const float* logits, const int64_t* target, const float* weight, const float* lse, const float* grad_out,
                      const float* grad_px, int64_t pixels, int classes, int ldc, int has_ignore, int64_t ignore_index, float eps,
                      int mean, const double* denom, float* dlogits, float* colsum_partials, float* colsum, void* stream);

/* ---- hard-pixel mining for the cross entropy (csrc/ohem.hip): OHEM (keep p < thresh, but at least min_kept pixels) and the
 * bootstrapped / top-k cross entropy (keep the hardest fraction), exact on the device: no sort, no host read, same bits every run.
 * logits: padded NHWC fp32 [pixels][ldc], ldc % 4 == 0, classes <= ldc <= 32, 0 < pixels < 2^31; target int64; weight optional.
 *   valid(p):      as udaseg_ce_opt_*.  A valid pixel whose row (channels < classes) is not all finite is NON-FINITE: void,
 *                  counted on its own, loss and gradient exactly 0.
 *   confidence:    m = the first maximum of the row, S = sum_c expf(z_c - m) in udaseg_conf_hist's order, p = expf(z_t - m) / S of
 *                  the TARGET class: 0 <= p <= 1, so the fp32 bits of p are an order-preserving unsigned integer below 2^30.
 *                  conf[pixel] = p; -1.0f at void, out-of-range and non-finite pixels.
 *   selection:     n = number of valid finite pixels; k = min_kept, or ceil(fraction * n) in float64 when fraction >= 0;
 *                  q = the k-th smallest p (1-indexed); -inf when k == 0, +inf when k > n.
 *                  kept(p) iff conf[p] >= 0 and (p < thresh or p <= q).  Ties at q are ALL kept: the kept set depends on the
 *                  values alone (not on pixel order or launch shape) and holds at least min(k, n) pixels.  Top-k is thresh = 0.
 *   loss:          l = -w[t] * log softmax(z)[t] over the kept pixels; 'mean' divides by D = the fixed-order f64 sum of w[t]
 *                  over the kept pixels (no kept pixel: NaN loss, all-zero gradient; 'sum': 0).
 *   gradient:      exactly 0 in all ldc lanes of every pixel that is not kept.
 * The k-th smallest is a three-level radix select over the 30 value bits, 10 bits a level (bits 29..20, 19..10, 9..0).
 * hist: int64 [1024] per level, ZEROED BY THE CALLER.  state: int64 [UDASEG_KTH_STATE], ZEROED BY THE CALLER before level 0:
 *   state[0]  prefix: the bits of q found so far (after level L, bits 29 .. 20 - 10 L); after level 2 the exact fp32 bits of q
 *   state[1]  rank still to find inside the prefix's bin (1-indexed; 0: nothing is selected, k == 0 or n == 0)
 *   state[2]  n          state[3]  k          state[4]  flags: bit 0 k == 0, bit 1 k >= n          state[5]  levels done
 *   state[6..7] unused (0)
 * udaseg_kth_hist + udaseg_kth_select are a primitive of their own: the exact k-th smallest of a device buffer of floats in
 * [0, 2); a value with its sign bit set or >= 2 (-1.0f, inf, NaN) is skipped and not counted in n. */
#define UDASEG_KTH_STATE 8
/* One pass over the logits: conf, hist0 += the histogram of bits 29..20 of p over the valid finite pixels,
 * counters[0..2] += {void (== ignore_index), out-of-range targets, non-finite rows} (int64, zeroed by the caller). */
int udaseg_ohem_conf(const float* logits, const int64_t* target, int64_t pixels, int classes, int ldc, int has_ignore,
                     int64_t ignore_index, float* conf, int64_t* hist0, int64_t* counters, void* stream);
/* hist += the 10-bit histogram of `level` (0, 1, 2) over the values whose higher bits equal state's prefix (level 0: all values
 * in [0, 2); state may be NULL there). */
int udaseg_kth_hist(const float* values, int64_t count, int level, const int64_t* state, int64_t* hist, void* stream);
/* One block, bounded loops.  Level 0: n = the histogram's total, k from min_kept (>= 0; fraction < 0) or from fraction (in
 * [0, 1]); every level: the bin that holds the rank, into state.  Levels 1 and 2 ignore min_kept and fraction. */
int udaseg_kth_select(const int64_t* hist, int level, int64_t min_kept, double fraction, int64_t* state, void* stream);
/* out[0] = q, out[1] = max(q, thresh) from a state after level 2. */
int udaseg_kth_value(const int64_t* state, float thresh, float* out, void* stream);
/* One pass over conf, target and weight (no logits): *denom = D (f64, udaseg_ce_target_stats' order), counts[0..1] = {valid finite,
 * kept} pixels, keep[p] = 1 / 0 (uint8, optional); partials: 3*udaseg_ce_partials() doubles. */
int udaseg_ohem_denom(const float* conf, const int64_t* target, const float* weight, int64_t pixels, int classes, float thresh,
                      const int64_t* state, double* partials, double* denom, int64_t* counts, uint8_t* keep, void* stream);
/* udaseg_ce_opt_fwd_bwd with the keep predicate, read from conf and state (what the selection itself used): loss, dlogits for an
 * upstream gradient of 1 (divided by *denom when mean != 0), optional column sums.  dlogits == NULL: the loss alone. */
int udaseg_ce_ohem_fwd_bwd(const float* logits, const int64_t* target, const float* weight, const float* conf, const int64_t* state,
                           float thresh, int64_t pixels, int classes, int ldc, int mean, const double* denom, double* partials,
                           float* loss, float* dlogits, float* colsum_partials, float* colsum, void* stream);

/* ---- Lovasz-softmax loss (csrc/lovasz.hip; Berman, Rannen Triki, Blaschko 2018): the Jaccard surrogate on a grid of B error bins
 * instead of a sort.  Integer atomics only and fixed-order float sums: the same bits on every run.
 * logits: padded NHWC fp32 [pixels][ldc], ldc % 4 == 0, classes <= ldc <= 32, 0 < pixels < 2^31; target int64.
 *   valid(p):      as udaseg_ce_opt_*; a valid pixel whose row (channels < classes) is not all finite is void too.  Void pixels
 *                  are in no table and hold exact zeros in all ldc lanes of the gradient.
 *   group:         the whole batch (images == 1) or one image (images == N; pixels % images == 0).
 *   error:         p_c = expf(z_c - m) / S (m the row maximum, S as udaseg_conf_hist), e_c = [t == c] ? 1 - p_c : p_c
 *   grid:          bins = B, a power of two in [64, 4096]; bin(e) = min(B - 1, floor(e B))
 *   tables:        int32 [images][classes][2][B], ZEROED BY THE CALLER: row 0 the fg pixels (t == c) per bin, row 1 the bg pixels
 *   coefficients:  bins walked from the top (largest error first); a0, b0 the fg / bg counts strictly above a bin, p, n its own,
 *                  G the fg total of the (group, class):
 *                    G > 0:   wf = (1 / (G + b0) + 1 / (G + b0 + n)) / 2,  wb = (G - a0 - p / 2) / ((G + b0) (G + b0 + n))
 *                    G == 0:  wb = 1 / n in the highest non-empty bin, 0 elsewhere; wf = 0
 *                  times the reduction factor 1 / (images * present classes of the group) (0 for an absent class), or
 *                  1 / (images * classes) when all_classes != 0.  coef: fp32 [images][classes][2][B].
 *   loss:          sum over the valid finite pixels and the classes of e_c * coef[group][c][fg ? 0 : 1][bin(e_c)]
 *   gradient:      d_c = -coef (fg) / +coef (bg), taken as constants; dz_k = p_k (d_k - sum_c p_c d_c)
 *   bound:         0 <= (the sort-based loss of the paper) - loss <= sum_c slack[c] <= 1 / B    */
/* One pass over logits and targets: tables += the error histograms; counters[0..3] += {valid finite, void (== ignore_index),
 * out-of-range, non-finite} pixels (int64, zeroed by the caller). */
int udaseg_lovasz_hist(const float* logits, const int64_t* target, int64_t pixels, int classes, int ldc, int has_ignore,
                       int64_t ignore_index, int images, int bins, int32_t* tables, int64_t* counters, void* stream);
/* tables -> coef, present[images][classes] (int32 1 / 0: the class has a fg pixel in the group) and slack[classes] (f64, the
 * reduction-weighted grid bound summed over the groups).  slack_parts: images * classes doubles of scratch. */
int udaseg_lovasz_table(const int32_t* tables, int images, int classes, int bins, int all_classes, float* coef, int32_t* present,
                        double* slack_parts, double* slack, void* stream);
/* The second pass over the logits: *loss, dlogits for an upstream gradient of 1 (NULL: the loss alone), optional column sums.
 * ce_weight != 0 adds ce_weight * mean over the valid finite pixels of -log p_t and its gradient, the count read from
 * counters[0] of udaseg_lovasz_hist (no such pixel: NaN).  partials: udaseg_ce_partials() doubles. */
int udaseg_lovasz_fwd_bwd(const float* logits, const int64_t* target, const float* coef, const int64_t* counters, int64_t pixels,
                          int classes, int ldc, int has_ignore, int64_t ignore_index, int images, int bins, float ce_weight,
                          double* partials, float* loss, float* dlogits, float* colsum_partials, float* colsum, void* stream);

/* ---- the reference's other segmentation losses (src/models/losses.py), same logits layout as udaseg_ce_* (ldc <= 32) ----
 * udaseg_seg_partials(): doubles of scratch the *_fwd calls below need in `partials`. */
int udaseg_seg_partials(void);
/* DiceLoss (losses.py:110-152): softmax over classes, per image b and class c
 *   I = sum_pix p_c*[t==c], U = sum_pix p_c + sum_pix [t==c]; loss = 1 - mean_{b,c} (2I+smooth)/(U+smooth).
 * pooled != 0: the segmentation_models_pytorch DiceLoss(mode='multiclass') form used by the reference's UDALoss
 *   (src/models/uda.py:84): I, U summed over the batch too, score_c = (2I+smooth)/max(U+smooth, eps),
 *   loss = mean_c (1-score_c)*[class c occurs in target]   (smp defaults: smooth 0, eps 1e-7).
 * sums: batch*3*classes doubles, caller-zeroed; coef: batch*2*classes floats kept for udaseg_dice_bwd. */
int udaseg_dice_fwd(const float* logits, const int64_t* target, int batch, int64_t pix_per_image, int classes, int ldc,
                    float smooth, float eps, int pooled, double* sums, float* coef, float* loss, void* stream);
/* dlogits (+)= (*grad_out) * weight * dLoss/dlogits (grad_out may be NULL = 1); pad channels written as 0 */
int udaseg_dice_bwd(const float* logits, const int64_t* target, const float* coef, const float* grad_out, float weight,
                    int batch, int64_t pix_per_image, int classes, int ldc, float* dlogits, int accumulate, void* stream);
/* focal term of WeightedSegmentationLoss (losses.py:181-197): ce = w[t]*(-log softmax_t) (class_weights may be NULL),
 * pt = exp(-ce), f = alpha*(1-pt)^gamma*ce; loss (+)= mean (mean=1) or sum (mean=0) of f over pixels */
int udaseg_focal_fwd(const float* logits, const int64_t* target, const float* class_weights, float alpha, float gamma,
                     int64_t pixels, int classes, int ldc, int mean, double* partials, float* loss, int accumulate,
                     void* stream);
/* dlogits (+)= (*grad_out) * weight * df/dlogits per pixel (the caller folds 1/pixels into weight for 'mean') */
int udaseg_focal_bwd(const float* logits, const int64_t* target, const float* class_weights, float alpha, float gamma,
                     const float* grad_out, float weight, int64_t pixels, int classes, int ldc, float* dlogits,
                     int accumulate, void* stream);
/* The four calls above with void labels: a pixel whose target is ignore_index (any int64) or lies outside [0, classes) is left out
 * of all three Dice sums, has a focal term of 0 ('mean' still divides by `pixels`; class_weights[t] is not read for it) and a
 * gradient of exactly 0 in all ldc lanes. */
int udaseg_dice_fwd_ignore(const float* logits, const int64_t* target, int batch, int64_t pix_per_image, int classes, int ldc,
                           float smooth, float eps, int pooled, double* sums, float* coef, float* loss, int64_t ignore_index,
                           void* stream);
int udaseg_dice_bwd_ignore(const float* logits, const int64_t* target, const float* coef, const float* grad_out, float weight,
                           int batch, int64_t pix_per_image, int classes, int ldc, float* dlogits, int accumulate,
                           int64_t ignore_index, void* stream);
int udaseg_focal_fwd_ignore(const float* logits, const int64_t* target, const float* class_weights, float alpha, float gamma,
                            int64_t pixels, int classes, int ldc, int mean, double* partials, float* loss, int accumulate,
                            int64_t ignore_index, void* stream);
int udaseg_focal_bwd_ignore(const float* logits, const int64_t* target, const float* class_weights, float alpha, float gamma,
                            const float* grad_out, float weight, int64_t pixels, int classes, int ldc, float* dlogits,
                            int accumulate, int64_t ignore_index, void* stream);
/* ConsistencyLoss (losses.py:53-108): p_i = softmax(z_i / T);
 * loss = (KL(p2||p1) + KL(p1||p2)) / (2 * batch)  (F.kl_div(..., reduction='batchmean') both ways, averaged) */
int udaseg_consistency_fwd(const float* z1, const float* z2, float temperature, int batch, int64_t pixels, int classes,
                           int ldc, double* partials, float* loss, void* stream);
/* gradients with respect to BOTH predictions (the reference detaches neither); d1 or d2 may be NULL */
int udaseg_consistency_bwd(const float* z1, const float* z2, float temperature, const float* grad_out, float weight,
                           int batch, int64_t pixels, int classes, int ldc, float* d1, float* d2, int accumulate,
                           void* stream);

/* ---- output-space adaptation (AdvEnt, Vu et al., CVPR 2019; maximum squares, Chen et al., ICCV 2019), csrc/advent.hip ----
 * Same logits layout as above: fp32 [pixels][ldc], 2 <= classes <= ldc <= 32, ldc % 4 == 0 (log C divides, so classes >= 2);
 * only lanes < classes are read, the pad lanes may hold any finite junk.  With s = 1 / log(classes), lp = log_softmax(z),
 * p = exp(lp):
 *   I_c = p_c > 0 ? -s * p_c * lp_c : 0      weighted self-information; a lane whose probability is 0 (underflow, a -inf logit)
 *                                            contributes exactly 0 and gets a gradient of exactly 0 -- it is never 0 * inf
 *   H   = sum_c I_c                          normalised entropy, in [0, 1]
 * udaseg_selfinfo_fwd: maps[pixels][cpad] (fp32, or bf16 when out_bf16 != 0; classes <= cpad <= 32, cpad % 4 == 0 for fp32 and
 * cpad % 8 == 0 for bf16; cpad may differ from ldc) = I_c in the lanes < classes and exactly 0 in the lanes [classes, cpad): a
 * convolution reads this buffer in place.  entropy[pixels] (fp32, NULL = not wanted) = H. */
int udaseg_selfinfo_fwd(const float* logits, int64_t pixels, int classes, int ldc, void* maps, int cpad, int out_bf16,
                        float* entropy, void* stream);
/* dmaps[pixels][cpad] (fp32, or bf16 when in_bf16 != 0; pad lanes ignored) = the gradient with respect to the maps;
 * with g_c = -s * (lp_c + 1) * dmaps_c for c < classes:  dlogits[pixels][ldc]_k = p_k * (g_k - sum_c p_c * g_c), pad lanes
 * written as exactly 0. */
int udaseg_selfinfo_bwd(const float* logits, const void* dmaps, int64_t pixels, int classes, int ldc, int cpad, int in_bf16,
                        float* dlogits, void* stream);
/* The direct part, loss and gradient in ONE pass over the logits (as udaseg_ce_fwd_bwd):
 *   kind 0, entropy (MinEnt):  loss = (1 / pixels) * sum_p H_p;   dlogits_k = -(s / pixels) * p_k * (lp_k + H_nat),
 *                              H_nat = -sum_c p_c * lp_c
 *   kind 1, maximum squares:   loss = -(1 / (2 * pixels)) * sum_p sum_c p_c^2;   dlogits_k = -(1 / pixels) * p_k * (p_k - sum_c p_c^2)
 * dlogits[pixels][ldc] (NULL = not wanted) is the gradient for an upstream gradient of 1, pad lanes exactly 0; entropy[pixels]
 * (NULL = not wanted) = H whatever the kind; partials: udaseg_seg_partials() doubles of scratch.  The loss is a fixed-order sum
 * (no float atomics): the same bits on every call, with and without dlogits / entropy. */
int udaseg_entropy_loss(const float* logits, int64_t pixels, int classes, int ldc, int kind, double* partials, float* loss,
                        float* dlogits, float* entropy, void* stream);

/* ---- distillation: a loss between student logits and a teacher DISTRIBUTION with pixel and image weights (Hinton et al. 2015;
 * symmetric cross entropy, Wang et al., ICCV 2019; an extension, the reference has no counterpart).  Loss and gradient in ONE
 * pass over the logits, as udaseg_ce_fwd_bwd.
 * logits: fp32 [pixels][ldc], teacher: fp32 [pixels][ldt], pixels = batch * pix_per_image, both 16-byte aligned,
 * 2 <= classes <= ld <= 32, ld % 4 == 0, ldt may differ from ldc; only lanes < classes are read.  Per pixel, in fp32:
 *   lp = log_softmax(z), p = exp(lp) of the student
 *   probs == 0: q = softmax(t * teacher_inv_temp), lq = log_softmax(t * teacher_inv_temp);  probs == 1: q_c = t_c, lq_c = logf(q_c)
 *   Q = sum_c q_c
 *   kind 0 (soft CE):    l = -sum_c q_c * lp_c;           kind 1 (KL(q||p)):  l = sum_c q_c * (lq_c - lp_c)
 *                        dl/dz_k = Q * p_k - q_k for both; a lane with q_c == 0 contributes exactly 0 (never 0 * inf)
 *   kind 2 (symmetric):  l = alpha * (-sum_c q_c * lp_c) + beta * sum_c p_c * g_c,  g_c = -max(lq_c, log_floor) (log_floor < 0),
 *                        g_c = -log_floor where q_c == 0;   dl/dz_k = alpha * (Q * p_k - q_k) + beta * p_k * (g_k - sum_c p_c * g_c);
 *                        a lane with p_c == 0 contributes exactly 0 to the reverse term
 * w_p = weight_px[p] * weight_img[p / pix_per_image] (fp32 product; either pointer NULL = 1).  A pixel is VOID -- loss exactly 0,
 * gradient exactly 0 in all ldc lanes -- when w_p == 0, when w_p is negative or not finite, when a teacher lane < classes (times
 * teacher_inv_temp for probs == 0) is not finite, or, with probs == 1, when a q_c lies outside [0, 1] or Q == 0.
 * stats (NULL = not wanted): int64 [3], ACCUMULATED with integer atomics: counted pixels, void by weight 0, void otherwise.
 * loss = sum_p w_p * l_p, divided by pixels when mean != 0, by *denom (device f64, udaseg_pixel_weight_sum) when denom != NULL
 * (*denom == 0: NaN); mean and denom exclude each other.  partials: udaseg_seg_partials() doubles of scratch; the loss is a
 * fixed-order sum (no float atomics): the same bits on every call, with and without dlogits / colsum.
 * dlogits[pixels][ldc] (NULL = not wanted): the gradient for an upstream gradient of 1, divided like the loss, pad lanes exactly 0.
 * colsum[ldc] with colsum_partials[udaseg_seg_partials() * ldc] (both or neither): the gradient's per-class sums, as
 * udaseg_ce_fwd_bwd's (the head convolution's bias gradient). */
int udaseg_soft_ce_fwd_bwd(const float* logits, const float* teacher, const float* weight_px, const float* weight_img, int batch,
                           int64_t pix_per_image, int classes, int ldc, int ldt, int probs, int kind, float teacher_inv_temp,
                           float alpha, float beta, float log_floor, int mean, const double* denom, double* partials, float* loss,
                           float* dlogits, float* colsum_partials, float* colsum, int64_t* stats, void* stream);
/* denom[0] = the fixed-order f64 sum of w_p (as above) over the pixels whose weight does not void them (w_p > 0 and finite);
 * counts: int64 [2] = zero weights, negative or non-finite weights (written).  Reads only the weights, as udaseg_ce_target_stats
 * reads only the targets.  partials: 3 * udaseg_seg_partials() doubles of scratch.  Both weight pointers NULL: denom = pixels. */
int udaseg_pixel_weight_sum(const float* weight_px, const float* weight_img, int batch, int64_t pix_per_image, double* partials,
                            double* denom, int64_t* counts, void* stream);
/* Per image i: above[i] (int64, written) = its pixels whose winner confidence is >= tau, the confidence being exactly
 * udaseg_conf_hist's (1 / S for logits, q[c^] for probabilities); nonfinite[i] (int64, written) = its NON-FINITE pixels, which
 * are in no count; share[i] = (float)((double)above[i] / pix_per_image).  Integer atomics only: exact, the same on every run.
 * scores: fp32 [batch * pix_per_image][ldc], 16-byte aligned, 0 < classes <= 32, classes <= ldc, ldc % 4 == 0; batch <= 65535. */
int udaseg_conf_share(const float* scores, int batch, int64_t pix_per_image, int classes, int ldc, int probs, float tau,
                      int64_t* above, int64_t* nonfinite, float* share, void* stream);

/* ---- validation metrics (SegmentationTrainer.calculate_metrics, train.py:225-243; src/analysis/metrics.py:17-29):
 * confusion[t*classes + argmax(logits[p])] += 1 over all pixels (int64, caller-zeroed); pred[p] = argmax (optional).
 * classes <= 32, ldc <= 32. */
int udaseg_argmax_confusion(const float* logits, const int64_t* target, int64_t pixels, int classes, int ldc,
                            int64_t* confusion, int64_t* pred, void* stream);

/* ---- per-class ROC / PR curves (SegmentationTrainer._log_roc_curves / _log_pr_curves, train.py:245-328, which sort
 * softmax(outputs)[:, c] on the host with sklearn).  Score of class c: the log-odds of the softmax probability,
 * s_c = z_c - log(sum_{j != c} exp(z_j)); grid: bin = clamp(floor((s_c + score_range) * bins / (2 * score_range)), 0, bins - 1)
 * (a NaN score is counted in bin 0).  pos[c*bins + b] += pixels of target c, neg[c*bins + b] += pixels of every other target in
 * [0, classes), with s_c in bin b (int64 counters that ACCUMULATE across calls; the caller zeroes them once).
 * pixels < 2^31, classes <= 32, ldc <= 32, bins in {256, 512, 1024, 2048, 4096}, score_range > 0. */
int udaseg_score_hist(const float* logits, const int64_t* target, int64_t pixels, int classes, int ldc, int bins,
                      float score_range, int64_t* pos, int64_t* neg, void* stream);
/* from the two tables, per class, bins walked from the top (tp, fp = running sums; P, N = totals): auc = trapezoid over
 * (fp/N, tp/P) from (0, 0) (sklearn.metrics.roc_auc_score of the bin index), ap = sum (recall_k - recall_{k-1}) * precision_k
 * (average_precision_score of the bin index), auc_slack = 0.5 * sum_b pos_b * neg_b / (P * N) >= |auc - auc of the exact score|,
 * support[c] = {P, N}.  auc and auc_slack are NaN when P == 0 or N == 0, ap when P == 0.  Deterministic (fixed summation order). */
int udaseg_curve_finish(const int64_t* pos, const int64_t* neg, int classes, int bins, double* auc, double* ap,
                        double* auc_slack, int64_t* support, void* stream);

/* ---- calibration of the winner's confidence (csrc/calib.hip): reliability tables, expected calibration error, temperature fit.
 * (The reference bins a host copy of the softmax with numpy.)  scores / logits: padded NHWC fp32 [pixels][ldc], 16-byte aligned,
 * 0 < classes <= 32, classes <= ldc, ldc % 4 == 0, 0 < pixels < 2^31; target: int64 [pixels], a target outside [0, classes) is
 * VOID and left out of everything.  inv_temp: device float [1], the reciprocal temperature beta (NULL: beta = 1); a beta that is
 * not a positive finite number makes every pixel of the call non-finite.  ONE definition of the confidence, udaseg_conf_hist's:
 *   c^ = first maximum of z, m = z[c^], p = 1 / sum_{j < classes} expf((z_j - m) * beta), the sum as four partial sums by j % 4,
 *   then (s0 + s1) + (s2 + s3); with inv_temp == NULL bit for bit udaseg_conf_share's and udaseg_conf_hist's p;
 *   probs == 1 (probabilities q; inv_temp must be NULL): c^ = first maximum of q, p = q[c^].
 * A pixel with a valid target is NON-FINITE when p is not a finite number in [0, 1] (a NaN or +inf logit, all logits -inf; with
 * probs also a NaN in any channel < classes): it is in no table.
 *   b = min((int)floorf(p * (float)bins), bins - 1),  2 <= bins <= 64
 *   tables: uint64 [3][classes][bins], indexed by the PREDICTED class c^:
 *     tables[0][c^][b] += 1;  tables[1][c^][b] += (c^ == target);  tables[2][c^][b] += __float2uint_rn(p * 16777216.f)
 *   (the confidence in 2^-24 fixed point: integer sums, independent of order, below 2^55 at 2^31 pixels).
 *   counters: int64 [3] += the pixels in the tables, the void pixels, the non-finite pixels (they sum to `pixels`).
 * Both buffers ACCUMULATE across calls; the caller zeroes them once.  Integer atomics only: exact, the same on every run.
 * The kernel's grid covers 512 * 256 pixels per sweep and strides over the rest. */
int udaseg_calib_hist(const float* scores, const int64_t* target, int64_t pixels, int classes, int ldc, int probs,
                      const float* inv_temp, int bins, int64_t* tables, int64_t* counters, void* stream);
/* From the tables, in float64 and a fixed order (bins 0 .. bins - 1): n_b, a_b, q_b = count, correct, conf_q of bin b summed over the
 * classes (integers), N = sum n_b.  out: double [6] =
 *   N;  accuracy = sum a_b / N;  mean_conf = sum q_b / 2^24 / N;  ece = sum_b |a_b - q_b / 2^24| / N;
 *   mce = max over the non-empty bins of |a_b / n_b - q_b / 2^24 / n_b|;  gap = mean_conf - accuracy (positive: over-confident).
 * per_class: double [4][classes] = n_c, acc_c, conf_c, ece_c: the same quantities over the pixels PREDICTED as c.
 * Everything but the counts is NaN where its denominator is 0. */
int udaseg_calib_finish(const int64_t* tables, int classes, int bins, double* out, double* per_class, void* stream);
/* The negative log likelihood of the target under softmax(beta z) and its first two derivatives in beta.  Per pixel with a valid
 * target t, in fp32, d_j = z_j - m (m as above), e_j = expf(beta * d_j), S = sum e_j, A = sum e_j d_j, B = sum e_j d_j^2 (each as
 * four partial sums by j % 4):
 *   nll = logf(S) - beta * d_t;   mu = A / S;   g1 = mu - d_t  (= d nll / d beta);   g2 = B / S - mu * mu  (= d^2 nll / d beta^2)
 * A pixel whose three terms are not all finite is skipped and counted in counters[2].  sums: double [4] += n, sum nll, sum g1,
 * sum g2 over the counted pixels -- float64 sums in the fixed order of the loss kernels (thread: its pixels in order; block:
 * block_partial_rows; grid: one wave over the block partials), so two identical call sequences give identical bits.  sums
 * ACCUMULATES across calls (a loader pass is one sum); counters: int64 [3] += counted, void, non-finite.
 * partials: 4 * udaseg_seg_partials() doubles of scratch. */
int udaseg_calib_nll(const float* logits, const int64_t* target, int64_t pixels, int classes, int ldc, const float* inv_temp,
                     double* partials, double* sums, int64_t* counters, void* stream);
/* One guarded Newton step on beta = inv_temp[0] (the NLL is convex in beta, not in the temperature), in float64:
 *   if n > 0, sum g2 > 0, every sum finite and beta positive and finite:
 *     beta' = beta - sum g1 / sum g2, clamped to [beta / 4, 4 beta], then to [1 / 64, 64], stored as fp32;
 *   otherwise beta is unchanged.
 * state: double [4] = mean nll, mean g1 (NaN when n == 0), (double)(fp32 beta') - beta, state[3] + 1 (the number of steps taken
 * since the caller zeroed it).  sums is zeroed for the next pass. */
int udaseg_calib_step(double* sums, float* inv_temp, double* state, void* stream);

/* ---- class-balanced pseudo-labels of unlabelled target frames (CBST, Zou et al. 2018; an extension, the reference's phase 3 is
 * consistency only).  scores: padded NHWC fp32 [pixels][ldc], 16-byte aligned, ldc % 4 == 0, 0 < classes <= 32, classes <= ldc,
 * 0 < pixels < 2^31; only channels < classes are read.  ONE definition serves both pixel entry points:
 *   probs == 0 (logits z):        c^ = first maximum of z (udaseg_score_hist's comparison), m = z[c^],
 *                                 S = sum_{c < classes} expf(z_c - m), confidence p = 1 / S
 *   probs == 1 (probabilities q): c^ = first maximum of q, p = q[c^]      (udaseg_predict_finish's normalised accumulator)
 *   bin(p) = min((int)floorf(p * bins), bins - 1), bins in {256, 512, 1024, 2048, 4096}: edges k / bins exact, p == 1 in the top bin
 *   a pixel whose p is not finite (a NaN logit, a +inf logit, all logits -inf) or, with probs, outside [0, 1] or beside a NaN in
 *   any channel < classes is NON-FINITE: counted in no histogram cell, always labelled void, counted on its own.
 * hist[c^ * bins + bin(p)] += 1 for every finite pixel, nonfinite[0] += the others (int64 counters that ACCUMULATE across calls;
 * the caller zeroes them once, as for udaseg_score_hist). */
int udaseg_conf_hist(const float* scores, int64_t pixels, int classes, int ldc, int probs, int bins, int64_t* hist,
                     int64_t* nonfinite, void* stream);
/* per class c, in integers and IEEE float64 only: n_c = sum_b hist[c][b], need_c = (int64)ceil(portion[c] * (double)n_c),
 * k_c = the largest k in [0, bins - 1] with sum_{b >= k} hist[c][b] >= need_c (bins - 1 when n_c == 0; 0 if no k qualifies), then
 * thr_bins[c] = min(max(k_c, k_floor), k_cap) and support[c] = n_c.  portion: float64 [classes] ON THE DEVICE, each in (0, 1];
 * 0 <= k_floor <= k_cap <= bins - 1 is checked.  A pixel predicted as c is kept iff bin(p) >= thr_bins[c], i.e. p >= thr_bins[c] /
 * bins; k_cap is CBST's rule that no class has to be more confident than the cap.  Deterministic (fixed summation order). */
int udaseg_pseudo_thresholds(const int64_t* hist, int classes, int bins, const double* portion, int k_floor, int k_cap,
                             int32_t* thr_bins, int64_t* support, void* stream);
/* labels[p] = c^ if the pixel is finite and bin(p) >= thr_bins[c^], else void_label (classes <= void_label <= 255); conf (fp32
 * [pixels], may be NULL) receives p, or 0 for a non-finite pixel; counts (int64 [classes + 2], ACCUMULATES) += the kept pixels per
 * class, then the void pixels (the non-finite ones included), then the non-finite ones.  bins must be the value the thresholds
 * were made with. */
int udaseg_pseudo_labels(const float* scores, int64_t pixels, int classes, int ldc, int probs, int bins, const int32_t* thr_bins,
                         int void_label, uint8_t* labels, float* conf, int64_t* counts, void* stream);

/* ---- prototype-rectified pseudo-labels (ProDA, Zhang et al. 2021; an extension, the reference has no feature-space component).
 * feat: padded NHWC fp32 [pixels][ldf], 16-byte aligned, dim % 4 == 0, 4 <= dim <= 64, dim <= ldf, ldf % 4 == 0, 0 < pixels < 2^31;
 * only channels < dim are read.  0 < classes <= 32.
 * accumulate: for a pixel with labels[p] = c < classes and finite features sums[c][j] += f_j, sq[c] += sum_j f_j^2,
 * counts[c] += 1; a label >= classes adds to counts[classes]; a pixel with a non-finite feature in a channel < dim adds to
 * counts[classes + 1] and to nothing else (whatever its label).  sums: float64 [classes][dim], sq: float64 [classes], counts:
 * int64 [classes + 2]; all three ACCUMULATE across calls.  Every addition and every square is float64 (features are widened on
 * load; a pixel's squared norm is the float64 sum over ascending j of the exact squares, ONE number that is then added), so a
 * cell differs from any other float64 summation of the same n_c numbers by at most n_c 2^-52 sum|x|; the order of the atomic
 * additions is not fixed. */
int udaseg_proto_accumulate(const float* feat, int ldf, int dim, const uint8_t* labels, int64_t pixels, int classes, double* sums,
                            double* sq, int64_t* counts, void* stream);
/* One small block; IEEE float64 with every product, quotient and sum rounded on its own (no fused multiply-add), bit for bit
 * proto.update_mirror.  For a class c with n = counts[c] >= min_pixels (min_pixels >= 1): mean_j = sums[c][j] / (double)n,
 * s = max(sq[c] / (double)n - sum_j mean_j * mean_j, 0) (the sum over ascending j from 0.0); if seen[c] == 0: proto[c] = mean,
 * spread[c] = s, seen[c] = 1; else proto[c][j] = momentum * proto[c][j] + (1 - momentum) * mean_j and spread[c] likewise
 * (0 <= momentum <= 1).  Then last_counts = counts (int64 [classes + 2]) and, with clear != 0, sums = sq = counts = 0.
 * With tau_scale > 0: t = tau_scale * ((sum over the seen c, ascending, of spread[c]) / n_seen) and inv_tau[0] = (float)(1 / t)
 * when t is finite and positive, else 0; with tau_scale <= 0 inv_tau is left as the caller filled it (a fixed temperature).
 * proto: float64 [classes][dim], spread: float64 [classes], seen: int32 [classes], inv_tau: fp32 [1]. */
int udaseg_proto_update(double* sums, double* sq, int64_t* counts, int classes, int dim, double momentum, int64_t min_pixels,
                        double tau_scale, int clear, double* proto, double* spread, int32_t* seen, int64_t* last_counts,
                        float* inv_tau, void* stream);
/* out: fp32 [pixels][ldc], 16-byte aligned like scores ([pixels][ldc], ldc % 4 == 0, classes <= ldc); one pass, no atomics,
 * the same bits on every run.  Per pixel in fp32:
 *   probs == 0: m = the first maximum of the logits z, e_c = expf(z_c - m), S = sum_c e_c (udaseg_conf_hist's four chains),
 *               p_c = e_c * (1 / S);   probs == 1: p_c = the given probabilities
 *   d_c = sum_j (f_j - (float)proto[c][j])^2 (four chains, channel j in chain j % 4, folded as (s0 + s1) + (s2 + s3))
 *   over the seen classes d* = min d_c and u_c = expf(-(d_c - d*) * inv_tau[0]); u_c = 0 for an unseen class; u_c = 1 for all
 *   when no class is seen;   r_c = p_c * u_c, R = sum_c r_c, out_c = r_c / R;   channels classes .. ldc - 1 are written 0.
 * A row is NaN in every channel < classes when a feature in a channel < dim or a score in a channel < classes is not finite,
 * a probability lies outside [0, 1] (probs == 1), or R is zero or not finite: udaseg_pseudo_labels / udaseg_conf_hist with
 * probs == 1 then count the pixel as NON-FINITE.  inv_tau == 0 gives p renormalised over the seen classes; a very large
 * inv_tau gives the nearest seen prototype's class wherever its p is positive. */
int udaseg_proto_rectify(const float* feat, int ldf, int dim, const float* scores, int ldc, int classes, int probs,
                         const double* proto, const int32_t* seen, const float* inv_tau, int64_t pixels, float* out, void* stream);
/* ---- prototype contrast and structure losses (ProDA's structure learning; ProCA, Jiang et al. 2022; SePiCo, Xie et al. 2023): the
 * prototypes shape the features.  feat, dim, ldf, classes, proto, seen, inv_tau as above (proto is staged once per block as fp32).
 * Both entry points share ONE row routine, per pixel in fp32:
 *   d_c = sum_j (f_j - (float)proto[c][j])^2 (udaseg_proto_rectify's four chains, the same bits), d* = min d_c over the seen classes,
 *   a_c = -(d_c - d*) * inv_tau[0],  S = sum over the seen c of expf(a_c) (four chains, class c in chain c % 4),  L = logf(S),
 *   s_c = expf(a_c - L) for a seen class, 0 for an unseen one: the pixel's soft assignment to the seen prototypes.
 * assign: out fp32 [pixels][ldc] (16-byte aligned, classes <= ldc, ldc % 4 == 0) = s; channels classes .. ldc - 1 are written 0; a
 * row is NaN in every channel < classes when a feature in a channel < dim is not finite (the probs == 1 void convention of
 * udaseg_pseudo_labels, udaseg_soft_ce_fwd_bwd and udaseg_proto_rectify); while no class is seen s_c = 1 / classes for all
 * classes (rectify's "u = 1 for all").  One pass, no atomics, the same bits on every run. */
int udaseg_proto_assign(const float* feat, int ldf, int dim, int classes, int ldc, const double* proto, const int32_t* seen,
                        const float* inv_tau, int64_t pixels, float* out, void* stream);
/* The cross entropy of s against a target distribution over the classes, and its gradient with respect to the FEATURES, in one
 * pass; pixels = batch * pix_per_image.  Exactly one of labels and target is non-NULL:
 *   labels: uint8 [pixels] (hard):  t_c = [c == labels[p]]
 *   target: fp32 [pixels][ldt] probabilities, 16-byte aligned, classes <= ldt, ldt % 4 == 0 (soft; udaseg_proto_assign's and
 *           udaseg_proto_rectify's outputs are read in place):  t_c = target[c] for a seen class, 0 for an unseen one -- the mass on
 *           unseen classes is dropped
 *   T = sum_c t_c (four chains);  l = sum_c t_c * (-a_c) + T * L (a lane with t_c == 0 contributes exactly 0), for a hard label
 *   (d_y - d*) * inv_tau + L;  dl/df_j = 2 * inv_tau * sum_c (T * s_c - t_c) * P_cj, P the staged fp32 prototypes, summed over
 *   ascending c with fused multiply-adds.  The f_j terms of sum_c (T s_c - t_c)(f_j - P_cj) cancel identically and are not formed.
 *   The prototypes get no gradient: they are EMA state.
 * w_p = weight_px[p] * weight_img[p / pix_per_image] (fp32 product; either pointer NULL = 1).  A pixel is VOID -- loss exactly 0,
 * gradient exactly 0 in all ldf lanes -- for the first of these causes that holds:
 *   1. w_p is 0, negative or not finite;
 *   2. hard: the label is >= classes or its class is unseen; soft: a target lane < classes is not finite or outside [0, 1], or T == 0;
 *   3. a feature in a channel < dim is not finite.
 * stats (NULL = not wanted): int64 [4], ACCUMULATED with integer atomics: counted pixels, then the pixels void by cause 1, 2, 3.
 * While no class is seen every pixel falls under cause 1 or 2.  While inv_tau[0] == 0 (or is negative or NaN: no temperature yet)
 * the pixels are counted as usual and the loss and the gradient of every one of them are exactly 0.
 * loss, mean, denom, partials: as udaseg_soft_ce_fwd_bwd (sum_p w_p * l_p divided by pixels, by *denom from
 * udaseg_pixel_weight_sum -- *denom == 0: NaN -- or by 1; udaseg_seg_partials() doubles of scratch; a fixed-order sum without float
 * atomics: the same bits on every call, with and without dfeat).
 * dfeat fp32 [pixels][ldf] (NULL = not wanted; 16-byte aligned): the gradient for an upstream gradient of 1, divided like the
 * loss; lanes dim .. ldf - 1 are written 0. */
int udaseg_proto_contrast_fwd_bwd(const float* feat, int ldf, int dim, const uint8_t* labels, const float* target, int ldt,
                                  const float* weight_px, const float* weight_img, int batch, int64_t pix_per_image, int classes,
                                  const double* proto, const int32_t* seen, const float* inv_tau, int mean, const double* denom,
                                  double* partials, float* loss, float* dfeat, int64_t* stats, void* stream);

/* ---- cross-domain class mixing of a source and a target batch (DACS, Tranheden et al. 2021; ClassMix, Olsson et al. 2021; an
 * extension, the reference has no counterpart).  Integers only: every output is exact.
 * Selection, per source mask i, from the [n][256] table of udaseg_mask_hist_u8 (1 <= classes <= 32, min_pixels >= 1):
 *   present = the ascending list of c in [0, classes) with hist[i][c] >= min_pixels, P = its length, k = (P + 1) / 2;
 *   for j = 0 .. k-1:  r = word 0 of Philox4x32-10 with counter (j, 0, 0, 0) and key (keys[i][0], keys[i][1]) read as uint32,
 *                      t = j + (int)(((uint64)r * (P - j)) >> 32), swap present[j] and present[t];
 *   sel[i] = OR of 1 << present[j] for j < k, stored as the bit pattern of an int32 (bit 31 is class 31); P == 0 gives 0.
 * One launch for all n samples; nothing is read back. */
int udaseg_classmix_select(const int64_t* hist, int n, int classes, int64_t min_pixels, const int32_t* keys, int32_t* sel,
                           void* stream);
/* Mixing: src, tgt, out uint8 [n][h][w][3]; src_masks, tgt_masks (may be NULL), out_masks uint8 [n][h][w]; sel int32 [n]; boxes
 * (may be NULL) int32 [n][4] = (y0, x0, y1, x1), 0 <= y0 <= y1 <= h, 0 <= x0 <= x1 <= w, empty allowed; counts (may be NULL) int64
 * [n][3].  Per sample i and pixel (y, x), with s = src_masks[i][y][x]:
 *   m = (s < classes and (sel[i] >> s) & 1) or (boxes and y0 <= y < y1 and x0 <= x < x1)
 *   out[i][y][x] = m ? src[i][y][x] : tgt[i][y][x] (three bytes);  out_masks[i][y][x] = m ? s : (tgt_masks ? tgt_masks[i][y][x]
 *   : void_label);  counts[i] += {pixels with m, pixels without m whose output label is < classes, pixels without m whose output
 *   label is >= classes}: int64 counters that ACCUMULATE across calls, the three add up to h * w per call.
 * Refused (non-zero, nothing launched): classes outside 1..32, void_label outside classes..255, n, h or w <= 0, n*h*w >= 2^31,
 * a required pointer NULL, an output range that overlaps an input range or another output.  Two forms with identical bytes,
 * chosen per launch: 16 pixels per lane in 16-byte accesses when h * w % 16 == 0 and every frame and mask pointer is 16-byte
 * aligned, one pixel per lane otherwise. */
int udaseg_classmix_u8(const uint8_t* src, const uint8_t* src_masks, const uint8_t* tgt, const uint8_t* tgt_masks,
                       const int32_t* sel, const int32_t* boxes, int n, int h, int w, int classes, int void_label, uint8_t* out,
                       uint8_t* out_masks, int64_t* counts, void* stream);

/* ---- Fourier-domain style transfer of source frames to a target's style (FDA, Yang & Soatto 2020; the amplitude mix of Xu et al.
 * 2021; an extension, the reference has no counterpart), csrc/fda.hip.  Frames are uint8 [n][h][w][3].  With K = 2 bmax + 1,
 * 0 <= bmax <= (min(h, w) - 1) / 2, and ku = u + bmax, kv = v + bmax for the frequencies u, v in [-bmax, bmax]:
 *     out = src + Re(IDFT(D)),  D[u][v] = lam (|F_t[u][v]| - |F_s[u][v]|) F_s[u][v] / |F_s[u][v]| for |u|, |v| <= b, 0 elsewhere.
 * Twiddle tables: tw[k] = (cos, sin)(2 pi k / L) for k in [0, L), L = h and L = w, made on the host in float64; the analysis reads
 * them as float64 [L][2], the synthesis their float32 roundings; the index is (u * y) mod L in integers.  Every entry point
 * refuses (non-zero, nothing launched) a NULL required pointer, n, h or w <= 0, n*h*w >= 2^31, bmax outside its range and an output
 * range that overlaps an operand.  b and pick are device tables: the kernels clamp b[i] to [-1, bmax] and pick[i] to [0, m).
 *
 * Analysis, float64 from the exact integer pixels: coeffs[i][c][ku][kv] = sum_y sum_x frames[i][y][x][c] e^{-2 pi i (u y / h + v x / w)}
 * as (re, im), float64 [n][3][K][K][2], in two stages through rows_ws, float64 [n][3][h][K][2] (the sums over x).  No atomics: the
 * same frames give the same bits. */
int udaseg_fda_spectrum_u8(const uint8_t* frames, const double* tw_h, const double* tw_w, int n, int h, int w, int bmax,
                           double* rows_ws, double* coeffs, void* stream);
/* amps[j] = sqrt(re_j^2 + im_j^2) of count coefficients: the target side's float64 [m][3][K][K] table from its coefficients. */
int udaseg_fda_amplitude(const double* coeffs, int64_t count, double* amps, void* stream);
/* delta[i][c][ku][kv] = D / (h w) as (re, im), float32 [n][3][K][K][2].  coeffs: the source's; amps: float64 [m][3][K][K]; pick
 * int32 [n]: the row of amps that styles sample i; b int32 [n]: the sample's band half-width, -1 for none (delta is 0 outside
 * |u|, |v| <= b[i]); lam float32 [n] in [0, 1].  Where |F_s| <= 1e-9 * 255 * h * w the unit phasor F_s / |F_s| is taken as 1. */
int udaseg_fda_delta(const double* coeffs, const double* amps, const int32_t* pick, const int32_t* b, const float* lam, int n, int m,
                     int h, int w, int bmax, float* delta, void* stream);
/* Synthesis, float32: v = src + sum_{u, v} Re(delta[u][v] e^{+2 pi i (u y / h + v x / w)}) per value; field (float32 [n][h][w][3],
 * may be NULL) = v; out (uint8 [n][h][w][3], may be NULL; one of the two is required) = v rounded half to even, then clamped to
 * [0, 255]; counts (int64 [n][2], may be NULL, ACCUMULATES) += {values with v < 0, values with v > 255}.  cols_ws: float32
 * [n][3][K][w][2], the sums over v, written by a pre-kernel.  tw_h, tw_w: float32 [h][2], [w][2].  A sample with b[i] = -1 is
 * copied.  Two forms with identical bytes, chosen per launch: the frame tile is moved in 16-byte accesses when w % 16 == 0 and src
 * and out are 16-byte aligned, in bytes otherwise. */
int udaseg_fda_apply_u8(const uint8_t* src, const float* delta, const int32_t* b, const float* tw_h, const float* tw_w, int n, int h,
                        int w, int bmax, float* cols_ws, uint8_t* out, float* field, int64_t* counts, void* stream);

/* ---- rendering of label maps: colour masks, overlays, error maps, outlines, class counts in one pass (reference predict.py
 * create_colored_mask / create_overlay / test_model's class distribution, train.py _log_predictions).  Per pixel of image i of
 * n images [h][w], all tensors contiguous:
 *   L   = labels[i][y][x]: uint8 (labels_i64 == 0) or int64 (== 1; a value outside [0, 255] is read as 255; 8-byte aligned)
 *   c   = table[L], table uint8 [256][3] (the palette for L < classes, the void colour elsewhere: made by the caller)
 *   b   = the base pixel (base_kind, UDASEG_RENDER_BASE_*): NONE (base NULL); U8, a uint8 frame [n][h][w][3]; F32 / BF16, the
 *         model input, padded NHWC with 16-byte pixels ([n][h][w][4] fp32 / [n][h][w][8] bf16, 16-byte aligned), channel j
 *         de-normalised as clip(rint(x * denorm[j] + denorm[3 + j]), 0, 255): an fp32 multiply, an fp32 add (not fused), round
 *         half to even, NaN -> 0.  denorm: HOST float[6], std * 255 then mean * 255.
 *   k   = 3 if truth is given and void (has_ignore and truth == ignore_index, or truth >= classes after the same int64 rule;
 *         the comparison with ignore_index uses the raw int64 value), else 2 if truth is given and equals L, else 1 if
 *         L >= classes, else 0.  truth: NULL or the dtype and shape of labels.
 *   out = (b * (256 - alpha[k]) + c * alpha[k] + 128) >> 8 per channel in integers, alpha: HOST int32[4], each in [0, 256]
 *         (0 returns b, 256 returns c); out = c without a base.
 *   outline >= 0 (r | g << 8 | b << 16; -1: none): a pixel whose label differs from its left, right, upper or lower neighbour
 *         INSIDE image i gets that colour instead (the frame's edge is no outline).
 *   counts (NULL or int64 [n][256], ACCUMULATES): counts[i][L] += 1.  agreement (NULL or int64 [n][3], needs truth, ACCUMULATES):
 *         += the pixels with truth == L / truth valid and != L / truth void.
 * out: uint8 [n][h][w][3].  No operand needs more than its dtype's alignment beyond the two stated: labels, frame and output
 * of an image that does not start on a 4-byte boundary are moved in bytes.  0 < n <= 65535, h * w < 2^31 - 4, 1 <= classes <= 256. */
#define UDASEG_RENDER_BASE_NONE 0
#define UDASEG_RENDER_BASE_U8 1
#define UDASEG_RENDER_BASE_F32 2
#define UDASEG_RENDER_BASE_BF16 3
int udaseg_render_u8(const void* labels, const void* truth, int labels_i64, const void* base, int base_kind, const uint8_t* table,
                     int n, int h, int w, int classes, int has_ignore, int ignore_index, const int32_t* alpha, const float* denorm,
                     int outline, uint8_t* out, int64_t* counts, int64_t* agreement, void* stream);

/* ---- label boundary distances: band erosion, boundary weight maps, Boundary IoU / trimap counters (csrc/boundary.hip;
 * tests/_boundary_ref.py is the numpy mirror, every product is integers or a table lookup and is bit for bit).  A label map is n
 * images [h][w], contiguous: uint8 (labels_i64 == 0) or int64 (== 1; 8-byte aligned; a value outside [0, 255] reads as 255).
 * With has_ignore == 1 the pixels whose value (after that rule) equals ignore_index, in [0, 255], are VOID; with has_ignore == 0
 * no pixel is void and ignore_index is only range-checked.
 *   boundary pixel  p is a boundary pixel if some 4-neighbour q INSIDE the same image has L(q) != L(p) and neither p nor q is void.
 *                   The frame's edge is no boundary (the rule of udaseg_render_u8's outline); images never see each other.
 *   D2(p)           the minimum over the boundary pixels b of the same image of (py - by)^2 + (px - bx)^2
 *   d2(p)           D2(p) if D2(p) <= radius^2, else radius^2 + 1 ("far"; also when the image has no boundary pixel).  A boundary
 *                   pixel has d2 = 0; a void pixel has a d2 like any other.  0 <= radius <= 32.
 * The cap makes the two-pass form exact: g(y, x) = the smallest |dy| <= radius with (y + dy, x) a boundary pixel, else
 * radius + 1; D2(y, x) = min over |dx| <= radius with g(y, x + dx) <= radius of dx^2 + g(y, x + dx)^2.
 * Limits of every entry point, refused with a message before any launch: 0 < n <= 65535, h, w >= 1, h * w < 2^31,
 * 0 <= radius <= 32, ignore_index (and void_label) in [0, 255], 1 <= classes <= 255. */
/* (tile height << 16) | tile width of the launch at this radius: the counters' (stats != 0) or the other three products'. */
int udaseg_boundary_tile(int radius, int stats);
/* d2: int32 [n][h][w] = d2(p). */
int udaseg_boundary_d2(const void* labels, int labels_i64, int n, int h, int w, int radius, int has_ignore, int ignore_index,
                       int32_t* d2, void* stream);
/* out: float32 [n][h][w] = table[slot(p)]; table: DEVICE float32 [radius^2 + 3]; slot(p) = d2(p) (0 .. radius^2 + 1) for a pixel
 * that is not void, radius^2 + 2 for a void pixel.  The table's bits are copied, nothing is computed. */
int udaseg_boundary_lookup(const void* labels, int labels_i64, int n, int h, int w, int radius, int has_ignore, int ignore_index,
                           const float* table, float* out, void* stream);
/* out: uint8 [n][h][w] = void_label where p is not void and d2(p) <= radius^2, else L(p) (a void pixel keeps ignore_index).
 * counts (NULL or int64 [n][2], ACCUMULATES): counts[i] += {pixels of image i this call set to void_label, pixels of image i that
 * were void already}. */
int udaseg_boundary_erode(const void* labels, int labels_i64, int n, int h, int w, int radius, int has_ignore, int ignore_index,
                          int void_label, uint8_t* out, int64_t* counts, void* stream);
/* Band counters of two maps of one dtype and shape.  truth's void pixels are as above; a pixel of pred is void where pred equals
 * ignore_index OR truth is void there (has_ignore == 1).  The inner band of class c in a map M is {p : M(p) = c, p not void in M,
 * d2_M(p) <= radius^2}, d2_M taken of M with M's void pixels.
 *   stats  (int64 [classes][3], ACCUMULATES): stats[c] += {|band_T(c)|, |band_P(c)|, |band_T(c) n band_P(c)|}
 *   trimap (int64 [2], ACCUMULATES): += {pixels not void in truth with d2_T <= radius^2, those among them with pred == truth
 *          (pred not void)}
 * A label >= classes that is not void counts in no band of stats; it makes boundaries like any label and counts in trimap. */
int udaseg_boundary_stats(const void* pred, const void* truth, int labels_i64, int n, int h, int w, int radius, int classes,
                          int has_ignore, int ignore_index, int64_t* stats, int64_t* trimap, void* stream);

/* ---- connected components of label maps: region ids and areas, a sieve, per-class region statistics (csrc/regions.hip;
 * tests/_regions_ref.py is the numpy mirror, every product is integers and is compared for equality).  A label map is n images
 * [h][w], contiguous: uint8 (labels_i64 == 0) or int64 (== 1; 8-byte aligned; a value outside [0, 255] reads as 255).  With
 * has_ignore == 1 the pixels whose value (after that rule) equals ignore_index, in [0, 255], are VOID; with has_ignore == 0 no
 * pixel is void and ignore_index is only range-checked (the conventions of udaseg_boundary_*).
 *   adjacent   two pixels of the SAME image are adjacent if neither is void, they carry the same label, and they are 4-neighbours
 *              (connectivity == 4) or 8-neighbours (connectivity == 8).  Images never see each other; the frame's edge connects
 *              nothing.
 *   component  a class of the transitive closure of "adjacent".
 *   id(p)      the smallest y * w + x over the pixels of p's component: its first pixel in raster order.  -1 for a void pixel.
 *              This makes the result unique: the same on every run, whatever order the atomics land in.
 *   area(p)    the number of pixels of p's component; 0 for a void pixel.
 * Limits of every entry point, refused with a message before any launch: 0 < n <= 65535, h, w >= 1, h * w < 2^31, connectivity
 * 4 or 8, ignore_index (and void_label) in [0, 255], 1 <= classes <= 255. */
/* (tile height << 16) | tile width of the labelling: regions are first labelled per tile and then joined across the seams. */
int udaseg_regions_tile(void);
/* ids: int32 [n][h][w] = id(p).  area: int32 [n][h][w] = area(p), or NULL when only the ids are wanted.  The labelling itself
 * needs one int32 [n][h][w] beside ids (the sizes of the tile-local components, then the ids of their roots): area serves as it;
 * with area == NULL a stream-ordered allocation of that size is taken and released inside the call. */
int udaseg_regions_label(const void* labels, int labels_i64, int n, int h, int w, int connectivity, int has_ignore,
                         int ignore_index, int32_t* ids, int32_t* area, void* stream);
/* ids, area: what udaseg_regions_label wrote for these labels with the same has_ignore / ignore_index.  min_area: DEVICE int32
 * [256], a threshold per label, each >= 0.  out: uint8 [n][h][w] = void_label if p is not void and area(p) < min_area[L(p)],
 * else L(p) (a void pixel keeps ignore_index).  counts (NULL or int64 [n][3], ACCUMULATES): counts[i] += {pixels of image i set
 * to void_label, components removed, components kept}; a component is counted at its root pixel, where ids[p] == y * w + x. */
int udaseg_regions_sieve(const void* labels, int labels_i64, const int32_t* ids, const int32_t* area, int n, int h, int w,
                         int has_ignore, int ignore_index, const int32_t* min_area, int void_label, uint8_t* out, int64_t* counts,
                         void* stream);
/* stats (int64 [classes][34], ACCUMULATES): per class c < classes {components, pixels, hist[32]}, hist[floor(log2(area))] += 1
 * per component of label c, each counted at its root pixel.  A label >= classes that is not void counts nowhere. */
int udaseg_regions_stats(const void* labels, int labels_i64, const int32_t* ids, const int32_t* area, int n, int h, int w,
                         int classes, int has_ignore, int ignore_index, int64_t* stats, void* stream);
/* The same labelling of an int32 map [n][h][w] (4-byte aligned), for maps of more than 256 values such as a superpixel map: every
 * value >= 0 is a label of its own and a negative value is VOID; there is no ignore_index.  ids, area: as udaseg_regions_label
 * writes them (area NULL or int32 [n][h][w]); ids must not be labels itself.  The uint8 / int64 entry point is not changed by it:
 * the tile kernel is instantiated a third time with its labels as 32-bit words in LDS (48 KB of static LDS in place of 40 KB). */
int udaseg_regions_label_i32(const int32_t* labels, int n, int h, int w, int connectivity, int32_t* ids, int32_t* area,
                             void* stream);

/* ---- CRF refinement of class scores under the frame: mean-field inference of a dense CRF (Kraehenbuehl & Koltun 2011) with the
 * message passing restricted to a local window (ConvCRF, Teichmann & Cipolla 2018); an extension, the reference has no counterpart
 * (csrc/crf.hip; tests/_crf_ref.py is the numpy mirror, as plain loops over the neighbours).  No sort, no atomics, every sum in a
 * fixed order: two calls give the same bits.
 * Operands: scores fp32 [n][h][w][ldc] as scores_common.h describes (classes <= 32, classes <= ldc, ldc % 4 == 0; logits, or
 * probabilities with probs == 1); frames uint8 [n][h][w][3]; logp, q0, q, q_out fp32 [n][h][w][ldq], classes <= ldq, ldq % 4 == 0;
 * valid uint8 [n][h][w].  Every fp32 buffer is 16-byte aligned.
 * Parameters: radius R in 1..5, dilation d in 1..4 with R * d <= 10; w_app, w_smooth >= 0 and not both 0; theta_beta > 0 enters as
 * inv2b = fp32(1 / (2 theta_beta^2)), strength >= 0.  s_alpha, s_gamma: fp32 [(2R+1)^2], made on the host in float64 and rounded:
 *   S_alpha[dy+R][dx+R] = exp(-(dy^2 + dx^2) d^2 / (2 theta_alpha^2)), S_gamma the same with theta_gamma.
 *   valid     P0_i = softmax(s_i), or s_i / sum_c s_i with probs.  Pixel i is VALID if, over the channels < classes, its row is
 *             finite (logits), or every value lies in [0, 1] (so none is NaN) and the row sum is positive and finite (probs).
 *             log P0_i(c) = (s_c - max) - log sum exp(s - max) under logits, log(P0_i(c)) with probs; log 0 = -inf is kept.
 *   neighbour j = i + d * (dy, dx), |dy|, |dx| <= R, (dy, dx) != (0, 0), inside the SAME image and valid.  Images never see each
 *             other; the frame's edge contributes nothing.
 *   weight    col_ij = exp(-c2_ij * inv2b), c2_ij the integer squared RGB distance of the two frame pixels (exact in fp32);
 *             k_ij = w_app * S_alpha * col_ij + w_smooth * S_gamma;  Z_i = sum_j (w_app * S_alpha + w_smooth * S_gamma): the
 *             colour-free mass, so the frame's edge and void neighbours are compensated and a pixel whose neighbours all differ
 *             in colour receives little.
 *   message   m_i(c) = strength * (sum_j k_ij Q_j(c)) / Z_i, and 0 when Z_i == 0;  0 <= m <= strength.
 *   update    Q'_i = softmax_c(log P0_i(c) + m_i(c)): Potts compatibility, a Jacobi sweep (every Q_j is the previous sweep's).
 * An invalid pixel has valid == 0, sends no message, carries no mass, and its rows of q0 and q_out are NaN in the channels
 * < classes (udaseg_proto_rectify's void row); its logp row is NaN too and is never read.  Channels classes .. ldq - 1 of logp, q0
 * and q_out are written 0 on every call.  Refused with a message before any launch: a parameter outside the ranges above, n <= 0,
 * h, w < 1, h * w >= 2^31, more than 2^31 - 1 tiles, a NULL or misaligned pointer, q_out == q. */
/* (tile height << 16) | tile width of udaseg_crf_step's blocks at this radius and dilation (the height depends on the dilation: a
 * thread owns two pixels `dilation` rows apart); 0 for parameters outside their ranges. */
int udaseg_crf_tile(int radius, int dilation);
/* scores -> logp = log P0, q0 = P0 and the valid flags.  One streaming pass. */
int udaseg_crf_prepare(const float* scores, int ldc, int classes, int probs, int64_t pixels, float* logp, float* q0, int ldq,
                       uint8_t* valid, void* stream);
/* One sweep q -> q_out.  logp and valid: what udaseg_crf_prepare wrote for these scores. */
int udaseg_crf_step(const float* logp, const float* q, const uint8_t* valid, const uint8_t* frames, int n, int h, int w, int classes,
                    int ldq, int radius, int dilation, const float* s_alpha, const float* s_gamma, float w_app, float w_smooth,
                    float inv2b, float strength, float* q_out, void* stream);

/* ---- window votes of label maps and active label acquisition (RIPU, Xie et al., CVPR 2022; an extension, the reference has no
 * counterpart; csrc/window.hip; tests/_active_ref.py is the numpy mirror).  A label map is n images [h][w], contiguous: uint8
 * (labels_i64 == 0) or int64 (== 1; 8-byte aligned; a value outside [0, 255] reads as 255), with has_ignore / ignore_index as for
 * udaseg_boundary_*.
 *   void         a pixel is VOID if it equals ignore_index (has_ignore == 1) OR its label is >= classes.
 *   W(p)         the pixels q of the same image with |qy - py| <= radius, |qx - px| <= radius, inside the image and not void.  The
 *                window is clipped at the frame, never padded; images never see each other.
 *   n(p), n_c(p) |W(p)|, and the number of q in W(p) with L(q) = c.
 *   mode(p)      the class with the largest n_c(p); among tied classes the centre's own label if it is one of them (the centre
 *                is then not void), else the smallest class index.  With n(p) = 0 there is no mode.
 *   agreement(p) float32(n_mode(p)) / float32(n(p)), one correctly rounded fp32 division of two exact integers; 0 where n(p) = 0.
 *   impurity(p)  (n log n - sum_c n_c log n_c) / (n log(classes)), with 0 log 0 = 0: the entropy of the window's label histogram
 *                over log(classes), in [0, 1]; 0 where n(p) <= 1.  As computed: T[m] = fp32(m log m) comes from a DEVICE fp32 table
 *                [(2 radius + 1)^2 + 1] the caller passes (made on the host in float64 and rounded once; T[0] = T[1] = 0);
 *                S = sum over c = 0 .. classes - 1, ascending, of T[n_c] in fp32;  impurity = clamp((T[n] - S) / (float32(n) *
 *                fp32(log(classes))), 0, 1): one subtraction, one product, one division.  A window of one class gives exactly 0.
 *   entropy(q)   -sum_c p_c log p_c / log(classes) of softmax(scores), or of the probabilities as they are with probs == 1:
 *                udaseg_entropy_loss's map (lp_c = (z_c - max) - log sum exp(z - max), p_c = exp(lp_c); a term with p_c = 0 is 0;
 *                the terms are added in ascending class order).
 *   uncertainty(p)  (sum of entropy(q) over q in W(p)) / float32(n(p)), 0 where n(p) = 0.  The sum is taken DIRECTLY: per row of the
 *                window its 2 radius + 1 terms left to right (0 for a position outside W), then the 2 radius + 1 row sums top to
 *                bottom.  No running add / subtract.
 *   A(p)         min(A0(p), 1) with A0(p) = impurity(p) * uncertainty(p) for kind 0 (RIPU), impurity(p) for kind 1,
 *                uncertainty(p) for kind 2.  The cap matters: the fp32 entropy of a uniform row can be 1 + 1 ulp.
 *   key(p)       1.0f - A(p); but -1.0f where p is void, p is excluded (exclude[p] != 0), A0(p) <= 0 or A0(p) is not finite.
 *                The CANDIDATES are the pixels with key >= 0; their keys lie in [0, 1], what udaseg_kth_* takes.
 * Limits, refused with a message before any launch: 0 < n <= 65535, h, w >= 1, h * w < 2^31, 0 <= radius <= 16,
 * 2 <= classes <= 32, ignore_index (and void_label) in [0, 255].  Two calls give the same bits. */
/* (tile height << 16) | tile width of the window kernels' launch at this radius. */
int udaseg_window_tile(int radius);
/* out: uint8 [n][h][w] = mode(p) for a pixel that is not void; a void pixel gets void_label, unless fill_void == 1 and n(p) > 0:
 * then it gets mode(p).  agreement (NULL or fp32 [n][h][w]) = agreement(p), of void pixels too.  counts (NULL or int64 [n][3],
 * ACCUMULATES): counts[i] += {pixels not void whose label changed, void pixels filled, void pixels left}. */
int udaseg_window_mode(const void* labels, int labels_i64, int n, int h, int w, int radius, int classes, int has_ignore,
                       int ignore_index, int fill_void, int void_label, uint8_t* out, float* agreement, int64_t* counts,
                       void* stream);
/* out: fp32 [n][h][w] = impurity(p), of void pixels too. */
int udaseg_window_impurity(const void* labels, int labels_i64, int n, int h, int w, int radius, int classes, int has_ignore,
                           int ignore_index, const float* table, float* out, void* stream);
/* One pass over padded NHWC scores (scores_common.h: [pixels][ldc] fp32, 16-byte aligned, classes <= ldc, ldc % 4 == 0; the
 * channels >= classes are never looked at): labels uint8 [pixels] = the first maximal class, entropy fp32 [pixels] = entropy(q).
 * A row with a non-finite score below `classes` (or whose entropy is not finite) gets label 255 and entropy 0.  counters (int64
 * [2], ACCUMULATES) += {finite rows, non-finite rows}. */
int udaseg_acquire_prepare(const float* scores, int ldc, int classes, int probs, int64_t pixels, uint8_t* labels, float* entropy,
                           int64_t* counters, void* stream);
/* labels uint8 [n][h][w] (a label >= classes, 255 among them, is void), entropy fp32 [n][h][w] (read at pixels that are not void
 * only), exclude NULL or uint8 [n][h][w].  score fp32 [n][h][w] = A(p), or 0 where key(p) = -1; key fp32 [n][h][w] = key(p). */
int udaseg_acquire_score(const uint8_t* labels, const float* entropy, const uint8_t* exclude, int n, int h, int w, int radius,
                         int classes, int kind, const float* table, float* score, float* key, void* stream);
/* Per cell of the grid of cell_h x cell_w rectangles anchored at (0, 0) (the last row / column of cells is smaller where the image
 * is no multiple): a = (sum over the cell's candidates of (1.0f - key), in float64) / (pixels of the cell inside the image), rounded
 * to fp32 once; cell_key fp32 [n][ceil(h / cell_h)][ceil(w / cell_w)] = 1.0f - a, or -1.0f for a cell without a candidate.  One
 * wave per cell, partial sums folded in a fixed order. */
int udaseg_acquire_cells(const float* key, int n, int h, int w, int cell_h, int cell_w, float* cell_key, void* stream);
/* key fp32 [n][items_per_image], thresholds DEVICE fp32 [n]: mask[i][j] |= 1 where key[i][j] >= 0 and key[i][j] <= thresholds[i]
 * (uint8 [n][items_per_image]; other entries keep their value).  counts (NULL or int64 [n][2], ACCUMULATES): counts[i] +=
 * {items selected here whose mask was 0 before, candidates}.  0 < items_per_image < 2^31. */
int udaseg_acquire_select(const float* key, const float* thresholds, int n, int64_t items_per_image, uint8_t* mask, int64_t* counts,
                          void* stream);
/* mask uint8 [n][h][w] |= 1 on every pixel, void or not, whose cell of udaseg_acquire_cells's grid has cell_mask != 0. */
int udaseg_acquire_expand(const uint8_t* cell_mask, int n, int h, int w, int cell_h, int cell_w, uint8_t* mask, void* stream);

/* ---- superpixels: an integer SLIC (Achanta et al. 2012) whose superpixels are 4-connected, the majority vote of a label map per
 * superpixel, the mean of a score map per superpixel, a gather of a per-superpixel table; an extension, the reference has no
 * counterpart (csrc/superpixels.hip; tests/_superpixels_ref.py is the numpy mirror, compared for equality).  EVERYTHING IS INTEGER
 * ARITHMETIC: two runs give the same bits in whatever order the atomics land, and there is no float atomic.
 * Inputs: frames uint8 [n][h][w][3], the three channels used as they are (the colour space is the caller's; no Lab conversion);
 * step S in [2, 64]; compactness m in [1, 1024]; iterations T in [1, 64]; min_area >= 0; 0 < n <= 65535, 1 <= h, w <= 32768,
 * h * w < 2^31.  Every entry point refuses anything else with a message that names the argument, before any launch.
 *   grid     gh = ceil(h / S), gw = ceil(w / S), K = gh * gw clusters per image; cluster k = gy * gw + gx belongs to cell (gy, gx),
 *            the pixels with y / S == gy and x / S == gx.
 *   centres  int32 [n][K][6] = (Y, X, C0, C1, C2, count), Y .. C2 in units of 1/16.  Start: y0 = min(gy * S + S / 2, h - 1)
 *            (integer division), x0 likewise, centre = 16 * (y0, x0, frame[y0][x0][:]), count = 0.  NO GRADIENT PERTURBATION of the
 *            seeds is applied (SLIC moves a seed to the lowest gradient of its 3 x 3 neighbourhood; this rule does not).
 *   assign   a pixel (y, x) of cell (gy, gx) considers the clusters of the up to 9 cells (gy + dy, gx + dx), dy, dx in {-1, 0, 1},
 *            that lie inside the grid, and takes the smallest
 *                D = S^2 * sum_i (16 c_i - C_i)^2 + m^2 * ((16 y - Y)^2 + (16 x - X)^2)
 *            in 64-bit integers (D < 2.1e13 for S <= 64, m <= 1024); among equal D the smallest k.  A cluster's pixels therefore lie
 *            in the 3 x 3 cells around its own: count <= 9 S^2 <= 36864.
 *   update   per cluster the integer sums of y, x, c0, c1, c2 over its pixels and their count (36864 * 32767 < 2^31: int32); each
 *            component becomes (16 * sum + count / 2) / count, in 64 bits with integer division.  A cluster with count == 0 keeps its
 *            centre.  The count is stored in either case.
 *   iterate  T times: labels = assign(centres), then centres = update(labels).  The centres returned are the last update's.
 *   connect  Take the 4-connected components of the last labels; a component's root is its first pixel in raster order, its area its
 *            pixel count.  The MAIN component of cluster k: the one that holds pixel (0, 0) if that carries label k, else the
 *            component of k with the largest area, ties to the smallest root.  A component is KEPT if it is main and (area >=
 *            min_area or it holds pixel (0, 0)).  Every other component is ABSORBED: it takes the final label of the pixel just
 *            before its root -- (y, x - 1) if x > 0, else (y - 1, 0) -- which belongs to a component with a smaller root; applied
 *            transitively, the chain of roots strictly decreases and ends at a kept component.
 *            With min_area == 0: every non-empty cluster keeps its main component, and every final superpixel is 4-connected (a
 *            chain links adjacent components up to a kept one, so what a kept component gathers is connected through it).  With
 *            min_area > 0 whole clusters may vanish (on a pure-noise frame nearly all do); the connectivity still holds.
 *   ids      int32 [n][h][w]: the final cluster index in [0, K) of every pixel.
 *   counts   NULL or int64 [n][4], ACCUMULATES per image {components found, components absorbed, pixels whose label changed,
 *            clusters that own at least one pixel at the end}. */
int udaseg_superpixel_slic(const uint8_t* frames, int n, int h, int w, int step, int compactness, int iterations, int min_area,
                           int32_t* ids, int32_t* centres, int64_t* counts, void* stream);
/* ONE iteration from given centres (int32 [n][K][6] as udaseg_superpixel_slic or this call wrote them; updated in place).  labels:
 * NULL, or int32 [n][h][w] that receives the assignment the update was made from. */
int udaseg_superpixel_assign(const uint8_t* frames, int n, int h, int w, int step, int compactness, int32_t* centres,
                             int32_t* labels, void* stream);
/* The connect step alone on a map of cluster indices of the grid of `step`: labels int32 [n][h][w], every value in [0, K); ids and
 * counts as above (ids may be labels itself).  A value outside [0, K) is no cluster of the grid: a negative pixel stays as it is
 * and belongs to no component, a component of a value >= K is kept as it is, and a component absorbed into either takes that value. */
int udaseg_superpixel_connect(const int32_t* labels, int n, int h, int w, int step, int min_area, int32_t* ids, int64_t* counts,
                              void* stream);
/* The vote of a label map per superpixel.  ids int32 [n][h][w] with 0 <= ids < clusters (a pixel outside that range belongs to no
 * superpixel: it counts nowhere and comes out void); masks uint8 (masks_i64 == 0) or int64 (== 1, a value outside [0, 255] reads as
 * 255) [n][h][w]; a pixel whose mask value is ignore_index (with has_ignore == 1) or >= classes is VOID and is not counted.
 *   T[k][c]      the pixels of superpixel k whose mask value is class c; labelled(k) = sum_c T[k][c]; size(k) = the pixels of k.
 *   winner(k)    the class with the largest T[k][c], ties to the smallest class.
 *   out(p)       winner(k) for a pixel p of k if labelled(k) > 0 and (double)T[k][winner] >= (double)min_share * (double)labelled(k)
 *                and (double)labelled(k) >= (double)min_cover * (double)size(k); void_label otherwise.  uint8 [n][h][w].
 *   counts       NULL or int64 [n][3], ACCUMULATES {labelled pixels that come out with another class, void pixels that come out
 *                with a class, labelled pixels that come out void}.
 * 1 <= clusters <= 2^28, 1 <= classes <= 255, ignore_index and void_label in [0, 255], min_share and min_cover in [0, 1]. */
int udaseg_superpixel_vote(const int32_t* ids, const void* masks, int masks_i64, int n, int h, int w, int clusters, int classes,
                           int has_ignore, int ignore_index, float min_share, float min_cover, int void_label, uint8_t* out,
                           int64_t* counts, void* stream);
/* The mean of fp32 values [n][h][w] per superpixel: a pixel counts if its value is finite and lies in [0, 1] (and its id in
 * [0, clusters)); q = rint(v * 2^24), exact because scaling by a power of two is; the sums are int64.  mean fp32 [n][clusters] =
 * fp32((double)sum / ((double)count * 2^24)), or -1 where no pixel counts: the form udaseg_kth_hist and udaseg_acquire_select take. */
int udaseg_superpixel_mean(const float* values, const int32_t* ids, int n, int h, int w, int clusters, float* mean, void* stream);
/* mask uint8 [n][h][w]: mask[p] |= table[ids[p]] for every pixel with an id in [0, clusters); table uint8 [n][clusters]. */
int udaseg_superpixel_gather(const int32_t* ids, const uint8_t* table, int n, int h, int w, int clusters, uint8_t* mask,
                             void* stream);

/* ---- discriminator tail + adversarial BCE: discriminator.py:37-42, losses.py:18-51 ---- */
/* pooled[n][c] = mean over hw of z; p[n] = sigmoid(dot(pooled[n], w) + b).  partial: [n][splits][c] floats */
int udaseg_gap_splits(int hw);
int udaseg_gap_linear_sigmoid_fwd(const float* z, const float* w, const float* b, float* partial, float* pooled,
                                  float* p, int n, int hw, int c, void* stream);
/* given dp[n]: dw (+)=, db (+)=, dz[n][hw][c] = dp*p*(1-p)*w[c]/hw broadcast */
int udaseg_gap_linear_sigmoid_bwd(const float* dp, const float* p, const float* pooled, const float* w, float* dz,
                                  float* dw, float* db, int n, int hw, int c, int accumulate_param, void* stream);
/* feature-level discriminator tail Conv2d(c,1,1) -> AdaptiveAvgPool2d(1) (src/models/uda.py:22-23):
 * logit[n] = dot(mean_hw z[n], w) + b  (no sigmoid; that design applies BCE-with-logits to real logits) */
int udaseg_gap_linear_fwd(const float* z, const float* w, const float* b, float* partial, float* pooled, float* logit, int n,
                          int hw, int c, void* stream);
int udaseg_gap_linear_bwd(const float* dlogit, const float* pooled, const float* w, float* dz, float* dw, float* db, int n,
                          int hw, int c, int accumulate_param, void* stream);
/* loss (+)= weight * mean(softplus(x) - x*label)   (BCEWithLogits on whatever x is: reference feeds probabilities) */
int udaseg_bce_logits_fwd(const float* x, int n, float label, float weight, float* loss, int accumulate, void* stream);
/* dx = (*grad_out) * weight * (sigmoid(x) - label) / n */
int udaseg_bce_logits_bwd(const float* x, int n, float label, float weight, const float* grad_out, float* dx,
                          int accumulate, void* stream);
/* the same with a per-sample target vector (nn.BCEWithLogitsLoss()(x, y): src/models/uda.py:85,96; trainer_phases.py:157) */
int udaseg_bce_logits_target_fwd(const float* x, const float* target, int n, float weight, float* loss, int accumulate,
                                 void* stream);
int udaseg_bce_logits_target_bwd(const float* x, const float* target, int n, float weight, const float* grad_out, float* dx,
                                 int accumulate, void* stream);

/* ---- Adam: torch.optim.Adam(...).step() at train.py:344,461; adversarial_trainer.py:56-59,98,114 ----
 * flat fp32 arrays; bc1 = 1-beta1^t, bc2 = 1-beta2^t computed by the caller.  beta1 / beta2 are doubles: the kernel multiplies by
 * 1-beta1 and 1-beta2, which are formed in double and rounded to fp32 once (formed from fp32 betas they are off by up to 1.3e-5). */
int udaseg_adam_flat(float* p, const float* g, float* m, float* v, int64_t count, float lr, double beta1, double beta2,
                     float eps, float bc1, float bc2, void* stream);

/* ---- global-norm gradient clipping: torch.nn.utils.clip_grad_norm_(params, max_norm) at src/models/unsupervised_trainer.py:144,
 *      without a host round trip.  sumsq: *out (= or +=, by `accumulate`) the fp64 sum of g[i]^2; per-block partials are combined
 *      in a fixed order (no floating-point atomics: the same data give the same bits).  partials: UDASEG_SUMSQ_PARTIALS + 1
 *      doubles owned by the caller and zeroed ONCE when allocated (the last word is the kernel's arrival counter, which it
 *      clears itself); calls that share it must be ordered on one stream.
 *      scale_by_clip: g[i] *= min(1, max_norm / (sqrt(*sumsq) + eps)), the coefficient formed in fp64 on the device and the
 *      product rounded once; a coefficient >= 1 writes nothing, a NaN norm makes every g[i] NaN (as torch does with
 *      error_if_nonfinite=False). ---- */
#define UDASEG_SUMSQ_PARTIALS 256
int udaseg_sumsq_f32(const float* g, int64_t count, double* partials, double* out, int accumulate, void* stream);
int udaseg_scale_by_clip_f32(float* g, int64_t count, const double* sumsq, float max_norm, float eps, void* stream);

/* ---- mean teacher (Tarvainen & Valpola 2017): t[i] <- t[i] + (1 - decay) * (s[i] - t[i]) over two flat fp32 arrays in one
 *      streaming pass of 12 B per element.  Arithmetic contract: w = (float)(1.0 - decay), formed in double and rounded once;
 *      d = s[i] - t[i] in fp32; t[i] = fmaf(w, d, t[i]) (fused: one rounding of the result).  decay == 0 is a copy, t[i] = s[i]
 *      bit for bit; decay == 1 leaves t unchanged; where s[i] == t[i] the element keeps its bits; zero padding lanes of both
 *      arrays therefore stay zero.  0 <= decay <= 1, anything else (a NaN included) is UDASEG_E_BADARG.
 *      dist2 (may be NULL): *dist2 (= or +=, by `accumulate`) the fp64 sum of ((double)s[i] - (double)t_new[i])^2 of the same
 *      pass, combined in a fixed order as udaseg_sumsq_f32 combines its sum (same bits on every run); partials: that entry
 *      point's UDASEG_SUMSQ_PARTIALS + 1 doubles of scratch under the same rules, required only with dist2.
 *      t, s: 4-byte aligned; 16-byte vector loads and stores when both are 16-byte aligned, the scalar form otherwise;
 *      overlapping ranges are UDASEG_E_BADARG. ---- */
int udaseg_ema_flat(float* t, const float* s, int64_t count, double decay, double* partials, double* dist2, int accumulate,
                    void* stream);

/* ---- strong augmentation of the phase-3 step (src/models/augmentation.py:40-88, applied per image on the host at
 *      src/models/unsupervised_trainer.py:100-114): uint8 RGB frames [n][h][w][3] + one parameter record per (view, sample)
 *      -> `views` (1 or 2) normalised, channel-padded NHWC model inputs [views][n][h][w][cpad].  The pipeline (D4, Gaussian
 *      noise, blur, shift-scale-rotate, one of sharpen / emboss / brightness-contrast, HSV shift, A.Normalize) is defined in
 *      INTEGRATION.md, "Phase 3"; all randomness except the per-pixel noise is in the records, the noise is Philox4x32-10 keyed
 *      by the record.  table: int32 [views][n][UDASEG_STRONG_AUG_WORDS], floats stored as their bit patterns:
 *        0 flags (1 noise, 2 blur, 4 affine, 8 stage 5, 16 HSV)   1 D4 code (udaseg_prepare_batch_u8's)   2 blur kind (0 box,
 *        1 median, 2 motion)   3 blur size (3 or 5)   4 motion direction (0 horizontal, 1 vertical, 2 main diagonal, 3 anti-
 *        diagonal)   5 stage-5 kind (0 sharpen, 1 emboss, 2 brightness-contrast; 3 CLAHE: the _clahe entry points)   6,7 Philox key   8 sigma   9..14 inverse
 *        affine map (row-major 2 x 3, output pixel -> source position)   15,16 stage-5 parameters (alpha, lightness | alpha,
 *        strength | brightness, contrast)   17,18,19 hue / saturation / value shifts   20.. not read by the kernels
 *      mid: fp32 scratch [views][n][h][w][4], needed when source_pass != 0; pass source_pass = 0 when no record has noise or
 *      blur (one launch instead of two).  A record with flags == 0 gives udaseg_prepare_batch_u8's output bit for bit.
 *      Transposing D4 codes need h == w (the bit is ignored otherwise).  mean255 / inv_std255: HOST arrays of 3 floats. ---- */
#define UDASEG_STRONG_AUG_WORDS 32
int udaseg_strong_aug_u8(const uint8_t* images, const int32_t* table, int views, int n, int h, int w, float* mid,
                         const float* mean255, const float* inv_std255, void* out_images, int cpad, int out_bf16,
                         int source_pass, void* stream);
/* the generator's raw words, for tests: out[4i..4i+3] = Philox4x32-10(counter = counters[4i..4i+3], key = keys[2i..2i+1]) */
int udaseg_philox4x32_debug(const int32_t* counters, const int32_t* keys, int32_t* out, int count, void* stream);

/* ---- labelled training augmentation (src/models/augmentation.py:8-38, applied per sample on the host there): uint8 RGB
 *      frames [n][h][w][3] + uint8 masks [n][h][w] (may be NULL, with out_masks) + one parameter record per sample -> the
 *      normalised, channel-padded NHWC model input [n][h][w][cpad] and int64 masks [n][h][w], image and mask carried through
 *      the same geometry.  The pipeline is defined in INTEGRATION.md, "Training augmentation": the strong pipeline's stages
 *      plus one of optical / grid / elastic distortion, composed with the affine map into one gather (image bilinear, mask
 *      nearest; the label value passes through unchanged).  table: int32 [n][UDASEG_TRAIN_AUG_WORDS]:
 *        0..31 the record of udaseg_strong_aug_u8, flag bit 32 of word 0 = distortion   32 distortion kind (1 optical, 2 grid,
 *        3 elastic)   33,34,35 optical k, dx, dy   36..41 grid x steps   42..47 grid y steps   48 elastic alpha
 *        50,51 Philox key of the elastic field   the rest reserved, not read
 *      mid: fp32 scratch [n][h][w][4], needed when source_pass != 0 (a record with noise or blur).  field: float2 [n][h][w],
 *      read for the samples on elastic; field_pass != 0 fills it first (udaseg_elastic_field_f32's kernel) and then needs
 *      gauss_weights: a HOST array of 2 radius + 1 fp32 taps, radius <= UDASEG_ELASTIC_MAX_RADIUS.  A sample on elastic
 *      without a field buffer is refused by the Python binding; the kernels then leave its distortion out.  At most three
 *      launches, no synchronisation.  A record with flags == 0 gives udaseg_prepare_batch_u8's output bit for bit, image and
 *      mask.  mean255 / inv_std255: HOST arrays of 3 floats.  Transposing D4 codes need h == w (the bit is ignored otherwise).
 *      udaseg_elastic_field_f32: the field pass alone (samples not on elastic are left untouched): field[n][y][x] = the
 *      separable Gaussian (reflect-101 at any distance) of (2 u0 - 1, 2 u1 - 1), u = the first two uniforms of Philox4x32-10
 *      at counter (y w + x, 1, 0, 0) under the record's key. ---- */
#define UDASEG_TRAIN_AUG_WORDS 64
#define UDASEG_ELASTIC_MAX_RADIUS 18
int udaseg_train_aug_u8(const uint8_t* images, const uint8_t* masks, const int32_t* table, int n, int h, int w, float* mid,
                        float* field, const float* gauss_weights, int radius, const float* mean255, const float* inv_std255,
                        void* out_images, int cpad, int out_bf16, int64_t* out_masks, int source_pass, int field_pass,
                        void* stream);
int udaseg_elastic_field_f32(const int32_t* table, int n, int h, int w, const float* gauss_weights, int radius, float* field,
                             void* stream);

/* ---- CLAHE in both augmentation pipelines (the first child of the last OneOf of src/models/augmentation.py:29-34 and :70-79):
 *      stage-5 kind 3 of a record, flag 8 (stage 5) set, the clip limit (>= 1) in word 15.  Contrast-limited histogram
 *      equalisation of the Lab lightness of the image after stage 4 / 4b on a fixed 8 x 8 grid of tiles; the mask is never
 *      touched.  Defined in INTEGRATION.md, "CLAHE".  Frame sides must be multiples of 8.
 *      udaseg_clahe_lut_u8: the table pass alone, for `words` = 32 (strong records, views 1 or 2) or 64 (training records,
 *      views 1): lut[views][n][8][8][256] uint8, written for the samples on CLAHE and left untouched for the others.  mid /
 *      field: the intermediates of the source / field pass as the full calls hold them, or NULL (a record with noise or blur
 *      then reads the frame itself, a record on elastic is evaluated without its distortion).
 *      udaseg_strong_aug_clahe_u8 / udaseg_train_aug_clahe_u8: udaseg_strong_aug_u8 / udaseg_train_aug_u8 with the table
 *      buffer (views * n * UDASEG_CLAHE_LUT_BYTES bytes): every pass of the call, the table pass after the source pass, one
 *      launch more than the plain entry point and no synchronisation.  Records on the other kinds give the plain entry
 *      points' output bit for bit.  The plain entry points do not know kind 3. ---- */
#define UDASEG_CLAHE_GRID 8
#define UDASEG_CLAHE_LUT_BYTES (8 * 8 * 256)
int udaseg_clahe_lut_u8(const uint8_t* images, const int32_t* table, int words, int views, int n, int h, int w, const float* mid,
                        const float* field, uint8_t* lut, void* stream);
int udaseg_strong_aug_clahe_u8(const uint8_t* images, const int32_t* table, int views, int n, int h, int w, float* mid,
                               const float* mean255, const float* inv_std255, void* out_images, int cpad, int out_bf16,
                               int source_pass, uint8_t* lut, void* stream);
int udaseg_train_aug_clahe_u8(const uint8_t* images, const uint8_t* masks, const int32_t* table, int n, int h, int w, float* mid,
                              float* field, const float* gauss_weights, int radius, const float* mean255,
                              const float* inv_std255, void* out_images, int cpad, int out_bf16, int64_t* out_masks,
                              int source_pass, int field_pass, uint8_t* lut, void* stream);

/* ---- device-side input pipeline: uint8 RGB HWC images [n][h][w][3] (+ uint8 masks [n][h][w], may be NULL) ->
 *      normalised, D4-augmented, channel-padded NHWC model input (fp32, or bf16 when out_bf16) and int64 masks.
 *      Replaces the per-sample host work of src/data/dataset.py:116-138 with the geometric part of
 *      src/models/augmentation.py:11-13 (RandomRotate90 / Flip / Transpose = one D4 element per sample) and
 *      A.Normalize() (augmentation.py:36): out = (x - mean255[c]) * inv_std255[c] in fp32.
 *      d4[n] (may be NULL = identity): bit0 transpose, bit1 flip rows, bit2 flip columns, applied in that order.
 *      mean255 / inv_std255 are HOST arrays of 3 floats.  Transposing codes need h == w. ---- */
int udaseg_prepare_batch_u8(const uint8_t* images, const uint8_t* masks, const int32_t* d4, int n, int h, int w,
                            const float* mean255, const float* inv_std255, void* out_images, int cpad, int out_bf16,
                            int64_t* out_masks, int square_checked, void* stream);

/* ---- frame ingest (csrc/resize.hip): decoded uint8 frames and label masks of ANY size -> the uint8 batch at the model's size
 *      that the entry points above take, and the per-mask class statistics.  The reference does this per sample on the host:
 *      cv2.resize(INTER_AREA) in src/data/target_dataset.py:46-48, Resize(Config.IMAGE_SIZE) in src/models/predict.py:91-98,
 *      the mask reads of src/data/dataset.py:48-111.  Sizes are (height, width): H x W source, h x w destination.
 *      n, h <= 65535, H*h and W*w < 2^31. ---- */
/* Area resize, exact: src [n][H][W][3] -> dst [n][h][w][3], H >= h >= 1 and W >= w >= 1 (an enlargement on either axis is
 * refused: use udaseg_resize_aa_u8).  Per channel, in integer units: destination row i covers [i*H, (i+1)*H), source row s
 * covers [s*h, (s+1)*h), wy(i,s) = the length of their overlap (an integer in [0, h]; the weights of one destination row sum
 * to H); columns alike with W, w, wx.  total = sum_s sum_t wy(i,s) * wx(j,t) * src[s][t];
 * dst = floor((2*total + H*W) / (2*H*W)): the area-weighted mean, rounded half up.  total reaches 255*H*W (> 2^32 for a
 * 4000 x 6000 frame): column sums are u32 (255*H < 2^32: H <= 16843009, checked), the horizontal sum and the division u64.
 * The result does not depend on the order
 * of summation.  (OpenCV evaluates the same weights in fp32 and rounds to nearest-even: expected within one grey level.) */
int udaseg_resize_area_u8(const uint8_t* src, int n, int H, int W, int h, int w, uint8_t* dst, void* stream);
/* Nearest resize for label masks: src [n][H][W] -> dst [n][h][w], dst[i][j] = src[(i*H)/h][(j*W)/w] in integer arithmetic, any
 * size ratio; values pass through unchanged (255 included).  cv2 INTER_NEAREST / torch mode="nearest". */
int udaseg_resize_nearest_u8(const uint8_t* src, int n, int H, int W, int h, int w, uint8_t* dst, void* stream);
/* Mask histogram: masks [n][pixels] -> hist[k][v] += the number of pixels of mask k equal to v (int64 [n][256] counters that
 * ACCUMULATE across calls; the caller zeroes them once, as for udaseg_score_hist).  pixels < 2^32. */
int udaseg_mask_hist_u8(const uint8_t* masks, int n, int64_t pixels, int64_t* hist, void* stream);
/* Antialiased bilinear resize fused with A.Normalize: src [n][H][W][3] -> out [n][h][w][cpad] (fp32, or bf16 when out_bf16,
 * rounded once from the fp32 value; padding lanes 0), any size ratio.  Each axis has a DEVICE table built by the caller:
 * destination index i reads the `taps` source indices start[i] .. start[i] + taps - 1 (those outside the source are skipped)
 * with the fp32 weights w[i][0..taps).  The tables of torch.nn.functional.interpolate(mode="bilinear", antialias=True,
 * align_corners=False) for L -> l: scale = L/l, support = max(scale, 1), c = scale*(i + 0.5), lo = max(0, int(c - support + 0.5)),
 * hi = min(L, int(c + support + 0.5)), weight_j = max(0, 1 - |(j - c + 0.5) / support|) for j in [lo, hi) divided by their sum,
 * in float64, rounded to fp32 (at equal size the weights are (1, 0); an enlargement is plain bilinear).
 * v = sum_s y_w[i][s] * sum_t x_w[j][t] * src, accumulated in fp32 on the 0..255 scale (rows first), then
 * out = (v - mean255[c]) * inv_std255[c] with HOST arrays of 3 floats: the arithmetic of udaseg_prepare_batch_u8.  Normalising
 * after resampling equals the reference's normalise-then-resize up to rounding, since the weights of a pixel sum to 1. */
int udaseg_resize_aa_u8(const uint8_t* src, int n, int H, int W, int h, int w, const int32_t* y_start, const float* y_w, int y_taps,
                        const int32_t* x_start, const float* x_w, int x_taps, const float* mean255, const float* inv_std255,
                        void* out, int cpad, int out_bf16, void* stream);

/* ---- scratch: one caller-owned device buffer PER DEVICE the library may use for split partial results (currently the
 *      small-channel weight gradient, <= 10 MiB); the call binds it to the device that is current when it is made.
 *      Without it those calls take the generic atomics path. ---- */
int udaseg_set_workspace(void* ptr, size_t bytes);
/* bytes of that buffer udaseg_conv2d_wgrad would use for this convolution (0 = none); the maximum over a network's layers is
 * what the caller should provide (the Python host hands over 16 MiB once per device). */
size_t udaseg_workspace_bytes(const udaseg_conv_desc* d);

/* ---- bf16 storage path (BASELINE configs 3 / 5): the HBM-bound kernels above on bf16 NHWC tensors (channels % 8 == 0),
 *      arithmetic and statistics in fp32 / f64; same meaning as their fp32 namesakes.  Parameters, their gradients and the
 *      optimizer state stay fp32 (master copies); udaseg_cast_f32_to_bf16 makes the per-step bf16 weight copy. ---- */
int udaseg_bn_apply_bf16(const void* y, const double* sums, const float* gamma, const float* beta, const void* residual,
                         void* z, int64_t pixels, int c, float eps, float momentum, float* running_mean, float* running_var,
                         float* save_mean, float* save_rstd, int act, float slope, void* stream);
int udaseg_bn_bwd_reduce_bf16(const void* dz, const void* z, const void* y, const float* save_mean, const float* save_rstd,
                              int64_t pixels, int c, double* bsums, int act, float slope, void* stream);
int udaseg_bn_bwd_apply_bf16(const void* dz, const void* z, const void* y, const float* save_mean, const float* save_rstd,
                             const float* gamma, const double* bsums, void* dy, void* dres, float* dgamma, float* dbeta,
                             int64_t pixels, int c, int act, float slope, int accumulate_dy, int accumulate_dres,
                             int accumulate_param, void* stream);
int udaseg_act_bwd_bf16(const void* dz, const void* z, void* dy, int64_t count, int act, float slope, void* stream);
int udaseg_channel_sum_bf16(const void* x, int64_t pixels, int c, float* out, int accumulate, void* stream);
int udaseg_channel_sum_bf16_ws(const void* x, int64_t pixels, int c, float* out, int accumulate, float* scratch,
                               size_t scratch_bytes, void* stream);
int udaseg_nchw_to_nhwc_bf16(const float* x, void* y, int n, int c, int h, int w, int cpad, void* stream);
int udaseg_cast_f32_to_bf16(const float* x, void* y, int64_t count, void* stream);
int udaseg_maxpool3x3s2_fwd_bf16(const void* x, void* y, uint8_t* idx, int n, int h, int w, int c, void* stream);
int udaseg_maxpool3x3s2_bwd_bf16(const void* dy, const uint8_t* idx, void* dx, int n, int h, int w, int c, int accumulate,
                                 void* stream);
int udaseg_upsample2x_concat_bwd_bf16(const void* dout, void* da, void* dskip, int n, int h, int w, int ca, int cb,
                                      int accumulate_da, int accumulate_dskip, void* stream);
int udaseg_gap_partial_bf16(const void* z, float* partial, int n, int hw, int c, void* stream);
int udaseg_gap_finish(const float* partial, const float* w, const float* b, float* pooled, float* p, int n, int hw, int c,
                      void* stream);
int udaseg_gap_bwd_broadcast_bf16(const float* dp, const float* p, const float* w, void* dz, int n, int hw, int c, void* stream);
int udaseg_gap_bwd_param(const float* dp, const float* p, const float* pooled, float* dw, float* db, int n, int c,
                         int accumulate_param, void* stream);
int udaseg_pack_dgrad_batched_bf16(const float* arena, void* packed, const int* table, int entries, void* stream);

/* ---- bf16-first convolution kernels (round 3; csrc/conv_halo_bf16.hip): stride-1 3x3 / pad 1 and 1x1 / pad 0 convolutions of
 *      smp.Unet.forward and their data gradients (reference src/models/train.py:341,343; src/models/adversarial_trainer.py:104,113)
 *      for BASELINE configs 3 and 5.  The block stages the input halo of a channel chunk once into LDS, the weights arrive
 *      pre-packed in MFMA-fragment order and never touch LDS.
 *
 *      Fragment packing of a convolution with N produced / K gathered channels and a ks x ks window:
 *        packed[nb][dx][k16][dy][lane][j]  (nb < ceil(N/32), k16 < ceil(K/16), lane < 64, j < 8; bf16; udaseg_frag_elems elements)
 *          = Wsrc[n = 32 nb + (lane & 31)][tap][k = 16 k16 + 8 (lane >> 5) + j]   (zero where n >= N or k >= K)
 *      forward: Wsrc = the bf16 OHWI weights (N = co, K = ci, tap = dy*ks + dx); data gradient: Wsrc = the bf16 dgrad packing
 *      [ci][taps][co] (N = ci, K = co) with the window flipped.  udaseg_pack_frag_batched_bf16 packs every convolution of a
 *      network in one launch: table[i] = {mode (0 forward from w16 / 1 data gradient from wt16), source element offset,
 *      destination element offset, N, K, ks} (int32 x 6, device memory). ---- */
int64_t udaseg_frag_elems(int n_out, int k_in, int ks);
/* STREAM CONTRACT of the two per-device scratch bindings (udaseg_set_workspace, udaseg_set_stats_scratch): they are keyed by
 * DEVICE, not by stream.  Launches that use them -- K-sliced / split partial results, and the statistics of launches with more
 * than 1024 blocks -- must all be issued on ONE compute stream per device (or be ordered by the caller): two such launches on
 * different streams of one device would add into the same scratch and the first fold would take the second's partials.  The
 * weight-gradient side stream of the Python host (engine.py) only issues launches that use neither.  Round 5: for the STATISTICS
 * scratch the contract is enforced -- the first stream that needs it after a bind owns it; a launch on any other stream of that
 * device does not get it and adds into the 16 replicas of `stats` directly (correct, slower).
 * Optional caller-owned f64 scratch (bound to the current device; the caller ZEROES it once, the library leaves it zeroed after
 * every use): launches of more than 1024 blocks put their per-channel statistics there (256 replicas) and a fold kernel adds
 * them into `stats` -- otherwise hundreds of same-address f64 atomics per accumulator bound the low-channel full-resolution
 * layers.  Needs 256 * 2 * co * 8 bytes for a layer with co output channels (256 KiB covers co <= 64); NULL unbinds. */
int udaseg_set_stats_scratch(void* ptr, size_t bytes);
int udaseg_pack_frag_batched_bf16(const void* w16, const void* wt16, void* packed, const int* table, int entries, void* stream);
/* ---- a BatchNorm + activation that is never written (single-consumer layers, bf16): the producer's statistics are finalised
 *      into per-channel scale = gamma * rstd and shift = beta - mean * scale (plus the saved mean / rstd and the running
 *      statistics, exactly as udaseg_bn_apply_bf16 would), and every consumer of the activation applies
 *      act(fma(y, scale, shift)) rounded to bf16 while it stages y: the forward convolution (udaseg_conv2d_fwd_frag_bf16
 *      in_scale / in_shift), its weight gradient (udaseg_conv2d_wgrad_bnin_bf16) and the layer's own BatchNorm backward
 *      (udaseg_bn_bwd_apply_recompute_bf16: the mask is re-evaluated with the same fused multiply-add; its two reductions come
 *      from the consumer's data gradient, udaseg_conv2d_dgrad_frag_bf16 prev_y).  nn.BatchNorm2d + nn.ReLU inside smp.Unet's
 *      blocks, reference src/models/train.py:341,343. ---- */
int udaseg_bn_finalize(const double* sums, const float* gamma, const float* beta, int64_t pixels, int c, float eps, float momentum,
                       float* running_mean, float* running_var, float* save_mean, float* save_rstd, float* scale, float* shift,
                       void* stream);
int udaseg_bn_bwd_apply_recompute_bf16(const void* dz, const void* y, const float* fwd_scale, const float* fwd_shift,
                                       const float* save_mean, const float* save_rstd, const float* gamma, const double* bsums,
                                       void* dy, float* dgamma, float* dbeta, int64_t pixels, int c, int act, float slope,
                                       void* stream);
/* Weight gradient of a stride-1 3x3 / pad 1 convolution, bf16 operands, fp32 dW ACCUMULATED onto (caller-zeroed arena): a block
 * owns a 64 x 64 (or 32 x 64, 32 x 32) channel block of all nine taps and walks pixel tiles, x halo and dy tile staged once per
 * tile; few long-lived blocks, one set of atomics per wave (round 4: csrc/conv_wgrad_halo2.hip, shared with the fp32 split form
 * below; channel counts multiples of 32, images >= 32 pixels wide or 16-pixel-wide with 64-multiples).  skip / up_ca: the two
 * sources of a fused decoder input in ONE launch.  loss.backward() at reference src/models/train.py:343. */
int udaseg_conv2d_wgrad_halo_bf16_ok(const udaseg_conv_desc* d, int up_ca);
int udaseg_conv2d_wgrad_halo_bf16(const udaseg_conv_desc* d, const void* x, const void* skip, int up_ca, const void* dy, float* dw,
                                  void* stream);
int udaseg_conv2d_wgrad_bnin_bf16(const udaseg_conv_desc* d, const void* x, const float* in_scale, const float* in_shift, int in_act,
                                  float in_slope, const void* dy, float* dw, int accumulate, void* stream);
/* 1 when the convolution (dgrad = 0: forward, gathers ci and produces co; dgrad = 1: its data gradient; up_ca > 0: forward on the
 * fused decoder input cat([nearest_x2(a), skip]) with up_ca channels from a) can take these kernels */
int udaseg_conv_frag_ok(const udaseg_conv_desc* d, int dgrad, int up_ca);
/* 1 when, in addition, they are expected to be FASTER than the shared implicit-GEMM source for this shape (measured heuristic:
 * csrc/conv_halo_bf16.hip halo_choice) -- what the Python side asks before it routes a layer */
int udaseg_conv_frag_preferred(const udaseg_conv_desc* d, int dgrad, int up_ca);
/* y = act(conv(X, w) + bias) (+ BatchNorm statistics of conv(X, w) + bias into stats, as udaseg_conv2d_fwd_bnstats).
 * X = x [n][h][w][ci], or with up_ca > 0 the virtual cat([nearest_x2(x [n][h/2][w/2][up_ca]), skip [n][h][w][ci - up_ca]]), or with
 * in_scale / in_shift (fp32 [ci]) the producer's BatchNorm + activation applied on the fly: X = in_act(x * in_scale + in_shift)
 * rounded to bf16 -- the normalised activation of a single-consumer layer never reaches HBM.  out_f32: y is fp32 (logits).
 * Round 4: (1) 1x1 / stride-1 launches that are small GEMMs (ci, co multiples of 64 and >= 128, at most 73728 pixels: r50's
 * bottleneck projections from 96^2 down, reference smp.Unet("resnet50"), src/test_system.py:90-95) run on conv1x1_gemm_bf16_kernel
 * (LDS-DMA ring, persistent blocks), same epilogue options; (2) the descriptor may be the discriminator's 4x4 / stride 2 / pad 1
 * convolution (reference src/models/discriminator.py:15-34): x is [n][hi][wi][ci] with ci a power of two, y [n][hi/2][wi/2][co],
 * wfrag the 2x2-window packing over the input's four parity phases (table row mode 2: udaseg_frag_elems(co, 4 * ci, 2) elements);
 * no skip / in_scale there.  The data gradient takes the same descriptor with wfrag_t = the four parity-class packings (modes
 * 3, 4, 5, 6 = input row / column parity (0,0), (0,1), (1,0), (1,1)), udaseg_frag_elems(ci, co, 2) elements each, one after the other. */
int udaseg_conv2d_fwd_frag_bf16(const udaseg_conv_desc* d, const void* x, const void* skip, int up_ca, const void* wfrag,
                                const float* bias, const float* in_scale, const float* in_shift, int in_act, float in_slope,
                                void* y, int out_f32, int act, float slope, double* stats, void* stream);
/* dx = conv_transpose(dy, w) from the data-gradient fragment packing.  split > 0: channels [0, split) of the gradient go to dx
 * [n][h][w][split], the rest to dx2 (the two sources of a fused decoder input).  prev_y != NULL: also the BatchNorm-backward
 * reductions of the layer behind (as udaseg_conv2d_dgrad_bnreduce_bf16).  accumulate: dx += (one rounding of the fp32 sum). */
int udaseg_conv2d_dgrad_frag_bf16(const udaseg_conv_desc* d, const void* dy, const void* wfrag_t, void* dx, void* dx2, int split,
                                  const void* prev_y, const float* save_mean, const float* save_rstd, const float* gamma,
                                  const float* beta, int bn_act, float bn_slope, double* bsums, int accumulate, void* stream);

/* ---- fp32 convolutions on the bf16 matrix pipe (csrc/conv_halo_f32x3.hip): fp32 NHWC tensors in and out, every operand split
 *      exactly into three bf16 terms (x = bf16(x) + bf16(x - x0) + bf16(x - x0 - x1)), the six products with i + j <= 2 on
 *      v_mfma_f32_32x32x16_bf16, fp32 accumulation -- one unit in the last place of each PRODUCT is left out, below the
 *      rounding of the fp32 accumulation itself.  Stride-1 3x3 / pad 1 layers of smp.Unet (reference src/models/train.py:341,
 *      343) in the fp32 configurations; replaces udaseg_conv2d_fwd_bnstats / _upcat / udaseg_conv2d_dgrad(_bnreduce / _split)
 *      there.  UDASEG_F32_SPLIT=0 keeps every layer on the fp32-MFMA kernels.
 *      Weights: three planes of the fragment packing above (plane stride udaseg_frag_elems(N, K, 3) bf16 elements), made by
 *      udaseg_pack_frag_batched_f32x3 from the fp32 OHWI arena (mode 0) / the fp32 dgrad packing [ci][taps][co] (mode 1);
 *      table rows as for udaseg_pack_frag_batched_bf16, dst offset = plane 0 of the entry's 3 * frag_elems block. ---- */
int udaseg_pack_frag_batched_f32x3(const float* w32, const float* wt32, void* packed, const int* table, int entries, void* stream);
/* can / should this (forward or data-gradient) launch take the split kernel?  preferred = the library's measured heuristic */
int udaseg_conv_f32x3_ok(const udaseg_conv_desc* d, int dgrad, int up_ca);
int udaseg_conv_f32x3_preferred(const udaseg_conv_desc* d, int dgrad, int up_ca);
/* tests / tuning: 1 = 8 x 32 pixels x 32 channels per block, 2 = x 64 channels, for every launch; 0 = the heuristic again */
int udaseg_f32x3_force_config(int cfg);
/* y = act(conv(x) + bias); up_ca > 0: x is the half-resolution tensor of a fused decoder input cat([nearest_x2(x), skip]);
 * stats != NULL: BatchNorm statistics of y ([R][2][co] f64, accumulated) */
int udaseg_conv2d_fwd_f32x3(const udaseg_conv_desc* d, const float* x, const float* skip, int up_ca, const void* wfrag3,
                            const float* bias, float* y, int act, float slope, double* stats, void* stream);
/* The same BatchNorm + activation that is never written, on fp32 tensors (round 4; the <= 32-channel full-resolution decoder layers,
 * where the stand-alone udaseg_bn_apply pass moves 268 MB per layer at 8 x 512^2): x is the producer's RAW convolution output, the
 * staging applies act(fma(x, in_scale[c], in_shift[c])) -- udaseg_bn_apply's own arithmetic, bit for bit -- before the split, zero
 * padding stays zero.  up != 0: x is the half-resolution tensor [n][hi/2][wi/2][ci] behind a nearest x2 up-sampling (a decoder
 * block without a skip input).  Forward: every geometry of udaseg_conv2d_fwd_f32x3 with a single source.  Weight gradient: the
 * small-channel direct kernel (<= 32 channels, fp32 pipe; also up) or the halo-resident split kernel (plain source); dW accumulated
 * or overwritten.  The producer's own BatchNorm backward needs nothing new: on fp32 it re-evaluates the activation's
 * argument from its conv output already (udaseg_bn_bwd_reduce / _apply with z = NULL).  nn.BatchNorm2d + nn.ReLU in front of a
 * 3x3 convolution inside smp.Unet's decoder blocks and head, reference src/models/train.py:341,343. */
int udaseg_conv2d_fwd_f32x3_bnin_ok(const udaseg_conv_desc* d, int up);
/* z_out != NULL (plain source, launches for which udaseg_conv2d_fwd_f32x3_bnin_writes says 1: the wave-specialised kernel): the
 * loader waves also WRITE the transformed activation ([n][hi][wi][ci], bit for bit udaseg_bn_apply's output) -- the convolution's
 * weight gradient then reads it like any activation; saved: bn_apply's launch and its read of x */
int udaseg_conv2d_fwd_f32x3_bnin_writes(const udaseg_conv_desc* d);
int udaseg_conv2d_fwd_f32x3_bnin(const udaseg_conv_desc* d, const float* x, int up, const float* in_scale, const float* in_shift,
                                 int in_act, float in_slope, float* z_out, const void* wfrag3, const float* bias, float* y, int act,
                                 float slope, double* stats, void* stream);
int udaseg_conv2d_wgrad_bnin_ok(const udaseg_conv_desc* d, int up);
int udaseg_conv2d_wgrad_bnin(const udaseg_conv_desc* d, const float* x, int up, const float* in_scale, const float* in_shift,
                             int in_act, float in_slope, const float* dy, float* dw, int accumulate, void* stream);
/* dx (+)= conv_transpose(dy, w); split / prev_y / accumulate as udaseg_conv2d_dgrad_frag_bf16, on fp32 tensors */
int udaseg_conv2d_dgrad_f32x3(const udaseg_conv_desc* d, const float* dy, const void* wfrag3_t, float* dx, float* dx2, int split,
                              const float* prev_y, const float* save_mean, const float* save_rstd, const float* gamma,
                              const float* beta, int bn_act, float bn_slope, double* bsums, int accumulate, void* stream);

/* dW[co][9][ci] += weight gradient of a stride-1 3x3 layer, fp32 x / dy with the same three-term split (round 4:
 * csrc/conv_wgrad_halo2.hip, conv_wgrad_h2_kernel -- conflict-free 32-channel LDS sub-planes, one x fragment shared by the three
 * taps of a kernel column, double-buffered 2-row tiles).  Channel
 * blocks: 64 x 64, 32 produced x 64 gathered, 32 x 32 (co % 32 == 0 and ci % 32 == 0); images at least 32 pixels wide, or 16-pixel-
 * wide ones with 64-multiples (8 x 16 tiles).  Reference: loss.backward(), src/models/train.py:343.
 * up_ca > 0: x is the half-resolution tensor of a fused decoder input, skip the other source (up_ca a multiple of the gathered
 * channel block).
 * Pair-packed forms (UDASEG_OPT_WGRAD_PAIR): ci == 16 with co in {8, 16, 24, 32} and an even width >= 16 (two pixels of a
 * 16-channel tensor fill the 32 rows of an MFMA operand), and the one geometry with up_ca == ci: 32 up-sampled -> 16 produced
 * channels without a skip half (skip == NULL). */
int udaseg_conv2d_wgrad_halo_f32x3_ok(const udaseg_conv_desc* d, int up_ca);
int udaseg_conv2d_wgrad_halo_f32x3(const udaseg_conv_desc* d, const float* x, const float* skip, int up_ca, const float* dy,
                                   float* dw, void* stream);

/* ---- the decoder's up-sampled input convolved as what it is (round 5, csrc/conv_up_f32x3.hip).  smp's DecoderBlock runs
 *      conv3x3(cat([nearest_x2(a), skip])) (reference: model created src/test_system.py:90-95, called src/models/train.py:341,
 *      differentiated :343; trace fixture tests/golden/unet_r50_trace.json: aten::upsample_nearest2d + aten::cat in front of every
 *      decoder conv1).  On the up-sampled channels the nine taps of an output pixel of parity phase (oy & 1, ox & 1) read FOUR
 *      distinct pixels of `a`: a 2 x 2 convolution of `a` per phase with weights pre-summed over the taps that coincide --
 *      4/9 of the multiplications, forward and data gradient, and the data gradient comes out at a's own resolution (no 2 x 2
 *      sum-pool pass).  fp32 tensors, the three-term split of udaseg_conv2d_fwd_f32x3; the pre-sums are fp32 additions in the
 *      packer.  The skip half of the concatenation is a plain 3x3 convolution of `skip` (udaseg_conv2d_fwd_f32x3 /
 *      udaseg_conv2d_dgrad_f32x3 on weight slices packed by modes 0 / 1 below), run FIRST; the up half accumulates on top.
 *      d: the whole convolution at the OUTPUT resolution (hi x wi = 2h x 2w, ci = up_ca + skip channels, co).
 *      udaseg_pack_up_batched_f32x3: table rows of 8 int32 {mode, src element offset, dst element offset (plane 0), N, K, ldk, 0, 0}
 *        mode 0: 3x3 forward packing of channels [offset, offset + K) of OHWI rows of ldk channels (w32), N = co;
 *        mode 1: 3x3 data-gradient packing from wt32 [N][9][K] (ldk = K; rows [up_ca, ci) of the dgrad packing);
 *        mode 2: phase packing for udaseg_conv2d_fwd_up_f32x3 from w32 OHWI [N = co][3][3][ldk], channels [0, K = up_ca);
 *        mode 3: phase packing for udaseg_conv2d_dgrad_up_f32x3 from wt32 [ci][9][K = co], rows [0, N = up_ca);
 *        plane stride udaseg_frag_elems(N, K, 3) (modes 0, 1) / udaseg_frag_elems(N, K, 4) (modes 2, 3) bf16 elements. ---- */
int udaseg_conv_up_f32x3_ok(const udaseg_conv_desc* d, int up_ca);
int udaseg_pack_up_batched_f32x3(const float* w32, const float* wt32, void* packed, const int* table, int entries, void* stream);
/* y[n][hi][wi][co] (+)= conv3x3(nearest_x2(a)) over a's up_ca channels (accumulate != 0: on top of the skip half's result);
 * stats != NULL: BatchNorm statistics of y AFTER the accumulation ([R][2][co] f64, accumulated) */
int udaseg_conv2d_fwd_up_f32x3(const udaseg_conv_desc* d, const float* a, int up_ca, const void* wfrag_up, float* y, int accumulate,
                               double* stats, void* stream);
/* da[n][hi/2][wi/2][up_ca] (+)= gradient of `a` through conv3x3(nearest_x2(a)) given dy[n][hi][wi][co] (co a multiple of 8).
 * prev_y != NULL (the conv output [n][hi/2][wi/2][up_ca] of the conv + BatchNorm + activation layer that produced a, when this
 * convolution is a's only consumer): also that layer's two BatchNorm-backward sums, as udaseg_conv2d_dgrad_f32x3 */
int udaseg_conv2d_dgrad_up_f32x3(const udaseg_conv_desc* d, const float* dy, int up_ca, const void* wfrag_up_t, float* da,
                                 const float* prev_y, const float* save_mean, const float* save_rstd, const float* gamma,
                                 const float* beta, int bn_act, float bn_slope, double* bsums, int accumulate, void* stream);
/* tests / tuning: one tile configuration (1..8, csrc/conv_up_f32x3.hip up_choice) for every launch; 0 = the heuristic again */
int udaseg_up_f32x3_force_config(int cfg);
/* The weight gradient in the same form (csrc/conv_wgrad_halo2.hip, conv_wgrad_up_kernel): the 16 phase-tap correlations
 * T_{py,px}[u][v] = sum_{q,r} dy[2q+py, 2r+px] (x) a[q+py-1+u, r+px-1+v] at a's resolution, each added into the 1, 2 or 4 taps of
 * dW[co][9][ci] it stands for -- 16 tap evaluations per pixel of `a` instead of 36.  dW rows are d->ci channels long, the launch
 * fills channels [0, up_ca) (accumulated onto, like every weight gradient here).  up_ca a multiple of 64, co of 32, a at least 16
 * pixels wide.  The skip half: udaseg_conv2d_wgrad_halo_slice_f32x3 = udaseg_conv2d_wgrad_halo_f32x3 on a channel slice
 * [c_off, c_off + d->ci) of rows of ldw channels (d: the slice as a convolution of its own).  loss.backward(), src/models/train.py:343. */
int udaseg_conv2d_wgrad_up_f32x3_ok(const udaseg_conv_desc* d, int up_ca);
int udaseg_conv2d_wgrad_up_f32x3(const udaseg_conv_desc* d, const float* a, int up_ca, const float* dy, float* dw, void* stream);
int udaseg_conv2d_wgrad_halo_slice_f32x3(const udaseg_conv_desc* d, const float* x, const float* dy, float* dw, int ldw, int c_off,
                                         void* stream);
/* tests / tuning: blocks per launch of the phase-form weight gradient (0 = the default, 128) */
int udaseg_wgrad_up_set_blocks(int blocks);

/* ---- sixteen produced channels on a sixteen-wide matrix tile (round 5, csrc/conv_n16_f32x3.hip): the full-resolution tail of
 *      smp.Unet's decoder (decoder_channels[-1] = 16: block 4 conv2 forward and data gradient, the head's data gradient; reference
 *      src/test_system.py:90-95, src/models/train.py:341,343).  v_mfma_f32_16x16x32_bf16 with K = two taps of a 16-channel chunk:
 *      0.28 of the matrix-pipe cycles of the 32-row tile these layers half-filled.  fp32 tensors, three-term split; stride-1 3x3,
 *      produced channels == 16, gathered channels a multiple of 8 up to 32.  Weight fragments: udaseg_pack_up_batched_f32x3 mode 4
 *      (forward, from the OHWI arena) / mode 5 (data gradient, from the dgrad packing), 3 planes of ceil(K / 16) * 5 * 512 bf16. ---- */
int udaseg_conv_n16_f32x3_ok(const udaseg_conv_desc* d, int dgrad);
int udaseg_conv2d_fwd_n16_f32x3(const udaseg_conv_desc* d, const float* x, const float* in_scale, const float* in_shift, int in_act,
                                float in_slope, const void* wfrag, float* y, double* stats, void* stream);
int udaseg_conv2d_dgrad_n16_f32x3(const udaseg_conv_desc* d, const float* dy, const void* wfrag_t, float* dx, const float* prev_y,
                                  const float* save_mean, const float* save_rstd, const float* gamma, const float* beta, int bn_act,
                                  float bn_slope, double* bsums, void* stream);

/* ---- the encoder's stem (round 5, csrc/conv_stem_f32x3.hip): 7x7 / stride 2 / pad 3, 4 (3 + padding) -> 64 channels, forward --
 *      torchvision ResNet.conv1 inside smp.Unet (reference src/test_system.py:90-95, src/models/train.py:341).  For one kernel row the
 *      7 taps x 4 channels of an output pixel are 28 contiguous floats of an input row: the kernel stages a band of input rows once
 *      and runs K as 7 rows x 32, no im2col gather.  fp32 tensors, three-term split.  Weights: udaseg_pack_up_batched_f32x3 mode 8
 *      (3 planes of 28 * 512 bf16).  Replaces udaseg_conv2d_fwd_bnstats (conv_igemm_kernel, generic gather) on that layer. ---- */
int udaseg_conv_stem_f32x3_ok(const udaseg_conv_desc* d);
int udaseg_conv2d_fwd_stem_f32x3(const udaseg_conv_desc* d, const float* x, const void* wfrag, float* y, double* stats, void* stream);
/* The stem's weight gradient with the apply half of its BatchNorm backward in the staging (csrc/conv_stem_wgrad.hip,
 * conv_small_ci_wgrad_kernel, v_mfma_f32_32x32x2_f32): autograd's aten::convolution_backward of ResNet.conv1 and the dy of bn1's
 * aten::native_batch_norm_backward, reached by loss.backward() (reference src/models/train.py:343).  The stem has no data gradient,
 * so dy = udaseg_bn_bwd_apply(dz, y) has one reader: here it is formed from dz and y while they are staged (the same fp32
 * arithmetic from the same sums; the mask re-evaluated from y, so ReLU / leaky layers WITHOUT a residual input only) and never
 * stored.  dW[64][7][7][4] (+)= over the 147 live (ky, kx, c) columns, the fourth-channel entries are not touched; dgamma / dbeta as
 * udaseg_bn_bwd_apply writes them (accumulate_param).  bsums: udaseg_bn_bwd_reduce's.  Replaces udaseg_bn_bwd_apply +
 * udaseg_conv2d_wgrad on that layer; UDASEG_OPT_STEM_WGRAD_BN = 0 makes the query answer no. */
int udaseg_conv_stem_wgrad_bn_ok(const udaseg_conv_desc* d);
int udaseg_conv2d_wgrad_stem_bn(const udaseg_conv_desc* d, const float* x, const float* dz, const float* y, const float* save_mean,
                                const float* save_rstd, const float* gamma, const float* beta, const double* bsums, int act,
                                float slope, float* dw, float* dgamma, float* dbeta, int accumulate, int accumulate_param,
                                void* stream);
/* tests / tuning: cap on the blocks of that launch (0 = the default, one per CU) */
int udaseg_stem_wgrad_set_blocks(int blocks);

/* ---- diagnosis: while a device buffer of 6 * blocks u64 is registered, every implicit-GEMM launch of at most `blocks` blocks
 *      writes per block {entry, first tile load, end of K loop, exit} (100 MHz wall-clock ticks), HW_ID and XCC_ID into it
 *      (tools/igemm_timeline.py).  NULL switches it off.  Not for timed runs. ---- */
int udaseg_debug_set_timeline(void* buffer, int blocks);

/* ---- small utilities ---- */
int udaseg_fill_f32(float* p, int64_t count, float value, void* stream);
int udaseg_axpy_f32(float* y, const float* x, int64_t count, float alpha, void* stream); /* y += alpha*x */
/* p[i] += value, int64: num_batches_tracked of every nn.BatchNorm2d of a network (views of one arena) in one launch; reference
 * src/models/train.py:341 (training-mode forward) */
int udaseg_add_i64(int64_t* p, int64_t count, int64_t value, void* stream);
int udaseg_scale_f32(const float* x, float* y, int64_t count, float alpha, void* stream); /* y = alpha*x: gradient reversal,
                                                                                         * src/models/uda.py:99-111 */

/* ---- prediction: src/models/predict.py -- predict_batch (:113-130, argmax of the logits), predict_mask (:70-111,
 *      (sigmoid(logits) > 0.5).float()), and predict_large: one frame of any size through the model as a grid of tiles,
 *      blended back with a window (no reference counterpart; the reference resizes the frame to the model size).
 *      Tile grid of a frame axis of length L, tile t, stride s: n = 1 if L <= t else ceil((L - t) / s) + 1 tiles with
 *      origins max(0, min(i*s, L - t)); tiles numbered raster, row-major (k = i*cols + j).  A call covers the tiles
 *      [first, first + tiles).  views: bitmask of the D4 codes (prepare_batch's convention) taken per tile, in ascending code
 *      order; odd codes (transposes) need th == tw.  Tile sides are multiples of 32; classes 1..32; ldc, ldp multiples of 4. */
/* image uint8 [h][w][3] -> out [tiles*V][th][tw][cpad] (fp32, or bf16 when out_bf16; padding lanes 0): crop, numpy "reflect"
 * padding outside the frame, D4 view, A.Normalize with the arithmetic of udaseg_prepare_batch_u8 (host mean255 / inv_std255). */
int udaseg_predict_gather_u8(const uint8_t* image, int h, int w, int th, int tw, int rows, int cols, int sy, int sx, int first,
                             int tiles, int views, const float* mean255, const float* inv_std255, void* out, int cpad,
                             int out_bf16, void* stream);
/* logits fp32 [tiles*V][th][tw][ldc] (that gather's order) -> for every frame pixel covered by the call's tiles, in tile
 * order: acc[p][0..classes) += win_y[ty] * win_x[tx] * sum over views of softmax(logits of the view's pixel that holds it),
 * wsum[p] += win_y[ty] * win_x[tx] * V.  acc [h*w][ldp], wsum [h*w]; no atomics, bit-identical for any split into calls. */
int udaseg_predict_blend(const float* logits, int ldc, int h, int w, int th, int tw, int rows, int cols, int sy, int sx, int first,
                         int tiles, int views, int classes, const float* win_y, const float* win_x, float* acc, int ldp,
                         float* wsum, void* stream);
/* labels[p] = argmax over classes of probs[p] (first maximum on ties).  With wsum (may be NULL): first probs[p] /= wsum[p]
 * in place and the padding lanes [classes, ldc) are set to 0. */
int udaseg_predict_finish(float* probs, const float* wsum, int64_t pixels, int classes, int ldc, int64_t* labels, void* stream);
/* logits fp32 padded NHWC [n][hw][ldc] -> out fp32 NCHW [n][classes][hw] = (sigmoid(logit) > 0.5) ? 1 : 0 */
int udaseg_predict_threshold(const float* logits, int n, int hw, int classes, int ldc, float* out, void* stream);

/* ---- live kernel timing for bench.py's roofline leg: HIP events bracket every launch of the conv
 *      kernel families on the launch stream while enabled. ---- */
int udaseg_prof_enable(int on);
int udaseg_prof_reset(void);
/* family: 0 = igemm fwd/dgrad, 1 = wgrad.  Synchronises the recorded events (call outside timed regions). */
int udaseg_prof_read(int family, double* total_ms, double* total_flops, int64_t* launches);
/* Per KERNEL SYMBOL (one id per template instantiation; names match rocprofv3's kernel trace): total HIP-event time,
 * algorithmic GEMM FLOPs (2*M*N*K of every launch) and launch count while profiling was enabled. */
int udaseg_prof_kernel_count(void);
const char* udaseg_prof_kernel_name(int kid);
int udaseg_prof_kernel_read(int kid, double* total_ms, double* total_flops, int64_t* launches);
/* Per-launch records: ms, flops, kind (0 fwd, 1 dgrad, 2 wgrad) and the 11 ints of the conv desc. Returns the count. */
int udaseg_prof_records(int family, int max_records, double* ms, double* flops, int* kind, int* desc11);

#ifdef __cplusplus
}
#endif
#endif /* UDASEG_H */
