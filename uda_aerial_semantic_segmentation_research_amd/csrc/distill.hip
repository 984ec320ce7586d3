// Distillation: a loss between student logits and a teacher DISTRIBUTION, with per-pixel and per-image weights (Hinton et al.
// 2015; symmetric cross entropy, Wang et al., ICCV 2019, the loss ProDA's later stages train with; the per-image weight is
// DACS's / DAFormer's share of confident pixels).  fp32, HBM-bound, the family of losses.hip / losses_seg.hip / advent.hip:
// one thread per pixel row, both rows in registers, loss and gradient in ONE pass over the logits (ce_fwd_bwd_kernel's LDS tile:
// whole contiguous lines out, column sums on the way), loss_reduce.h's fixed-order f64 block partials and finish kernels, integer
// atomics for the counters only.
//
//   student z: [pixels][ldc], teacher t: [pixels][ldt]; only lanes < classes are read.   lp = log_softmax(z), p = exp(lp)
//   probs == 0:  q = softmax(t * teacher_inv_temp), lq = log_softmax(t * teacher_inv_temp)        probs == 1:  q = t, lq = logf(q)
//   Q = sum_c q_c
//   kind 0 (soft CE):   l = -sum_c q_c lp_c                          a lane with q_c == 0 contributes exactly 0
//   kind 1 (KL(q||p)):  l =  sum_c q_c (lq_c - lp_c)                 the same
//        dl/dz_k = Q p_k - q_k                                        (both)
//   kind 2 (symmetric): l = alpha (-sum_c q_c lp_c) + beta sum_c p_c g_c,  g_c = -max(lq_c, log_floor), -log_floor where q_c == 0;
//        dl/dz_k = alpha (Q p_k - q_k) + beta p_k (g_k - sum_c p_c g_c)     a lane with p_c == 0 contributes exactly 0 to the reverse term
//   w_p = weight_px[p] * weight_img[p / pix_per_image] (NULL: 1), the fp32 product.
//   VOID pixels (loss exactly 0, gradient exactly 0 in all ldc lanes):  w_p == 0 (counted in stats[1]);  w_p < 0 or not finite, a
//   teacher lane that is not finite (after the temperature), with probs a q_c outside [0, 1] or Q == 0 (all counted in stats[2]).
//   loss = sum_p w_p l_p / D,  D = pixels (mean), *denom (udaseg_pixel_weight_sum) or 1;  dlogits is d loss / d z for an upstream
//   gradient of 1, i.e. already carries w_p / D.
#include <float.h>

#include "loss_reduce.h"

namespace udaseg {

// lp[c] = log softmax(s x)[c], pr[c] = exp(lp[c]) for c < classes (0 in the pad lanes, whatever they hold): advent.hip's
// row_softmax over a row that is already in registers (the subtraction form and the contraction rule are explained there).
template <int LDC4>
__device__ __forceinline__ void row_log_softmax(const f32x4 (&v)[LDC4], int classes, float s, float* lp, float* pr) {
#pragma clang fp contract(off)
  float mx = -INFINITY;
#pragma unroll
  for (int k = 0; k < LDC4; ++k)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      lp[k * 4 + e] = v[k][e] * s;
      if (k * 4 + e < classes) mx = fmaxf(mx, lp[k * 4 + e]);
    }
  float sum = 0.f;
#pragma unroll
  for (int c = 0; c < LDC4 * 4; ++c) {
    lp[c] = c < classes ? lp[c] - mx : 0.f;
    if (c < classes) sum += expf(lp[c]);
  }
  const float lg = logf(sum);
#pragma unroll
  for (int c = 0; c < LDC4 * 4; ++c) {
    lp[c] = c < classes ? lp[c] - lg : 0.f;
    pr[c] = c < classes ? expf(lp[c]) : 0.f;
  }
}

// w_p and whether it voids the pixel: 0 = counts, 1 = void by a zero weight, 2 = void by a negative or non-finite weight.
// udaseg_pixel_weight_sum and the loss kernel share it, so the denominator and the loss cannot disagree about a pixel.
__device__ __forceinline__ int pixel_weight(const float* __restrict__ wpx, const float* __restrict__ wimg, int64_t p, int64_t ppi,
                                            bool small, float& w) {
  w = wpx ? wpx[p] : 1.f;
  if (wimg) {
    const int64_t i = small ? (int64_t)((uint32_t)p / (uint32_t)ppi) : p / ppi;
    w = w * wimg[i];
  }
  if (w == 0.f) return 1;
  return (w > 0.f && __builtin_isfinite(w)) ? 0 : 2;
}

constexpr int DS_STATS = 3;   // counted, void by weight 0, void otherwise

template <int LDC4, bool SYM>
__global__ __launch_bounds__(256) void soft_ce_kernel(const f32x4* __restrict__ logits, const float* __restrict__ teacher,
                                                      const float* __restrict__ wpx, const float* __restrict__ wimg, int64_t pixels,
                                                      int64_t ppi, int classes, int ldt, int probs, int kl, float inv_temp,
                                                      float alpha, float beta, float log_floor, int mean,
                                                      const double* __restrict__ denom, double* __restrict__ partials,
                                                      f32x4* __restrict__ dlogits, float* __restrict__ colpart,
                                                      unsigned long long* __restrict__ stats) {
#pragma clang fp contract(off)
  // The LDS tile is GradTile's (loss_reduce.h), written out: this kernel takes the barriers only when `grad` and stores only when
  // `dlogits`, and it sits at a cliff of the register allocator -- through the helper <6, true> took 176 VGPRs for 145 and the
  // symmetric loss of 8 x 512 x 512 pixels 0.257 ms for 0.233 (profiles/loss_reduce_refactor.txt).  Same map, same order.
  constexpr int LDC = LDC4 * 4;
  constexpr int NG = 256 / LDC;
  __shared__ __attribute__((aligned(16))) float tile[256 * LDC];
  __shared__ float colred[NG * LDC];
  __shared__ double red[4];
  const int tid = threadIdx.x;
  const bool grad = dlogits != nullptr || colpart != nullptr;   // uniform: the barriers below are taken by all or by none
  const bool small = pixels <= (int64_t)UINT32_MAX;
  const float scale = mean ? 1.f / (float)pixels : (denom ? (float)(1.0 / *denom) : 1.f);
  const int nvt = (classes + 3) >> 2;
  const int64_t nchunks = (pixels + 255) / 256;
  const int cc = tid % LDC, rg = tid / LDC;
  float colacc = 0.f;
  double local = 0.0;
  unsigned int cnt[DS_STATS] = {0u, 0u, 0u};
  for (int64_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
    const int64_t p = chunk * 256 + tid;
    bool ok = p < pixels;
    float w = 0.f;
    float lq[LDC], q[LDC];
    float Q = 0.f;
    if (ok) {
      int why = pixel_weight(wpx, wimg, p, ppi, small, w);
      if (why == 0) {
        // the teacher row: the vectors past its end (ldt < ldc) are read from vector 0 instead, every such lane is >= classes
        const f32x4* trow = reinterpret_cast<const f32x4*>(teacher + p * ldt);
        f32x4 tv[LDC4];
#pragma unroll
        for (int k = 0; k < LDC4; ++k) tv[k] = trow[k < nvt ? k : 0];
        bool bad = false;
#pragma unroll
        for (int k = 0; k < LDC4; ++k)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float x = probs ? tv[k][e] : tv[k][e] * inv_temp;
            if (k * 4 + e < classes) bad |= !__builtin_isfinite(x) || (probs && !(x >= 0.f && x <= 1.f));
          }
        if (!bad) {
          if (probs) {
#pragma unroll
            for (int k = 0; k < LDC4; ++k)
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                const int c = k * 4 + e;
                q[c] = c < classes ? tv[k][e] : 0.f;
                lq[c] = (kl || SYM) && q[c] > 0.f ? logf(q[c]) : 0.f;
              }
          } else {
            row_log_softmax<LDC4>(tv, classes, inv_temp, lq, q);
          }
#pragma unroll
          for (int c = 0; c < LDC; ++c) Q += q[c];
          bad = probs && Q == 0.f;
        }
        if (bad) why = 2;
      }
#pragma unroll
      for (int k = 0; k < DS_STATS; ++k) cnt[k] += why == k;
      ok = why == 0;
    }
    if (ok) {
      f32x4 v[LDC4];
      load_row<LDC4>(logits + p * LDC4, v);
      float lp[LDC], pr[LDC];
      row_log_softmax<LDC4>(v, classes, 1.f, lp, pr);
      float fwd = 0.f;                                   // -sum q lp, or sum q (lq - lp)
#pragma unroll
      for (int c = 0; c < LDC; ++c) {
        const float term = (!SYM && kl) ? q[c] * (lq[c] - lp[c]) : -(q[c] * lp[c]);
        fwd += q[c] > 0.f ? term : 0.f;
      }
      float l = fwd, R = 0.f;
      if (SYM) {
#pragma unroll
        for (int c = 0; c < LDC; ++c) {
          lq[c] = q[c] > 0.f ? -fmaxf(lq[c], log_floor) : -log_floor;      // g_c from here on
          R += pr[c] > 0.f ? pr[c] * lq[c] : 0.f;
        }
        l = alpha * fwd + beta * R;
      }
      local += (double)(w * l);
      if (grad) {
        const float cw = scale * w;
#pragma unroll
        for (int k = 0; k < LDC4; ++k) {
          f32x4 g;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int c = k * 4 + e;
            float d = Q * pr[c] - q[c];
            if (SYM) d = alpha * d + (pr[c] > 0.f ? beta * (pr[c] * (lq[c] - R)) : 0.f);
            g[e] = c < classes ? cw * d : 0.f;
          }
          *reinterpret_cast<f32x4*>(tile + tid * LDC + k * 4) = g;
        }
      }
    } else if (grad) {
#pragma unroll
      for (int k = 0; k < LDC4; ++k) *reinterpret_cast<f32x4*>(tile + tid * LDC + k * 4) = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    if (grad) {
      __syncthreads();
      if (dlogits) {
        const int64_t base4 = chunk * 256 * LDC4, lim4 = pixels * LDC4;
#pragma unroll
        for (int it = 0; it < LDC4; ++it) {
          const int idx = it * 256 + tid;
          if (base4 + idx < lim4) dlogits[base4 + idx] = reinterpret_cast<const f32x4*>(tile)[idx];
        }
      }
      if (colpart && rg < NG) {
        for (int r = rg; r < 256; r += NG) colacc += tile[r * LDC + cc];
      }
      __syncthreads();
    }
  }
  if (colpart && rg < NG) colred[rg * LDC + cc] = colacc;
  block_partial(local, red, partials);   // its barrier is the column sums' too
  if (stats) {
#pragma unroll
    for (int k = 0; k < DS_STATS; ++k) {
      const unsigned int n = wave_sum_u32(cnt[k]);       // per wave, not BlockCounts: the kernel sits at a register cliff
      if ((tid & 63) == 0 && n) atomicAdd(&stats[k], (unsigned long long)n);   // (profiles/loss_reduce_refactor.txt)
    }
  }
  if (colpart && tid < LDC) {
    float s = 0.f;
    for (int g2 = 0; g2 < NG; ++g2) s += colred[g2 * LDC + tid];
    colpart[(size_t)blockIdx.x * LDC + tid] = s;
  }
}

// partials[k][block], k = 0: sum of w_p over the pixels whose weight counts (f64), 1: zero weights, 2: negative / non-finite
// weights (whole numbers < 2^53: exact in f64).  Fixed pixel-to-thread map, fixed-order reductions: ce_target_stats_kernel's shape.
__global__ __launch_bounds__(256) void pixel_weight_sum_kernel(const float* __restrict__ wpx, const float* __restrict__ wimg,
                                                               int64_t pixels, int64_t ppi, double* __restrict__ partials) {
  __shared__ double red[3][4];
  const bool small = pixels <= (int64_t)UINT32_MAX;
  const int64_t T = (int64_t)gridDim.x * 256;
  double d = 0.0;
  unsigned int nz = 0, nbad = 0;
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < pixels; p += T) {
    float w;
    const int why = pixel_weight(wpx, wimg, p, ppi, small, w);
    if (why == 0) d += (double)w;
    nz += why == 1;
    nbad += why == 2;
  }
  double v[3] = {d, (double)nz, (double)nbad};
  block_partial_rows<3>(v, red, partials);
}

// above[i] += pixels of image i (blockIdx.y) whose winner confidence (pixel_conf: udaseg_conf_hist's) is >= tau, nonfinite[i] +=
// its non-finite pixels.  One 64-bit integer atomic per non-zero counter per block: exact, the same on every run.
constexpr int CS_BLOCKS_X = 256;

template <int NV>
__global__ __launch_bounds__(256) void conf_share_kernel(const float* __restrict__ scores, int64_t ppi, int classes, int ldc, int probs,
                                                         float tau, unsigned long long* __restrict__ above,
                                                         unsigned long long* __restrict__ nonfinite) {
  __shared__ BlockCounts<2>::Slots red;                    // 256 threads: four waves
  const float* img = scores + (int64_t)blockIdx.y * ppi * ldc;
  unsigned int ev[2] = {0, 0};                             // above tau, non-finite
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < ppi; p += (int64_t)gridDim.x * 256) {
    const PixelConf r = pixel_conf<NV>(img + p * ldc, classes, probs);
    ev[0] += r.finite && r.p >= tau;
    ev[1] += !r.finite;
  }
  BlockCounts<2>::put(red, ev);
  __syncthreads();
  if (threadIdx.x < 2) {                                   // two arrays, so total and not flush
    const unsigned int n = BlockCounts<2>::total(red, threadIdx.x);
    if (n) atomicAdd((threadIdx.x ? nonfinite : above) + blockIdx.y, (unsigned long long)n);
  }
}

__global__ void conf_share_finish_kernel(const unsigned long long* __restrict__ above, int batch, double ppi, float* __restrict__ share) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < batch) share[i] = (float)((double)above[i] / ppi);
}

}  // namespace udaseg

using namespace udaseg;

extern "C" int udaseg_soft_ce_fwd_bwd(const float* logits, const float* teacher, const float* weight_px, const float* weight_img,
                                      int batch, int64_t pix_per_image, int classes, int ldc, int ldt, int probs, int kind,
                                      float teacher_inv_temp, float alpha, float beta, float log_floor, int mean, const double* denom,
                                      double* partials, float* loss, float* dlogits, float* colsum_partials, float* colsum,
                                      int64_t* stats, void* stream) {
  if (!image_grid_ok("soft_ce_fwd_bwd", batch, pix_per_image)) return UDASEG_E_BADARG;
  const int64_t pixels = (int64_t)batch * pix_per_image;
  if (!scores_args_ok("soft_ce_fwd_bwd", pixels, classes, ldc, 32) ||
      !scores_args_ok("soft_ce_fwd_bwd", pixels, classes, ldt, 32, "ldt"))
    return UDASEG_E_BADARG;
  UDASEG_CHECK_ARG(classes >= 2, "soft_ce_fwd_bwd: need classes >= 2 (classes=%d)", classes);
  UDASEG_CHECK_ARG(logits && teacher && partials && loss, "soft_ce_fwd_bwd: NULL pointer");
  UDASEG_CHECK_ARG(((reinterpret_cast<uintptr_t>(logits) | reinterpret_cast<uintptr_t>(teacher) | reinterpret_cast<uintptr_t>(dlogits)) & 15) == 0,
                   "soft_ce_fwd_bwd: logits, teacher and dlogits must be 16-byte aligned");
  UDASEG_CHECK_ARG(probs == 0 || probs == 1, "soft_ce_fwd_bwd: probs must be 0 (logits) or 1 (probabilities), got %d", probs);
  UDASEG_CHECK_ARG(kind >= 0 && kind <= 2, "soft_ce_fwd_bwd: kind must be 0 (soft CE), 1 (KL) or 2 (symmetric CE), got %d", kind);
  UDASEG_CHECK_ARG(probs || (teacher_inv_temp > 0.f && teacher_inv_temp <= FLT_MAX),
                   "soft_ce_fwd_bwd: teacher_inv_temp must be positive and finite, got %g", (double)teacher_inv_temp);
  UDASEG_CHECK_ARG(kind != 2 || (log_floor < 0.f && log_floor >= -FLT_MAX && alpha >= -FLT_MAX && alpha <= FLT_MAX &&
                                 beta >= -FLT_MAX && beta <= FLT_MAX),
                   "soft_ce_fwd_bwd: symmetric CE needs finite alpha, beta and a finite log_floor < 0 (alpha=%g beta=%g log_floor=%g)",
                   (double)alpha, (double)beta, (double)log_floor);
  UDASEG_CHECK_ARG(!(mean && denom), "soft_ce_fwd_bwd: mean (divide by pixels) and denom (divide by *denom) exclude each other");
  UDASEG_CHECK_ARG((colsum == nullptr) == (colsum_partials == nullptr), "soft_ce_fwd_bwd: colsum and colsum_partials come together");
  hipStream_t st = as_stream(stream);
  const int grid = capped_grid(pixels, 256, udaseg_seg_partials());
  if (!dispatch_width<8>(ldc / 4, [&](auto w) {
        constexpr int W = decltype(w)::value;
        hipLaunchKernelGGL((kind == 2 ? soft_ce_kernel<W, true> : soft_ce_kernel<W, false>), dim3(grid), dim3(256), 0, st,
                           (const f32x4*)logits, teacher, weight_px, weight_img, pixels, pix_per_image, classes, ldt, probs,
                           kind == 1 ? 1 : 0, teacher_inv_temp, alpha, beta, log_floor, mean, denom, partials, (f32x4*)dlogits,
                           colsum_partials, (unsigned long long*)stats);
      }))
    return unsupported_width("soft_ce_fwd_bwd", "ldc", ldc);
  UDASEG_LAUNCH_CHECK("soft_ce launch");
  // mean and denom exclude each other (above): D = pixels, *denom or 1
  const int rc = launch_loss_finish(partials, grid, mean ? (double)pixels : 1.0, denom, loss, 0, st, "soft_ce_finish launch");
  return rc || !colsum ? rc : launch_colsum_finish(colsum_partials, grid, ldc, colsum, 0, st, "soft_colsum_finish launch");
}

extern "C" int udaseg_pixel_weight_sum(const float* weight_px, const float* weight_img, int batch, int64_t pix_per_image,
                                       double* partials, double* denom, int64_t* counts, void* stream) {
  if (!image_grid_ok("pixel_weight_sum", batch, pix_per_image)) return UDASEG_E_BADARG;
  UDASEG_CHECK_ARG(partials && denom && counts, "pixel_weight_sum: NULL pointer");
  const int64_t pixels = (int64_t)batch * pix_per_image;
  hipStream_t st = as_stream(stream);
  const int grid = capped_grid(pixels, 256, udaseg_seg_partials());
  hipLaunchKernelGGL(pixel_weight_sum_kernel, dim3(grid), dim3(256), 0, st, weight_px, weight_img, pixels, pix_per_image, partials);
  UDASEG_LAUNCH_CHECK("pixel_weight_sum launch");
  return launch_rows_finish(3, partials, grid, denom, counts, st, "pixel_weight_sum_finish launch");
}

extern "C" int udaseg_conf_share(const float* scores, int batch, int64_t pix_per_image, int classes, int ldc, int probs, float tau,
                                 int64_t* above, int64_t* nonfinite, float* share, void* stream) {
  if (!image_grid_ok("conf_share", batch, pix_per_image)) return UDASEG_E_BADARG;
  if (!scores_args_ok("conf_share", (int64_t)batch * pix_per_image, classes, ldc)) return UDASEG_E_BADARG;
  UDASEG_CHECK_ARG(scores && above && nonfinite && share, "conf_share: NULL pointer");
  UDASEG_CHECK_ARG((reinterpret_cast<uintptr_t>(scores) & 15) == 0, "conf_share: scores must be 16-byte aligned");
  UDASEG_CHECK_ARG(probs == 0 || probs == 1, "conf_share: probs must be 0 (logits) or 1 (probabilities), got %d", probs);
  UDASEG_CHECK_ARG(batch <= 65535, "conf_share: at most 65535 images per call (batch=%d)", batch);
  UDASEG_CHECK_ARG(tau == tau, "conf_share: tau is NaN");
  hipStream_t st = as_stream(stream);
  hipError_t e = hipMemsetAsync(above, 0, sizeof(int64_t) * batch, st);
  if (e == hipSuccess) e = hipMemsetAsync(nonfinite, 0, sizeof(int64_t) * batch, st);
  if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync(conf_share)");
  const int gx = capped_grid(pix_per_image, 256, CS_BLOCKS_X);
  if (!dispatch_width<8>(cdiv(classes, 4), [&](auto w) {
        hipLaunchKernelGGL(conf_share_kernel<decltype(w)::value>, dim3(gx, batch), dim3(256), 0, st, scores, pix_per_image, classes, ldc,
                           probs, tau, (unsigned long long*)above, (unsigned long long*)nonfinite);
      }))
    return unsupported_width("conf_share", "classes", classes);
  UDASEG_LAUNCH_CHECK("conf_share launch");
  hipLaunchKernelGGL(conf_share_finish_kernel, dim3(cdiv(batch, 256)), dim3(256), 0, st, (const unsigned long long*)above, batch,
                     (double)pix_per_image, share);
  UDASEG_LAUNCH_CHECK("conf_share_finish launch");
  return UDASEG_OK;
}
