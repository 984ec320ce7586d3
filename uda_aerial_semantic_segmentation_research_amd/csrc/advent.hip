// Output-space adaptation (AdvEnt, Vu et al., CVPR 2019; maximum squares, Chen et al., ICCV 2019), fp32, HBM-bound:
//   weighted self-information maps  I_c = -p_c log p_c / log C  of a prediction, forward and backward (the discriminator's input)
//   entropy / maximum-squares loss of a prediction with its gradient in the same pass (the direct part)
// Logits are NHWC rows [pixel][ldc] with `classes` valid channels (ldc % 4 == 0, ldc <= 32), as produced by Unet; the maps are
// rows [pixel][cpad] of fp32 or bf16 that a convolution reads in place, so their pad lanes are written as zeros.
// One thread per pixel, softmax row in registers, wave/block reductions, f64 cross-block partials and a finish kernel: the
// pattern of losses_seg.hip, with loss_reduce.h's block partial and finish.
#include "loss_reduce.h"

namespace udaseg {

typedef __bf16 bf16x8a __attribute__((ext_vector_type(8)));

// lp[c] = log softmax(z)[c], pr[c] = exp(lp[c]) for c < classes (0 in the pad lanes, whatever they hold).
// Max-shifted log-sum-exp, but lp = (x - mx) - log(sum) rather than x - (mx + log(sum)): the sum mx + log(sum) is never rounded.
// Its rounding is half an ulp of |lse| (2.4e-7 at lse = 6.5) added to EVERY log probability of the row, i.e. that much relative
// error on every probability, the largest included: one ulp of lse moved sum p^2 of a 32-class row by 9e-7 of its value, where the
// form below leaves the winner's lp = -log(sum) with the error of logf alone (tests/test_gpu_advent_grade.py, the single-row cases).
// No contraction, for losses_seg.hip's reason: the subtraction of mx must see the values the max was taken over.
template <int LDC4>
__device__ __forceinline__ void row_softmax(const f32x4* __restrict__ logits, int64_t p, int classes, float* lp, float* pr) {
#pragma clang fp contract(off)
  f32x4 v[LDC4];
  load_row<LDC4>(logits + p * LDC4, v);
  float mx = -INFINITY;
#pragma unroll
  for (int k = 0; k < LDC4; ++k)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      lp[k * 4 + e] = v[k][e];
      if (k * 4 + e < classes) mx = fmaxf(mx, v[k][e]);
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

// info[c] = I_c = -s p_c lp_c where p_c > 0, else exactly 0 (an underflowed probability, a -inf logit: never 0 * inf); returns
// H = sum_c I_c.  The pad lanes hold p = 0, so they give 0.
template <int LDC>
__device__ __forceinline__ float self_info(const float* lp, const float* pr, float s, float* info) {
  float h = 0.f;
#pragma unroll
  for (int c = 0; c < LDC; ++c) {
    info[c] = pr[c] > 0.f ? -(s * (pr[c] * lp[c])) : 0.f;
    h += info[c];
  }
  return h;
}

// maps[p][c] = I_c (c < classes), 0 (classes <= c < cpad); entropy[p] = H (optional)
template <int LDC4, bool BF16>
__global__ __launch_bounds__(256) void selfinfo_fwd_kernel(const f32x4* __restrict__ logits, int64_t pixels, int classes, float s,
                                                           void* __restrict__ maps, int cpad, float* __restrict__ entropy) {
  constexpr int LDC = LDC4 * 4;
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < pixels; p += (int64_t)gridDim.x * 256) {
    float lp[LDC], pr[LDC], info[LDC];
    row_softmax<LDC4>(logits, p, classes, lp, pr);
    const float h = self_info<LDC>(lp, pr, s, info);
    if (entropy) entropy[p] = h;
    if (BF16) {
      f32x4* dst = reinterpret_cast<f32x4*>(static_cast<__bf16*>(maps) + p * cpad);
      const int nq = cpad >> 3;
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (q < nq) {
          bf16x8a o;
#pragma unroll
          for (int e = 0; e < 8; ++e) o[e] = (__bf16)(q * 8 + e < LDC ? info[q * 8 + e < LDC ? q * 8 + e : 0] : 0.f);
          dst[q] = __builtin_bit_cast(f32x4, o);
        }
    } else {
      f32x4* dst = reinterpret_cast<f32x4*>(static_cast<float*>(maps) + p * cpad);
      const int nq = cpad >> 2;
#pragma unroll
      for (int q = 0; q < 8; ++q)
        if (q < nq) {
          f32x4 o;
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] = q * 4 + e < LDC ? info[q * 4 + e < LDC ? q * 4 + e : 0] : 0.f;
          dst[q] = o;
        }
    }
  }
}

// dlogits_k = p_k (g_k - sum_c p_c g_c),  g_c = -s (lp_c + 1) dmaps_c;  a lane with p = 0 has g = 0 and a gradient of exactly 0
template <int LDC4, bool BF16>
__global__ __launch_bounds__(256) void selfinfo_bwd_kernel(const f32x4* __restrict__ logits, const void* __restrict__ dmaps,
                                                           int64_t pixels, int classes, float s, int cpad,
                                                           f32x4* __restrict__ dlogits) {
  constexpr int LDC = LDC4 * 4;
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < pixels; p += (int64_t)gridDim.x * 256) {
    float lp[LDC], pr[LDC], g[LDC];
    row_softmax<LDC4>(logits, p, classes, lp, pr);
    // the vectors past the row's end (cpad < ldc) are read from vector 0 instead: every lane >= cpad is >= classes and ignored
    // below, and a selected address keeps the loads unconditional (predicated loads cost the fp32 form 196 VGPRs at 24 lanes, 79 so)
    if (BF16) {
      const f32x4* src = reinterpret_cast<const f32x4*>(static_cast<const __bf16*>(dmaps) + p * cpad);
      const int nq = cpad >> 3;
#pragma unroll
      for (int q = 0; q < (LDC + 7) / 8; ++q) {
        const bf16x8a v = __builtin_bit_cast(bf16x8a, src[q < nq ? q : 0]);
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (q * 8 + e < LDC) g[q * 8 + e < LDC ? q * 8 + e : 0] = (float)v[e];
      }
    } else {
      const f32x4* src = reinterpret_cast<const f32x4*>(static_cast<const float*>(dmaps) + p * cpad);
      const int nq = cpad >> 2;
#pragma unroll
      for (int q = 0; q < LDC4; ++q) {
        const f32x4 v = src[q < nq ? q : 0];
#pragma unroll
        for (int e = 0; e < 4; ++e) g[q * 4 + e] = v[e];
      }
    }
    float S = 0.f;
#pragma unroll
    for (int c = 0; c < LDC; ++c) {
      g[c] = (c < classes && pr[c] > 0.f) ? -(s * (lp[c] + 1.f)) * g[c] : 0.f;
      S += pr[c] * g[c];
    }
#pragma unroll
    for (int k = 0; k < LDC4; ++k) {
      f32x4 d;
#pragma unroll
      for (int e = 0; e < 4; ++e) d[e] = pr[k * 4 + e] > 0.f ? pr[k * 4 + e] * (g[k * 4 + e] - S) : 0.f;
      dlogits[p * LDC4 + k] = d;
    }
  }
}

// KIND 0 (entropy): term = H;                 dlogits_k = coef p_k (lp_k + H_nat), H_nat = -sum p lp, coef = -(s / pixels)
// KIND 1 (maximum squares): term = sum p_c^2;  dlogits_k = coef p_k (p_k - sum p_c^2),             coef = -(1 / pixels)
// partials[block] = sum of the block's terms (f64); dlogits and entropy optional
template <int LDC4, int KIND>
__global__ __launch_bounds__(256) void entropy_loss_kernel(const f32x4* __restrict__ logits, int64_t pixels, int classes, float s,
                                                           float coef, double* __restrict__ partials, f32x4* __restrict__ dlogits,
                                                           float* __restrict__ entropy) {
  constexpr int LDC = LDC4 * 4;
  __shared__ double red[4];
  double local = 0.0;
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < pixels; p += (int64_t)gridDim.x * 256) {
    float lp[LDC], pr[LDC], info[LDC];
    row_softmax<LDC4>(logits, p, classes, lp, pr);
    float h = 0.f;
    if (KIND == 0 || entropy) h = self_info<LDC>(lp, pr, s, info);
    if (entropy) entropy[p] = h;
    float centre;                              // what the gradient's bracket subtracts: -H_nat or sum p^2
    if (KIND == 0) {
      local += (double)h;
      float a = 0.f;
#pragma unroll
      for (int c = 0; c < LDC; ++c) a += pr[c] > 0.f ? pr[c] * lp[c] : 0.f;
      centre = a;
    } else {
      float q = 0.f;
#pragma unroll
      for (int c = 0; c < LDC; ++c) q += pr[c] * pr[c];
      local += (double)q;
      centre = q;
    }
    if (dlogits) {
#pragma unroll
      for (int k = 0; k < LDC4; ++k) {
        f32x4 d;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int c = k * 4 + e;
          d[e] = pr[c] > 0.f ? coef * (pr[c] * ((KIND == 0 ? lp[c] : pr[c]) - centre)) : 0.f;
        }
        dlogits[p * LDC4 + k] = d;
      }
    }
  }
  block_partial(local, red, partials);
}

// Shared argument rules: the score buffer's shape, log C divides, and the map rows a convolution reads in place.
static bool advent_args_ok(const char* who, int64_t pixels, int classes, int ldc) {
  if (!scores_args_ok(who, pixels, classes, ldc, 32)) return false;
  if (classes < 2) {
    set_error("%s: need classes >= 2 (1 / log(classes) scales the maps; classes=%d)", who, classes);
    return false;
  }
  return true;
}
static bool map_row_ok(const char* who, int classes, int cpad, int bf16) {
  const int granule = bf16 ? 8 : 4;
  if (classes <= cpad && cpad <= 32 && cpad % granule == 0) return true;
  set_error("%s: need classes <= cpad <= 32, cpad %% %d == 0 for %s maps (classes=%d cpad=%d)", who, granule, bf16 ? "bf16" : "fp32",
            classes, cpad);
  return false;
}
static float inv_log(int classes) { return 1.f / logf((float)classes); }

}  // namespace udaseg

using namespace udaseg;

extern "C" int udaseg_selfinfo_fwd(const float* logits, int64_t pixels, int classes, int ldc, void* maps, int cpad, int out_bf16,
                                   float* entropy, void* stream) {
  if (!advent_args_ok("selfinfo_fwd", pixels, classes, ldc) || !map_row_ok("selfinfo_fwd", classes, cpad, out_bf16))
    return UDASEG_E_BADARG;
  UDASEG_CHECK_ARG(logits && maps, "selfinfo_fwd: NULL pointer");
  const int grid = capped_grid(pixels, 256, udaseg_seg_partials());
  if (!dispatch_width<8>(ldc / 4, [&](auto w) {
        constexpr int W = decltype(w)::value;
        hipLaunchKernelGGL((out_bf16 ? selfinfo_fwd_kernel<W, true> : selfinfo_fwd_kernel<W, false>), dim3(grid), dim3(256), 0,
                           as_stream(stream), (const f32x4*)logits, pixels, classes, inv_log(classes), maps, cpad, entropy);
      }))
    return unsupported_width("selfinfo_fwd", "ldc", ldc);
  UDASEG_LAUNCH_CHECK("selfinfo_fwd launch");
  return UDASEG_OK;
}

extern "C" int udaseg_selfinfo_bwd(const float* logits, const void* dmaps, int64_t pixels, int classes, int ldc, int cpad,
                                   int in_bf16, float* dlogits, void* stream) {
  if (!advent_args_ok("selfinfo_bwd", pixels, classes, ldc) || !map_row_ok("selfinfo_bwd", classes, cpad, in_bf16))
    return UDASEG_E_BADARG;
  UDASEG_CHECK_ARG(logits && dmaps && dlogits, "selfinfo_bwd: NULL pointer");
  const int grid = capped_grid(pixels, 256, udaseg_seg_partials());
  if (!dispatch_width<8>(ldc / 4, [&](auto w) {
        constexpr int W = decltype(w)::value;
        hipLaunchKernelGGL((in_bf16 ? selfinfo_bwd_kernel<W, true> : selfinfo_bwd_kernel<W, false>), dim3(grid), dim3(256), 0,
                           as_stream(stream), (const f32x4*)logits, dmaps, pixels, classes, inv_log(classes), cpad, (f32x4*)dlogits);
      }))
    return unsupported_width("selfinfo_bwd", "ldc", ldc);
  UDASEG_LAUNCH_CHECK("selfinfo_bwd launch");
  return UDASEG_OK;
}

extern "C" int udaseg_entropy_loss(const float* logits, int64_t pixels, int classes, int ldc, int kind, double* partials, float* loss,
                                   float* dlogits, float* entropy, void* stream) {
  if (!advent_args_ok("entropy_loss", pixels, classes, ldc)) return UDASEG_E_BADARG;
  UDASEG_CHECK_ARG(kind == 0 || kind == 1, "entropy_loss: kind must be 0 (entropy) or 1 (maximum squares), got %d", kind);
  UDASEG_CHECK_ARG(logits && partials && loss, "entropy_loss: NULL pointer");
  hipStream_t st = as_stream(stream);
  const int grid = capped_grid(pixels, 256, udaseg_seg_partials());
  const float s = inv_log(classes);
  const float coef = kind == 0 ? -(s / (float)pixels) : -(1.f / (float)pixels);
  if (!dispatch_width<8>(ldc / 4, [&](auto w) {
        constexpr int W = decltype(w)::value;
        hipLaunchKernelGGL((kind == 0 ? entropy_loss_kernel<W, 0> : entropy_loss_kernel<W, 1>), dim3(grid), dim3(256), 0, st,
                           (const f32x4*)logits, pixels, classes, s, coef, partials, (f32x4*)dlogits, entropy);
      }))
    return unsupported_width("entropy_loss", "ldc", ldc);
  UDASEG_LAUNCH_CHECK("entropy_loss launch");
  return launch_loss_finish(partials, grid, kind == 0 ? (double)pixels : -2.0 * (double)pixels, nullptr, loss, 0, st,
                            "entropy_finish launch");
}
