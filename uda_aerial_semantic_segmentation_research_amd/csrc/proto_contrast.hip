// Prototype contrast and structure losses on the decoder's features (ProDA, Zhang et al. 2021: structure learning; ProCA, Jiang et
// al., ECCV 2022; SePiCo, Xie et al. 2023; an extension: the reference has no feature-space component).  proto.hip READS the
// prototypes to clean the teacher's probabilities; here they shape the features: a pixel's soft assignment to the seen prototypes
//   d_c = |f - (float)proto_c|^2,  d* = min over the seen c,  a_c = -(d_c - d*) inv_tau,  L = log sum_seen exp(a_c),  s_c = exp(a_c - L)
// is an output of its own (udaseg_proto_assign: the teacher's assignment of the weak view) and the model distribution of a cross
// entropy against a hard label or a soft target (udaseg_proto_contrast_fwd_bwd), whose gradient goes to the FEATURES only:
//   l = sum_c t_c (-a_c) + T L,  T = sum_c t_c;   dl/df_j = 2 inv_tau sum_c (T s_c - t_c) P_cj
// (the f_j terms of sum_c (T s_c - t_c)(f_j - P_cj) cancel identically: sum_c (T s_c - t_c) = 0; the form without them has no
// cancellation against f and needs no feature row in the gradient pass).  With torch this is the [pixels, C, D] broadcast of
// proto.hip's header, differentiated; here both are ONE streaming pass, proto_rectify_kernel's shape: one lane per pixel,
// grid-stride, the prototypes staged once per block as fp32 in LDS and read as broadcasts, a template on the number of class
// vectors so that the class loops unroll, the channel loops rolled.  The distance pass holds 4 NV accumulator vectors; the
// gradient pass holds the 4 NV coefficients T s_c - t_c and ONE accumulator vector per channel quad: neither f nor d lives
// across it.  Weights and divisor are distill.hip's (udaseg_soft_ce_fwd_bwd), the block partials and the fixed-order loss scalar
// loss_reduce.h's: no float atomics, integer atomics for the counters only.  Measured (profiles/contrast_bench.txt, 8 x 512 x 512 pixels, 16 channels, 23
// classes): 0.195 ms, 3.4 x a device copy of the same bytes -- the pass is bound by its 3 C D multiply-adds and 2 C exponentials per
// pixel, not by its two streams; udaseg_proto_assign, the same pass without the gradient loop, takes 0.70 of it.
#include "loss_reduce.h"

namespace udaseg {

constexpr int PC_THREADS = 256;
static_assert(PC_THREADS == 256, "block_partial (loss_reduce.h) sums the four waves of a 256-thread block");
constexpr int PC_MAX_BLOCKS = 4096;       // udaseg_proto_assign: proto_rectify_kernel's grid
constexpr int PC_STATS = 4;               // counted, void by weight, void by label / target, void by a non-finite feature

// The block's prototypes as fp32 (the classes beyond `classes` of the last vector get zeros: their distances are computed and
// never used, and the loop over the channels has no branch) and the mask of the seen classes.  Ends in a barrier.
template <int NV>
__device__ __forceinline__ unsigned int stage_prototypes(const double* __restrict__ proto, const int* __restrict__ seen, int classes,
                                                         int dim, float* P, unsigned int* mask_slot) {
  if (threadIdx.x == 0) {
    unsigned int m = 0;
    for (int c = 0; c < classes; ++c) m |= (seen[c] != 0 ? 1u : 0u) << c;
    *mask_slot = m;
  }
  for (int i = threadIdx.x; i < 4 * NV * dim; i += PC_THREADS) P[i] = i < classes * dim ? (float)proto[i] : 0.f;
  __syncthreads();
  return *mask_slot;
}

// THE row routine of both entry points.  d_c in four chains, channel j in chain j % 4, folded as (s0 + s1) + (s2 + s3):
// proto_rectify_kernel's distances, bit for bit.  Then over the seen classes (sm != 0): a_c = -(d_c - d*) it, S = sum exp(a_c)
// in four chains (class c in chain c % 4), L = logf(S); an unseen class gets a_c = 0 and is in no sum.  a[] is written over d[].
// Returns whether every feature in a channel < dim is finite.
template <int NV>
__device__ __forceinline__ bool proto_row(const float* __restrict__ frow, const float* P, int dim, unsigned int sm, float it,
                                          float (&a)[4 * NV], float& L) {
  f32x4 d4[4 * NV];
#pragma unroll
  for (int c = 0; c < 4 * NV; ++c) d4[c] = f32x4{0.f, 0.f, 0.f, 0.f};
  bool fin = true;
  const int dv = dim >> 2;
#pragma unroll 1
  for (int q = 0; q < dv; ++q) {                           // rolled: 4 * NV accumulator vectors are live across it
    const f32x4 f = *reinterpret_cast<const f32x4*>(frow + 4 * q);
    fin &= __builtin_isfinite(f[0]) & __builtin_isfinite(f[1]) & __builtin_isfinite(f[2]) & __builtin_isfinite(f[3]);
    const float* pq = P + 4 * q;
#pragma unroll
    for (int c = 0; c < 4 * NV; ++c) {
      const f32x4 t = f - *reinterpret_cast<const f32x4*>(pq + c * dim);
#pragma unroll
      for (int e = 0; e < 4; ++e) d4[c][e] = fmaf(t[e], t[e], d4[c][e]);
    }
  }
  {
#pragma clang fp contract(off)
    float dmin = INFINITY;
#pragma unroll
    for (int c = 0; c < 4 * NV; ++c) {
      a[c] = (d4[c][0] + d4[c][1]) + (d4[c][2] + d4[c][3]);
      dmin = ((sm >> c) & 1u) ? fminf(dmin, a[c]) : dmin;
    }
    f32x4 s4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 4 * NV; ++c) {
      const bool in = ((sm >> c) & 1u) != 0u;
      a[c] = in ? -(a[c] - dmin) * it : 0.f;
      s4[c & 3] += in ? expf(a[c]) : 0.f;                  // exactly 1 at the nearest seen prototype: S >= 1 whenever it is a number
    }
    L = logf((s4[0] + s4[1]) + (s4[2] + s4[3]));
  }
  return fin;
}

template <int NV>
__global__ __launch_bounds__(PC_THREADS) void proto_assign_kernel(const float* __restrict__ feat, int ldf, int dim, int classes, int ldc,
                                                                  const double* __restrict__ proto, const int* __restrict__ seen,
                                                                  const float* __restrict__ inv_tau, int64_t pixels,
                                                                  float* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) float P[32 * 64];
  __shared__ unsigned int seen_mask;
  const unsigned int sm = stage_prototypes<NV>(proto, seen, classes, dim, P, &seen_mask);
  const unsigned int all = classes >= 32 ? 0xffffffffu : (1u << classes) - 1u;
  const float it = inv_tau[0];
  const float uniform = 1.f / (float)classes;              // while no class is seen: rectify's "u = 1 for all"
  const int lv = ldc >> 2;
  const float qnan = __builtin_nanf("");
  for (int64_t p = (int64_t)blockIdx.x * PC_THREADS + threadIdx.x; p < pixels; p += (int64_t)gridDim.x * PC_THREADS) {
    float a[4 * NV];
    float L;
    const bool ok = proto_row<NV>(feat + p * ldf, P, dim, sm, it, a, L);
    float* orow = out + p * ldc;
#pragma unroll
    for (int q = 0; q < NV; ++q) {
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int c = 4 * q + e;
        const float s = sm ? (((sm >> c) & 1u) ? expf(a[c] - L) : 0.f) : uniform;
        o[e] = ((all >> c) & 1u) ? (ok ? s : qnan) : 0.f;
      }
      *reinterpret_cast<f32x4*>(orow + 4 * q) = o;
    }
    for (int q = NV; q < lv; ++q) *reinterpret_cast<f32x4*>(orow + 4 * q) = f32x4{0.f, 0.f, 0.f, 0.f};
  }
}

// distill.hip's pixel_weight, restated: w_p and whether it voids the pixel (0 = counts, 1 = zero, negative or not finite).
// udaseg_pixel_weight_sum counts the same pixels into the denominator.
__device__ __forceinline__ bool contrast_weight_void(const float* __restrict__ wpx, const float* __restrict__ wimg, int64_t p,
                                                     int64_t ppi, float& w) {
#pragma clang fp contract(off)
  w = wpx ? wpx[p] : 1.f;
  if (wimg) w = w * wimg[(int64_t)((uint32_t)p / (uint32_t)ppi)];        // pixels < 2^31
  return !(w > 0.f && __builtin_isfinite(w));
}

template <int NV, bool SOFT>
__global__ __launch_bounds__(PC_THREADS) void proto_contrast_kernel(const float* __restrict__ feat, int ldf, int dim,
                                                                    const uint8_t* __restrict__ labels,
                                                                    const float* __restrict__ target, int ldt,
                                                                    const float* __restrict__ wpx, const float* __restrict__ wimg,
                                                                    int64_t pixels, int64_t ppi, int classes,
                                                                    const double* __restrict__ proto, const int* __restrict__ seen,
                                                                    const float* __restrict__ inv_tau, int mean,
                                                                    const double* __restrict__ denom, double* __restrict__ partials,
                                                                    float* __restrict__ dfeat, unsigned long long* __restrict__ stats) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) float P[32 * 64];
  __shared__ unsigned int seen_mask;
  __shared__ double red[PC_THREADS / 64];
  const unsigned int sm = stage_prototypes<NV>(proto, seen, classes, dim, P, &seen_mask);
  const float it = inv_tau[0];
  const bool on = it > 0.f;                                // inv_tau == 0 (no temperature yet): the whole call is 0
  const float scale = mean ? 1.f / (float)pixels : (denom ? (float)(1.0 / *denom) : 1.f);
  const int dv = dim >> 2, lf = ldf >> 2;
  const int tid = threadIdx.x;
  double local = 0.0;
  unsigned int cnt[PC_STATS] = {0u, 0u, 0u, 0u};
  for (int64_t p = (int64_t)blockIdx.x * PC_THREADS + tid; p < pixels; p += (int64_t)gridDim.x * PC_THREADS) {
    float w;
    int why = contrast_weight_void(wpx, wimg, p, ppi, w) ? 1 : 0;
    float k[4 * NV];                                       // a_c, then T s_c - t_c
    float T = 1.f, fwd = 0.f, L = 0.f;
    if (why == 0) {
      const bool fin = proto_row<NV>(feat + p * ldf, P, dim, sm, it, k, L);
      bool bad = false;
      if (SOFT) {
        f32x4 tv[NV];
        load_row<NV>(target + p * ldt, tv);
        f32x4 t4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int q = 0; q < NV; ++q)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int c = 4 * q + e;
            const float x = tv[q][e];
            if (c < classes) bad |= !(x >= 0.f && x <= 1.f);          // a NaN fails both comparisons
            const float t = ((sm >> c) & 1u) ? x : 0.f;               // the mass on unseen classes is dropped
            t4[e] += t;
            fwd += t > 0.f ? t * -k[c] : 0.f;
            tv[q][e] = t;
          }
        T = (t4[0] + t4[1]) + (t4[2] + t4[3]);
        bad |= T == 0.f;
#pragma unroll
        for (int c = 0; c < 4 * NV; ++c) {
          const float s = ((sm >> c) & 1u) ? expf(k[c] - L) : 0.f;
          k[c] = T * s - tv[c >> 2][c & 3];
        }
        fwd = fwd + T * L;
      } else {
        const int lab = labels[p];
        bad = lab >= classes || ((sm >> lab) & 1u) == 0u;
#pragma unroll
        for (int c = 0; c < 4 * NV; ++c) {
          fwd = c == lab ? -k[c] : fwd;                    // (d_y - d*) inv_tau
          const float s = ((sm >> c) & 1u) ? expf(k[c] - L) : 0.f;
          k[c] = s - (c == lab ? 1.f : 0.f);
        }
        fwd = fwd + L;
      }
      why = bad ? 2 : (fin ? 0 : 3);
    }
#pragma unroll
    for (int s = 0; s < PC_STATS; ++s) cnt[s] += why == s;
    const bool live = why == 0 && on;
    if (live) local += (double)(w * fwd);
    if (dfeat) {
      float* grow = dfeat + p * ldf;
      int q0 = 0;
      if (live) {
        const float coef = (2.f * it) * (scale * w);
#pragma unroll 1
        for (int q = 0; q < dv; ++q) {                     // rolled: 4 * NV coefficients and one accumulator vector are live
          const float* pq = P + 4 * q;
          f32x4 g = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int c = 0; c < 4 * NV; ++c) {
            const f32x4 pc = *reinterpret_cast<const f32x4*>(pq + c * dim);
#pragma unroll
            for (int e = 0; e < 4; ++e) g[e] = fmaf(k[c], pc[e], g[e]);
          }
          *reinterpret_cast<f32x4*>(grow + 4 * q) = coef * g;
        }
        q0 = dv;
      }
      for (int q = q0; q < lf; ++q) *reinterpret_cast<f32x4*>(grow + 4 * q) = f32x4{0.f, 0.f, 0.f, 0.f};   // void: all ldf lanes
    }
  }
  block_partial(local, red, partials);
  if (stats) {
#pragma unroll
    for (int s = 0; s < PC_STATS; ++s) {
      const unsigned int n = wave_sum_u32(cnt[s]);       // per wave, not BlockCounts: that cost +33 instructions a variant
      if ((tid & 63) == 0 && n) atomicAdd(&stats[s], (unsigned long long)n);   // (profiles/loss_reduce_refactor.txt)
    }
  }
}

}  // namespace udaseg

using namespace udaseg;

extern "C" int udaseg_proto_assign(const float* feat, int ldf, int dim, int classes, int ldc, const double* proto, const int32_t* seen,
                                   const float* inv_tau, int64_t pixels, float* out, void* stream) {
  if (!proto_feat_ok("proto_assign", pixels, classes, dim, ldf)) return UDASEG_E_BADARG;
  if (!scores_args_ok("proto_assign", pixels, classes, ldc)) return UDASEG_E_BADARG;
  UDASEG_CHECK_ARG(feat && proto && seen && inv_tau && out, "proto_assign: NULL pointer");
  UDASEG_CHECK_ARG(((reinterpret_cast<uintptr_t>(feat) | reinterpret_cast<uintptr_t>(out)) & 15) == 0,
                   "proto_assign: feat and out must be 16-byte aligned");
  const int gx = capped_grid(pixels, PC_THREADS, PC_MAX_BLOCKS);
  if (!dispatch_width<8>(cdiv(classes, 4), [&](auto w) {
        hipLaunchKernelGGL(proto_assign_kernel<decltype(w)::value>, dim3(gx), dim3(PC_THREADS), 0, as_stream(stream), feat, ldf, dim,
                           classes, ldc, proto, seen, inv_tau, pixels, out);
      }))
    return unsupported_width("proto_assign", "classes", classes);
  UDASEG_LAUNCH_CHECK("proto_assign launch");
  return UDASEG_OK;
}

extern "C" int udaseg_proto_contrast_fwd_bwd(const float* feat, int ldf, int dim, const uint8_t* labels, const float* target, int ldt,
                                             const float* weight_px, const float* weight_img, int batch, int64_t pix_per_image,
                                             int classes, const double* proto, const int32_t* seen, const float* inv_tau, int mean,
                                             const double* denom, double* partials, float* loss, float* dfeat, int64_t* stats,
                                             void* stream) {
  if (!image_grid_ok("proto_contrast_fwd_bwd", batch, pix_per_image)) return UDASEG_E_BADARG;
  const int64_t pixels = (int64_t)batch * pix_per_image;
  if (!proto_feat_ok("proto_contrast_fwd_bwd", pixels, classes, dim, ldf)) return UDASEG_E_BADARG;
  UDASEG_CHECK_ARG((labels != nullptr) != (target != nullptr),
                   "proto_contrast_fwd_bwd: exactly one of labels (hard) and target (soft) must be given");
  if (target && !scores_args_ok("proto_contrast_fwd_bwd", pixels, classes, ldt, INT_MAX, "ldt")) return UDASEG_E_BADARG;
  UDASEG_CHECK_ARG(feat && proto && seen && inv_tau && partials && loss, "proto_contrast_fwd_bwd: NULL pointer");
  UDASEG_CHECK_ARG(((reinterpret_cast<uintptr_t>(feat) | reinterpret_cast<uintptr_t>(target) | reinterpret_cast<uintptr_t>(dfeat)) & 15) == 0,
                   "proto_contrast_fwd_bwd: feat, target and dfeat must be 16-byte aligned");
  UDASEG_CHECK_ARG(!(mean && denom), "proto_contrast_fwd_bwd: mean (divide by pixels) and denom (divide by *denom) exclude each other");
  hipStream_t st = as_stream(stream);
  const int grid = capped_grid(pixels, PC_THREADS, udaseg_seg_partials());
  if (!dispatch_width<8>(cdiv(classes, 4), [&](auto w) {
        constexpr int NV = decltype(w)::value;
        hipLaunchKernelGGL((target ? proto_contrast_kernel<NV, true> : proto_contrast_kernel<NV, false>), dim3(grid), dim3(PC_THREADS),
                           0, st, feat, ldf, dim, labels, target, ldt, weight_px, weight_img, pixels, pix_per_image, classes, proto,
                           seen, inv_tau, mean, denom, partials, dfeat, (unsigned long long*)stats);
      }))
    return unsupported_width("proto_contrast_fwd_bwd", "classes", classes);
  UDASEG_LAUNCH_CHECK("proto_contrast launch");
  // mean and denom exclude each other (above): D = pixels, *denom or 1
  return launch_loss_finish(partials, grid, mean ? (double)pixels : 1.0, denom, loss, 0, st, "proto_contrast_finish launch");
}
