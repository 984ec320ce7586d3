// Calibration of the winner's confidence on the device: reliability tables, expected calibration error, temperature fit.
// (The reference copies softmax(outputs) to the host and bins it with numpy.)  The self-training recipes threshold, count and
// weight the winner's softmax probability; these kernels measure whether a confidence of 0.9 means 90 % correct and fit the one
// scalar -- the reciprocal temperature beta -- that corrects it.
//
// One definition of the confidence, scores_common.h's: c^ = first_max, m = z[c^],
//     p = 1 / sum_{j < classes} expf((z_j - m) * beta)        (four partial sums by j % 4, then (s0 + s1) + (s2 + s3))
// With inv_temp == NULL this IS pixel_conf (the function is called), so a reliability table, a pseudo-label threshold and a
// confidence share cannot disagree; with probs the buffer holds probabilities and p = the winner's value (pixel_conf again).
// beta is read from device memory (PrototypeBank.inv_tau's pattern): a fitted value flows into the next launch without a host read.
// A beta that is not a positive finite number makes every pixel NON-FINITE (it lands in counters[2], in no table and in no sum).
//
// udaseg_calib_hist   one pass; tables uint64 [3][classes][bins] by the PREDICTED class: count, correct, conf_q (the confidence in
//                     2^-24 fixed point): integer sums, independent of order, the same on every run.
// udaseg_calib_finish one block: N, accuracy, mean confidence, ECE, MCE, gap and the per-class rows, float64, fixed order.
// udaseg_calib_nll    one pass; n, sum nll, sum d nll / d beta, sum d^2 nll / d beta^2 as float64 block partials in the fixed
//                     order of loss_reduce.h, folded by a single wave and ADDED into sums.
// udaseg_calib_step   one thread: the guarded Newton step on beta.
#include <float.h>

#include "loss_reduce.h"

namespace udaseg {

__device__ __forceinline__ float load_beta(const float* __restrict__ inv_temp) {
  if (!inv_temp) return 1.f;
  const float b = *inv_temp;
  return (b > 0.f && b <= FLT_MAX) ? b : NAN;
}

// pixel_conf at a temperature: its order of operations with the exponent scaled by beta
template <int NV>
__device__ __forceinline__ PixelConf pixel_conf_at(const float* __restrict__ row, int classes, float beta) {
  f32x4 v[NV];
  load_row<NV>(row, v);
  float m;
  PixelConf r;
  r.cls = first_max<NV>(v, classes, m);
  f32x4 s4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int q = 0; q < NV; ++q)
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (4 * q + e < classes) s4[e] += expf((v[q][e] - m) * beta);
  const float S = (s4[0] + s4[1]) + (s4[2] + s4[3]);
  r.p = 1.f / S;
  r.finite = __builtin_isfinite(r.p);
  return r;
}

// The block's cells live in LDS, [classes][bins] <= 32 x 64 = 2048 of them: 32-bit count and correct, 64-bit conf_q (32 KiB).  One
// cell per pixel (score_hist_kernel has one per class), so no class groups.  Few, long blocks: a block flushes three 64-bit global
// atomics per NON-EMPTY cell, so its pixel count has to be large against its cell count.
constexpr int CH_CELLS = 2048;
constexpr int CH_THREADS = 256;
static_assert(CH_THREADS == 64 * 4, "BlockCounts<K>: four waves a block");
constexpr int CH_BLOCKS = 512;

template <int NV>
__global__ __launch_bounds__(CH_THREADS) void calib_hist_kernel(const float* __restrict__ scores, const int64_t* __restrict__ target,
                                                                int64_t pixels, int classes, int ldc, int probs,
                                                                const float* __restrict__ inv_temp, int bins,
                                                                unsigned long long* __restrict__ tables,
                                                                unsigned long long* __restrict__ counters) {
  __shared__ unsigned int cnt[CH_CELLS], cor[CH_CELLS];
  __shared__ unsigned long long cq[CH_CELLS];
  __shared__ BlockCounts<3>::Slots cred;
  const int cells = classes * bins;                        // <= CH_CELLS (checked by the entry point)
  for (int i = threadIdx.x; i < cells; i += CH_THREADS) {
    cnt[i] = 0;
    cor[i] = 0;
    cq[i] = 0;
  }
  __syncthreads();
  const float beta = load_beta(inv_temp);
  const float fbins = (float)bins;
  unsigned int nvoid = 0, nbad = 0, nval = 0;
  const int64_t T = (int64_t)gridDim.x * CH_THREADS;
  for (int64_t p = (int64_t)blockIdx.x * CH_THREADS + threadIdx.x; p < pixels; p += T) {
    const int64_t t64 = target[p];
    if (t64 < 0 || t64 >= classes) {
      ++nvoid;
      continue;
    }
    const float* row = scores + p * ldc;
    const PixelConf r = inv_temp ? pixel_conf_at<NV>(row, classes, beta) : pixel_conf<NV>(row, classes, probs);
    if (!(r.finite && r.p >= 0.f && r.p <= 1.f)) {
      ++nbad;
      continue;
    }
    const int b = min((int)floorf(r.p * fbins), bins - 1);
    const int cell = r.cls * bins + b;
    atomicAdd(&cnt[cell], 1u);
    if (r.cls == (int)t64) atomicAdd(&cor[cell], 1u);
    atomicAdd(&cq[cell], (unsigned long long)__float2uint_rn(r.p * 16777216.f));
    ++nval;
  }
  const unsigned int ev[3] = {nval, nvoid, nbad};         // counters[0]: the pixels in the tables
  BlockCounts<3>::add(cred, ev, counters);                 // its barrier also closes the LDS tables
  const size_t plane = (size_t)cells;
  for (int i = threadIdx.x; i < cells; i += CH_THREADS) {
    const unsigned int n = cnt[i];
    if (n) {
      atomicAdd(&tables[i], (unsigned long long)n);
      if (cor[i]) atomicAdd(&tables[plane + i], (unsigned long long)cor[i]);
      atomicAdd(&tables[2 * plane + i], cq[i]);
    }
  }
}

// One block of 64 threads.  Thread b < bins sums bin b over the classes in class order, thread c < classes walks class c's bins in
// bin order (integers: exact); thread 0 then folds the bins b = 0 .. bins - 1 in that order in float64.
constexpr double CQ_UNIT = 1.0 / 16777216.0;

__global__ __launch_bounds__(64) void calib_finish_kernel(const unsigned long long* __restrict__ tables, int classes, int bins,
                                                          double* __restrict__ out, double* __restrict__ per_class) {
  __shared__ unsigned long long sn[64], sa[64], sq[64];
  const int j = threadIdx.x;
  const size_t plane = (size_t)classes * bins;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  if (j < bins) {
    unsigned long long n = 0, a = 0, q = 0;
    for (int c = 0; c < classes; ++c) {
      n += tables[(size_t)c * bins + j];
      a += tables[plane + (size_t)c * bins + j];
      q += tables[2 * plane + (size_t)c * bins + j];
    }
    sn[j] = n;
    sa[j] = a;
    sq[j] = q;
  }
  if (j < classes) {
    unsigned long long n = 0, a = 0, q = 0;
    double e = 0.0;
    for (int b = 0; b < bins; ++b) {
      const unsigned long long nb = tables[(size_t)j * bins + b], ab = tables[plane + (size_t)j * bins + b],
                               qb = tables[2 * plane + (size_t)j * bins + b];
      n += nb;
      a += ab;
      q += qb;
      e += fabs((double)ab - (double)qb * CQ_UNIT);
    }
    const double dn = (double)n;
    per_class[j] = dn;
    per_class[classes + j] = n ? (double)a / dn : nan;
    per_class[2 * classes + j] = n ? (double)q * CQ_UNIT / dn : nan;
    per_class[3 * classes + j] = n ? e / dn : nan;
  }
  __syncthreads();
  if (j == 0) {
    unsigned long long N = 0, A = 0, Q = 0;
    double e = 0.0, mce = nan;
    for (int b = 0; b < bins; ++b) {
      N += sn[b];
      A += sa[b];
      Q += sq[b];
      const double ab = (double)sa[b], qb = (double)sq[b] * CQ_UNIT;
      e += fabs(ab - qb);
      if (sn[b]) {
        const double nb = (double)sn[b];
        const double g = fabs(ab / nb - qb / nb);
        if (!(mce >= g)) mce = g;                          // also the first non-empty bin, over the NaN
      }
    }
    const double dn = (double)N;
    const double acc = N ? (double)A / dn : nan, conf = N ? (double)Q * CQ_UNIT / dn : nan;
    out[0] = dn;
    out[1] = acc;
    out[2] = conf;
    out[3] = N ? e / dn : nan;
    out[4] = mce;
    out[5] = conf - acc;
  }
}

// Per valid pixel, fp32, with d_j = z_j - m, e_j = expf(beta d_j) and S, A = sum e_j d_j, B = sum e_j d_j^2 each as four partial sums
// by j % 4:  nll = logf(S) - beta d_t,  mu = A / S,  g1 = mu - d_t,  g2 = B / S - mu^2.  A thread adds its pixels' terms in float64
// in pixel order; block and grid as loss_reduce.h defines them.
template <int NV>
__global__ __launch_bounds__(256) void calib_nll_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                                                        int64_t pixels, int classes, int ldc, const float* __restrict__ inv_temp,
                                                        double* __restrict__ partials, unsigned long long* __restrict__ counters) {
  __shared__ double red[4][4];
  __shared__ BlockCounts<2>::Slots cred;
  const float beta = load_beta(inv_temp);
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  unsigned int nvoid = 0, nbad = 0;
  const int64_t T = (int64_t)gridDim.x * 256;
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < pixels; p += T) {
    const int64_t t64 = target[p];
    if (t64 < 0 || t64 >= classes) {
      ++nvoid;
      continue;
    }
    const int t = (int)t64;
    f32x4 v[NV];
    load_row<NV>(logits + p * ldc, v);
    float m;
    first_max<NV>(v, classes, m);
    f32x4 s4 = {0.f, 0.f, 0.f, 0.f}, a4 = s4, b4 = s4;
    float dt = 0.f;
#pragma unroll
    for (int q = 0; q < NV; ++q)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int c = 4 * q + e;
        if (c < classes) {
          const float d = v[q][e] - m;
          const float ex = expf(beta * d);
          const float ed = ex * d;
          s4[e] += ex;
          a4[e] += ed;
          b4[e] += ed * d;
          if (c == t) dt = d;
        }
      }
    const float S = (s4[0] + s4[1]) + (s4[2] + s4[3]);
    const float A = (a4[0] + a4[1]) + (a4[2] + a4[3]);
    const float B = (b4[0] + b4[1]) + (b4[2] + b4[3]);
    const float nll = logf(S) - beta * dt;
    const float mu = A / S;
    const float g1 = mu - dt;
    const float g2 = B / S - mu * mu;
    if (__builtin_isfinite(nll) && __builtin_isfinite(g1) && __builtin_isfinite(g2)) {
      acc[0] += 1.0;
      acc[1] += (double)nll;
      acc[2] += (double)g1;
      acc[3] += (double)g2;
    } else {
      ++nbad;
    }
  }
  const unsigned int ev[2] = {nvoid, nbad};
  BlockCounts<2>::put(cred, ev);
  block_partial_rows<4>(acc, red, partials);               // its barrier is the counters' too
  BlockCounts<2>::flush(cred, counters + 1);               // counters[1], counters[2]
}

// single wave over partials[4][n]: lane l sums partials[k][l], partials[k][l + 64], ..., then wave_sum_d; sums[k] += that
__global__ void calib_nll_finish_kernel(const double* __restrict__ partials, int n, double* __restrict__ sums,
                                        unsigned long long* __restrict__ counters) {
  double s[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    double a = 0.0;
    for (int i = threadIdx.x; i < n; i += 64) a += partials[(size_t)k * n + i];
    s[k] = wave_sum_d(a);
  }
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) sums[k] += s[k];
    counters[0] += (unsigned long long)s[0];               // a whole number < 2^31: exact
  }
}

__global__ void calib_step_kernel(double* __restrict__ sums, float* __restrict__ inv_temp, double* __restrict__ state) {
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  const double n = sums[0], l = sums[1], g1 = sums[2], g2 = sums[3];
  const float b32 = *inv_temp;
  const double beta = (double)b32;
  double moved = 0.0;
  const bool ok = n > 0.0 && __builtin_isfinite(n) && __builtin_isfinite(l) && __builtin_isfinite(g1) && __builtin_isfinite(g2) &&
                  g2 > 0.0 && beta > 0.0 && __builtin_isfinite(beta);
  if (ok) {
    double bn = beta - g1 / g2;
    bn = fmin(fmax(bn, beta / 4.0), 4.0 * beta);
    bn = fmin(fmax(bn, 1.0 / 64.0), 64.0);
    const float out = (float)bn;
    *inv_temp = out;
    moved = (double)out - beta;
  }
  state[0] = n > 0.0 ? l / n : nan;
  state[1] = n > 0.0 ? g1 / n : nan;
  state[2] = moved;
  state[3] = state[3] + 1.0;
  sums[0] = sums[1] = sums[2] = sums[3] = 0.0;
}

static inline bool calib_scores_ok(const char* who, const void* scores, const void* target, int64_t pixels, int classes, int ldc) {
  if (!scores_args_ok(who, pixels, classes, ldc)) return false;
  if (pixels >= ((int64_t)1 << 31)) {
    set_error("%s: need pixels < 2^31 (pixels=%lld)", who, (long long)pixels);
    return false;
  }
  if (!scores || !target) {
    set_error("%s: NULL pointer", who);
    return false;
  }
  if (reinterpret_cast<uintptr_t>(scores) & 15) {
    set_error("%s: the score buffer must be 16-byte aligned", who);
    return false;
  }
  return true;
}

}  // namespace udaseg

using namespace udaseg;

extern "C" int udaseg_calib_hist(const float* scores, const int64_t* target, int64_t pixels, int classes, int ldc, int probs,
                                 const float* inv_temp, int bins, int64_t* tables, int64_t* counters, void* stream) {
  if (!calib_scores_ok("calib_hist", scores, target, pixels, classes, ldc)) return UDASEG_E_BADARG;
  UDASEG_CHECK_ARG(tables && counters, "calib_hist: NULL pointer");
  UDASEG_CHECK_ARG(probs == 0 || probs == 1, "calib_hist: probs must be 0 (logits) or 1 (probabilities), got %d", probs);
  UDASEG_CHECK_ARG(!(probs && inv_temp), "calib_hist: probabilities take no temperature (probs=1 needs inv_temp == NULL)");
  UDASEG_CHECK_ARG(bins >= 2 && bins <= 64, "calib_hist: need 2 <= bins <= 64 (bins=%d)", bins);
  hipStream_t st = as_stream(stream);
  const int grid = capped_grid(pixels, CH_THREADS, CH_BLOCKS);
  if (!dispatch_width<8>(cdiv(classes, 4), [&](auto w) {
        hipLaunchKernelGGL(calib_hist_kernel<decltype(w)::value>, dim3(grid), dim3(CH_THREADS), 0, st, scores, target, pixels, classes,
                           ldc, probs, inv_temp, bins, (unsigned long long*)tables, (unsigned long long*)counters);
      }))
    return unsupported_width("calib_hist", "classes", classes);
  UDASEG_LAUNCH_CHECK("calib_hist launch");
  return UDASEG_OK;
}

extern "C" int udaseg_calib_finish(const int64_t* tables, int classes, int bins, double* out, double* per_class, void* stream) {
  UDASEG_CHECK_ARG(tables && out && per_class, "calib_finish: NULL pointer");
  UDASEG_CHECK_ARG(classes > 0 && classes <= 32, "calib_finish: need 0 < classes <= 32 (classes=%d)", classes);
  UDASEG_CHECK_ARG(bins >= 2 && bins <= 64, "calib_finish: need 2 <= bins <= 64 (bins=%d)", bins);
  hipLaunchKernelGGL(calib_finish_kernel, dim3(1), dim3(64), 0, as_stream(stream), (const unsigned long long*)tables, classes, bins, out,
                     per_class);
  UDASEG_LAUNCH_CHECK("calib_finish launch");
  return UDASEG_OK;
}

extern "C" int udaseg_calib_nll(const float* logits, const int64_t* target, int64_t pixels, int classes, int ldc, const float* inv_temp,
                                double* partials, double* sums, int64_t* counters, void* stream) {
  if (!calib_scores_ok("calib_nll", logits, target, pixels, classes, ldc)) return UDASEG_E_BADARG;
  UDASEG_CHECK_ARG(partials && sums && counters, "calib_nll: NULL pointer");
  hipStream_t st = as_stream(stream);
  const int grid = capped_grid(pixels, 256, udaseg_seg_partials());
  if (!dispatch_width<8>(cdiv(classes, 4), [&](auto w) {
        hipLaunchKernelGGL(calib_nll_kernel<decltype(w)::value>, dim3(grid), dim3(256), 0, st, logits, target, pixels, classes, ldc,
                           inv_temp, partials, (unsigned long long*)counters);
      }))
    return unsupported_width("calib_nll", "classes", classes);
  UDASEG_LAUNCH_CHECK("calib_nll launch");
  hipLaunchKernelGGL(calib_nll_finish_kernel, dim3(1), dim3(64), 0, st, (const double*)partials, grid, sums,
                     (unsigned long long*)counters);
  UDASEG_LAUNCH_CHECK("calib_nll_finish launch");
  return UDASEG_OK;
}

extern "C" int udaseg_calib_step(double* sums, float* inv_temp, double* state, void* stream) {
  UDASEG_CHECK_ARG(sums && inv_temp && state, "calib_step: NULL pointer");
  hipLaunchKernelGGL(calib_step_kernel, dim3(1), dim3(1), 0, as_stream(stream), sums, inv_temp, state);
  UDASEG_LAUNCH_CHECK("calib_step launch");
  return UDASEG_OK;
}
