// Per-class ROC / PR curves on the device (the reference's _log_roc_curves / _log_pr_curves, src/models/train.py:245-328, sort
// softmax(outputs) on the host class by class with sklearn).  Here: ONE pass over the logits makes a per-class histogram of the
// score, a second tiny kernel turns the histogram into AUC, AP and an error bound.  No sort, integer counters only.
//
// Score of class c at a pixel with logits z: the log-odds of the softmax probability,
//     s_c = z_c - log(sum_{j != c} exp(z_j))          (strictly increasing in p_c, so the curves are those of p_c)
// computed without cancellation: m = max z, e_j = exp(z_j - m), S = sum e_j, S' = sum_{j != argmax} e_j; the "others" term is
// S' for c = argmax and S - e_c (>= 1) otherwise.  Grid: `bins` uniform bins over [-range, range),
//     bin = clamp(floor((s + range) * bins / (2 range)), 0, bins - 1)
// so scores beyond the range fall into the end bins; a NaN score is counted in bin 0 (fmaxf(NaN, 0) = 0).
// pos[c][b] counts the pixels of target c, neg[c][b] the pixels of every other valid target; a pixel whose target is outside
// [0, classes) is left out of every table (the rule of argmax_confusion_kernel).  Both tables ACCUMULATE.
#include "scores_common.h"

namespace udaseg {

// The block's counters live in LDS: 64 KiB = 16384 32-bit cells = [cg][2][bins] for cg = 8192 / bins classes (4 at 2048 bins).
// The classes are split into groups of cg over blockIdx.y; every group re-reads the logits and recomputes the row's softmax
// terms (23 classes, 2048 bins: 6 passes over the logits, still a fraction of a millisecond at HBM rate).  Few, long blocks: a
// block flushes one 64-bit global atomic per NON-EMPTY cell, so its pixel count has to be large against its cell count.
constexpr int SH_CELLS = 16384;
constexpr int SH_THREADS = 512;
constexpr int SH_TOTAL_BLOCKS = 1024;

template <int LDC4>
__global__ __launch_bounds__(SH_THREADS) void score_hist_kernel(const f32x4* __restrict__ logits, const int64_t* __restrict__ target,
                                                                int64_t pixels, int classes, int bins, int cg, float range,
                                                                float scale, unsigned long long* __restrict__ pos,
                                                                unsigned long long* __restrict__ neg) {
  constexpr int LDC = LDC4 * 4;
  __shared__ unsigned int hist[SH_CELLS];
  const int c0 = blockIdx.y * cg;
  const int nc = min(cg, classes - c0);
  const int cells = nc * 2 * bins;                       // <= SH_CELLS: cg * 2 * bins == SH_CELLS
  for (int i = threadIdx.x; i < cells; i += SH_THREADS) hist[i] = 0;
  __syncthreads();
  const float top = (float)(bins - 1);
  const int64_t T = (int64_t)gridDim.x * SH_THREADS;
  for (int64_t p = (int64_t)blockIdx.x * SH_THREADS + threadIdx.x; p < pixels; p += T) {
    const int64_t t64 = target[p];
    if (t64 < 0 || t64 >= classes) continue;
    const int t = (int)t64;
    f32x4 v[LDC4];
    load_row<LDC4>(logits + p * LDC4, v);
    float m;
    const int am = first_max<LDC4>(v, classes, m);
    float z[LDC];
    float S = 0.f, Sp = 0.f;
#pragma unroll
    for (int c = 0; c < LDC; ++c) {
      z[c] = v[c / 4][c % 4] - m;                        // <= 0; exactly 0 at the argmax
      if (c < classes) {
        const float e = expf(z[c]);
        S += e;
        if (c != am) Sp += e;
      }
    }
#pragma unroll
    for (int c = 0; c < LDC; ++c) {
      if (c >= c0 && c < c0 + nc) {                      // uniform over the block
        const float others = c == am ? Sp : S - expf(z[c]);
        const float s = z[c] - logf(others);
        const float x = floorf((s + range) * scale);
        const int b = (int)fminf(fmaxf(x, 0.f), top);    // NaN -> 0
        atomicAdd(&hist[((c - c0) * 2 + (c == t ? 0 : 1)) * bins + b], 1u);
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < cells; i += SH_THREADS) {
    const unsigned int v = hist[i];
    if (v) {
      const int row = i / bins, b = i - row * bins;      // row = 2 * (class in the group) + (0 = pos, 1 = neg)
      unsigned long long* dst = (row & 1) ? neg : pos;
      atomicAdd(&dst[(size_t)(c0 + (row >> 1)) * bins + b], (unsigned long long)v);
    }
  }
}

// One block per class.  Bins are walked from the top (highest score first): tp_k, fp_k = running sums of pos, neg.
//   auc   = trapezoid over (fpr, tpr) from (0, 0)  = sum_b neg_b * (tp_{k-1} + tp_k) / (2 P N)
//   ap    = sum over the non-empty bins of (recall_k - recall_{k-1}) * precision_k = sum_b pos_b * tp_k / (tp_k + fp_k) / P
//   slack = 0.5 * sum_b pos_b * neg_b / (P N)         (|auc - auc of the un-quantised score| <= slack)
// Thread j owns the j-th chunk of bins / 256 bins from the top; the chunk sums are scanned in LDS, the three float64 sums are
// folded by a fixed tree: the result does not depend on timing.  auc and slack are NaN when P == 0 or N == 0, ap when P == 0.
constexpr int CF_THREADS = 256;

__global__ __launch_bounds__(CF_THREADS) void curve_finish_kernel(const unsigned long long* __restrict__ pos,
                                                                  const unsigned long long* __restrict__ neg, int bins,
                                                                  double* __restrict__ auc, double* __restrict__ ap,
                                                                  double* __restrict__ slack,
                                                                  unsigned long long* __restrict__ support) {
  __shared__ unsigned long long sp[CF_THREADS], sn[CF_THREADS];
  __shared__ double red[3][CF_THREADS];
  const int c = blockIdx.x, j = threadIdx.x;
  const int per = bins / CF_THREADS;
  const unsigned long long* pc = pos + (size_t)c * bins;
  const unsigned long long* nc = neg + (size_t)c * bins;
  const int hi = bins - 1 - j * per;                     // this thread's bins: hi, hi - 1, ..., hi - per + 1
  unsigned long long a = 0, b = 0;
  for (int i = 0; i < per; ++i) {
    a += pc[hi - i];
    b += nc[hi - i];
  }
  sp[j] = a;
  sn[j] = b;
  __syncthreads();
  unsigned long long tp = 0, fp = 0, P = 0, N = 0;
  for (int i = 0; i < CF_THREADS; ++i) {
    if (i == j) { tp = P; fp = N; }
    P += sp[i];
    N += sn[i];
  }
  double s_auc = 0.0, s_ap = 0.0, s_sl = 0.0;
  for (int i = 0; i < per; ++i) {
    const unsigned long long pb = pc[hi - i], nb = nc[hi - i];
    const unsigned long long tp1 = tp + pb, fp1 = fp + nb;
    s_auc += (double)nb * ((double)tp + (double)tp1);
    if (pb) s_ap += (double)pb * ((double)tp1 / ((double)tp1 + (double)fp1));
    s_sl += (double)pb * (double)nb;
    tp = tp1;
    fp = fp1;
  }
  red[0][j] = s_auc;
  red[1][j] = s_ap;
  red[2][j] = s_sl;
  __syncthreads();
  for (int w = CF_THREADS / 2; w > 0; w >>= 1) {
    if (j < w) {
      red[0][j] += red[0][j + w];
      red[1][j] += red[1][j + w];
      red[2][j] += red[2][j + w];
    }
    __syncthreads();
  }
  if (j == 0) {
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    const double pn = (double)P * (double)N;
    auc[c] = (P && N) ? red[0][0] / (2.0 * pn) : nan;
    ap[c] = P ? red[1][0] / (double)P : nan;
    slack[c] = (P && N) ? 0.5 * red[2][0] / pn : nan;
    support[2 * c] = P;
    support[2 * c + 1] = N;
  }
}

}  // namespace udaseg

using namespace udaseg;

extern "C" int udaseg_score_hist(const float* logits, const int64_t* target, int64_t pixels, int classes, int ldc, int bins,
                                 float score_range, int64_t* pos, int64_t* neg, void* stream) {
  UDASEG_CHECK_ARG(logits && target && pos && neg, "score_hist: NULL pointer");
  if (!scores_args_ok("score_hist", pixels, classes, ldc, 32)) return UDASEG_E_BADARG;
  UDASEG_CHECK_ARG(pixels < ((int64_t)1 << 31), "score_hist: need pixels < 2^31 (pixels=%lld)", (long long)pixels);
  UDASEG_CHECK_ARG(hist_bins_supported(bins), "score_hist: bins must be 256, 512, 1024, 2048 or 4096 (bins=%d)", bins);
  UDASEG_CHECK_ARG(score_range > 0.f && score_range <= 1e30f, "score_hist: score_range must be positive and finite");
  hipStream_t st = as_stream(stream);
  const int cg = SH_CELLS / (2 * bins);
  const int groups = (classes + cg - 1) / cg;
  int gx = SH_TOTAL_BLOCKS / groups;
  const int64_t want = (pixels + SH_THREADS - 1) / SH_THREADS;
  if (gx > want) gx = (int)want;
  if (gx < 1) gx = 1;
  const float scale = (float)bins / (2.f * score_range);
  if (!dispatch_width<8>(ldc / 4, [&](auto w) {
        hipLaunchKernelGGL(score_hist_kernel<decltype(w)::value>, dim3(gx, groups), dim3(SH_THREADS), 0, st, (const f32x4*)logits,
                           target, pixels, classes, bins, cg, score_range, scale, (unsigned long long*)pos,
                           (unsigned long long*)neg);
      }))
    return unsupported_width("score_hist", "ldc", ldc);
  UDASEG_LAUNCH_CHECK("score_hist launch");
  return UDASEG_OK;
}

extern "C" int udaseg_curve_finish(const int64_t* pos, const int64_t* neg, int classes, int bins, double* auc, double* ap,
                                   double* auc_slack, int64_t* support, void* stream) {
  UDASEG_CHECK_ARG(pos && neg && auc && ap && auc_slack && support, "curve_finish: NULL pointer");
  UDASEG_CHECK_ARG(classes > 0 && classes <= 32, "curve_finish: need 0 < classes <= 32 (classes=%d)", classes);
  UDASEG_CHECK_ARG(hist_bins_supported(bins), "curve_finish: bins must be 256, 512, 1024, 2048 or 4096 (bins=%d)", bins);
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(curve_finish_kernel, dim3(classes), dim3(CF_THREADS), 0, st, (const unsigned long long*)pos,
                     (const unsigned long long*)neg, bins, auc, ap, auc_slack, (unsigned long long*)support);
  UDASEG_LAUNCH_CHECK("curve_finish launch");
  return UDASEG_OK;
}
