// Class-balanced pseudo-labels of unlabelled target frames on the device (CBST, Zou et al. 2018; an extension: the reference's
// phase 3 is consistency only).  Done with torch this is softmax -> max -> one quantile (a sort) per class -> where, several
// passes over the scores; here ONE pass makes a per-class histogram of the winning class's confidence (udaseg_conf_hist), a
// tiny kernel turns the histogram into one threshold BIN per class (udaseg_pseudo_thresholds), and one more pass writes the
// uint8 masks with everything below its class's threshold marked void (udaseg_pseudo_labels).  No sort, integer counters only.
//
// The shared definition (pixel_conf of scores_common.h, used by BOTH pixel kernels and by udaseg_conf_share of distill.hip, so that
// histogram, labelling and share cannot disagree).
// scores: padded NHWC fp32 [pixels][ldc], ldc % 4 == 0, 0 < classes <= 32, classes <= ldc; only channels < classes count.
//   probs == 0 (logits z):     c^ = first maximum of z (first_max of scores_common.h), m = z[c^],
//                              S = sum_{c < classes} expf(z_c - m) in fp32 (four partial sums, channel c in sum c % 4,
//                              folded as (s0 + s1) + (s2 + s3): a third of the rounding of one chain), confidence p = 1 / S
//   probs == 1 (probabilities q, predict_large's accumulator view):   c^ = first maximum of q, p = q[c^]
//   bin(p) = min((int)floorf(p * B), B - 1), B in {256, 512, 1024, 2048, 4096}: the edges k / B are exact, p == 1 is in bin B - 1
//   a pixel whose p is not finite (a NaN logit, a +inf logit, all logits -inf) or, in probs mode, outside [0, 1] or beside a
//   NaN in any channel < classes is NON-FINITE: in no histogram cell, always void, counted on its own.
// A pixel predicted as c is kept iff bin(p) >= thr_bins[c], i.e. iff p >= thr_bins[c] / B.
//
// Routes of udaseg_conf_hist.  Each pixel touches ONE cell, so the block's whole [classes][bins] table of 32-bit counters sits
// in dynamic LDS whenever it fits CH_CELLS = 32768 cells (128 KiB of the CU's 160 KiB) and the scores are read once:
//   bins  256,  512, 1024: every class count (<= 32) in one group      -- 23 classes x 1024 bins = 92 KiB, ONE pass
//   bins 2048:             classes <= 16 one group, 17..32 two groups over blockIdx.y (each group re-reads the scores)
//   bins 4096:             classes <=  8 one group, then one more group per 8 classes (up to four)
// Blocks are few and long (CH_BLOCKS in all, 1024 threads each: a table beyond 80 KiB leaves one block per CU, and sixteen waves
// keep enough loads in flight for it), for the reason given in curves.hip: a block flushes one 64-bit global atomic per NON-EMPTY
// cell, so its pixel count has to be large against its cell count.  The LDS atomics are plain: a wave's 64 pixels are 6 KiB of
// scores, hundreds of clocks of a CU's share of the memory rate, against at most 64 clocks when every lane hits the same top
// bin; score_hist_kernel issues 23 such atomics per pixel and runs at the memory rate (profiles/curves_bench.txt).
// tools/bench_pseudo.py reports both pixel kernels against a device copy of the same bytes.
#include "scores_common.h"

namespace udaseg {

__device__ __forceinline__ int conf_bin(float p, int bins) { return min((int)floorf(p * (float)bins), bins - 1); }

constexpr int CH_CELLS = 32768;
constexpr int CH_THREADS = 1024;
constexpr int CH_BLOCKS = 256;
typedef BlockCounts<1, CH_THREADS / 64> ChBad;                // the non-finite pixels
constexpr int CH_LDS_MAX = CH_CELLS * 4 + (int)sizeof(ChBad::Slots);

// LDS: [tab] table cells of this block's class group, then the slots of the non-finite pixels' counter (group 0 reports it).
template <int NV>
__global__ __launch_bounds__(CH_THREADS) void conf_hist_kernel(const float* __restrict__ scores, int64_t pixels, int classes, int ldc,
                                                               int probs, int bins, int cg, int tab,
                                                               unsigned long long* __restrict__ hist,
                                                               unsigned long long* __restrict__ nonfinite) {
  extern __shared__ __attribute__((aligned(16))) unsigned int cells[];
  const int c0 = blockIdx.y * cg;
  const int nc = min(cg, classes - c0);
  const int ncell = nc * bins;                             // <= tab
  for (int i = threadIdx.x; i < ncell; i += CH_THREADS) cells[i] = 0;
  ChBad::Slots& bad_slots = *reinterpret_cast<ChBad::Slots*>(cells + tab);
  __syncthreads();
  unsigned int bad[1] = {0};
  const int64_t T = (int64_t)gridDim.x * CH_THREADS;
  for (int64_t p = (int64_t)blockIdx.x * CH_THREADS + threadIdx.x; p < pixels; p += T) {
    const PixelConf r = pixel_conf<NV>(scores + p * ldc, classes, probs);
    if (!r.finite) {
      ++bad[0];
      continue;
    }
    const int c = r.cls - c0;
    if (c >= 0 && c < nc) atomicAdd(&cells[c * bins + conf_bin(r.p, bins)], 1u);
  }
  if (blockIdx.y == 0) ChBad::put(bad_slots, bad);
  __syncthreads();                                         // closes the table and the slots
  for (int i = threadIdx.x; i < ncell; i += CH_THREADS) {
    const unsigned int v = cells[i];
    if (v) atomicAdd(&hist[(size_t)c0 * bins + i], (unsigned long long)v);
  }
  if (blockIdx.y == 0) ChBad::flush(bad_slots, nonfinite);
}

// One block per class.  Thread j owns the j-th chunk of bins / 256 bins from the top; the chunk sums are combined in thread
// order, so the result does not depend on timing.  need = (int64)ceil(portion * (double)n); the threshold bin is the largest k
// with sum_{b >= k} hist[b] >= need (bins - 1 for an empty class, 0 if no k qualifies), then clamped into [k_floor, k_cap].
constexpr int PT_THREADS = 256;

__global__ __launch_bounds__(PT_THREADS) void pseudo_thresholds_kernel(const unsigned long long* __restrict__ hist, int bins,
                                                                       const double* __restrict__ portion, int k_floor, int k_cap,
                                                                       int* __restrict__ thr_bins,
                                                                       unsigned long long* __restrict__ support) {
  __shared__ unsigned long long chunk[PT_THREADS];
  __shared__ int found;
  const int c = blockIdx.x, j = threadIdx.x;
  const int per = bins / PT_THREADS;
  const unsigned long long* row = hist + (size_t)c * bins;
  const int hi = bins - 1 - j * per;                       // this thread's bins: hi, hi - 1, ..., hi - per + 1
  unsigned long long s = 0;
  for (int i = 0; i < per; ++i) s += row[hi - i];
  chunk[j] = s;
  __syncthreads();
  unsigned long long above = 0, n = 0;                     // above: the pixels in the bins above this thread's chunk
  for (int i = 0; i < PT_THREADS; ++i) {
    if (i == j) above = n;
    n += chunk[i];
  }
  const long long need = (long long)ceil(portion[c] * (double)n);
  if (j == 0) found = need <= 0 ? bins - 1 : 0;
  __syncthreads();
  if ((long long)above < need) {                           // at most one thread crosses `need` inside its chunk
    unsigned long long run = above;
    for (int i = 0; i < per; ++i) {
      run += row[hi - i];
      if ((long long)run >= need) {
        found = hi - i;
        break;
      }
    }
  }
  __syncthreads();
  if (j == 0) {
    thr_bins[c] = min(max(found, k_floor), k_cap);
    support[c] = n;
  }
}

// A wave takes 256 consecutive pixels at a time, lane l the pixels 64 j + l (j = 0..3): consecutive lanes read consecutive rows.
// The four labels of a lane are packed into one word and exchanged so that lane l holds the pixels 4 l .. 4 l + 3 and writes them
// with ONE 32-bit store (256 contiguous bytes per wave); a chunk cut short by the end of the buffer, or labels that are not
// 4-byte aligned, take the byte stores.  conf is written as it is computed: one float per lane, contiguous over the wave.
// counts: kept per class through LDS counters, void / non-finite in registers, one global atomic per non-zero counter per block.
constexpr int PL_THREADS = 256;
constexpr int PL_MAX_BLOCKS = 2048;

template <int NV>
__global__ __launch_bounds__(PL_THREADS) void pseudo_labels_kernel(const float* __restrict__ scores, int64_t pixels, int classes,
                                                                   int ldc, int probs, int bins, const int* __restrict__ thr_bins,
                                                                   int void_label, uint8_t* __restrict__ labels,
                                                                   float* __restrict__ conf, unsigned long long* __restrict__ counts,
                                                                   int vec_ok) {
  __shared__ unsigned int cnt[34];
  __shared__ int thr[32];
  if (threadIdx.x < 34) cnt[threadIdx.x] = 0;
  if (threadIdx.x < classes) thr[threadIdx.x] = thr_bins[threadIdx.x];
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  constexpr int WAVES = PL_THREADS / 64;
  unsigned int nvoid = 0, nbad = 0;
  const int64_t chunks = (pixels + 255) >> 8;
  for (int64_t ch = (int64_t)blockIdx.x * WAVES + wave; ch < chunks; ch += (int64_t)gridDim.x * WAVES) {
    const int64_t base = ch << 8;
    unsigned int packed = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t p = base + 64 * j + lane;
      int lab = void_label;
      if (p < pixels) {
        const PixelConf r = pixel_conf<NV>(scores + p * ldc, classes, probs);
        float cf = 0.f;
        if (r.finite) {
          cf = r.p;
          if (conf_bin(r.p, bins) >= thr[r.cls]) {
            lab = r.cls;
            atomicAdd(&cnt[lab], 1u);
          } else {
            ++nvoid;
          }
        } else {
          ++nvoid;
          ++nbad;
        }
        if (conf) conf[p] = cf;
      }
      packed |= (unsigned int)lab << (8 * j);
    }
    if (vec_ok && base + 256 <= pixels) {                  // uniform over the wave
      unsigned int out = 0;
#pragma unroll
      for (int e = 0; e < 4; ++e) {                        // pixel 4 l + e: lane (4 l + e) & 63 holds it in byte l >> 4
        const unsigned int w = (unsigned int)__shfl((int)packed, (4 * lane + e) & 63, 64);
        out |= ((w >> (8 * (lane >> 4))) & 0xffu) << (8 * e);
      }
      reinterpret_cast<unsigned int*>(labels + base)[lane] = out;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t p = base + 64 * j + lane;
        if (p < pixels) labels[p] = (uint8_t)((packed >> (8 * j)) & 0xffu);
      }
    }
  }
  // Written out, not BlockCounts (common.h): with the pair in slots of its own beside a 32-word class table the labelling of
  // 8 x 512 x 512 pixels took 0.085 ms for 0.065 ms (profiles/block_counts_refactor.txt); the pair shares the table's zeroing and flush.
  nvoid = wave_sum_u32(nvoid);
  nbad = wave_sum_u32(nbad);
  if (lane == 0) {
    if (nvoid) atomicAdd(&cnt[32], nvoid);
    if (nbad) atomicAdd(&cnt[33], nbad);
  }
  __syncthreads();
  if (threadIdx.x < classes) {
    if (cnt[threadIdx.x]) atomicAdd(&counts[threadIdx.x], (unsigned long long)cnt[threadIdx.x]);
  } else if (threadIdx.x < classes + 2) {
    const unsigned int v = cnt[32 + threadIdx.x - classes];
    if (v) atomicAdd(&counts[threadIdx.x], (unsigned long long)v);
  }
}

static bool pseudo_args_ok(const char* who, const void* scores, int64_t pixels, int classes, int ldc, int probs, int bins) {
  if (!scores_args_ok(who, pixels, classes, ldc)) return false;
  if (pixels >= ((int64_t)1 << 31)) {
    set_error("%s: need pixels < 2^31 (pixels=%lld)", who, (long long)pixels);
    return false;
  }
  if (!hist_bins_supported(bins)) {
    set_error("%s: bins must be 256, 512, 1024, 2048 or 4096 (bins=%d)", who, bins);
    return false;
  }
  if (probs != 0 && probs != 1) {
    set_error("%s: probs must be 0 (logits) or 1 (probabilities), got %d", who, probs);
    return false;
  }
  if (reinterpret_cast<uintptr_t>(scores) & 15) {
    set_error("%s: scores must be 16-byte aligned", who);
    return false;
  }
  return true;
}

}  // namespace udaseg

using namespace udaseg;

extern "C" int udaseg_conf_hist(const float* scores, int64_t pixels, int classes, int ldc, int probs, int bins, int64_t* hist,
                                int64_t* nonfinite, void* stream) {
  UDASEG_CHECK_ARG(scores && hist && nonfinite, "conf_hist: NULL pointer");
  if (!pseudo_args_ok("conf_hist", scores, pixels, classes, ldc, probs, bins)) return UDASEG_E_BADARG;
  hipStream_t st = as_stream(stream);
  const int nv = cdiv(classes, 4);
  const int cg = min(classes, CH_CELLS / bins);            // classes per group
  const int groups = cdiv(classes, cg);
  const int tab = cg * bins;
  const size_t lds = (size_t)tab * 4 + sizeof(ChBad::Slots);
  static std::atomic<bool> attr_done[9];
  if (lds > 48 * 1024 && !attr_done[nv]) {
    hipError_t e = hipSuccess;
    dispatch_width<8>(nv, [&](auto w) {
      e = hipFuncSetAttribute(reinterpret_cast<const void*>(conf_hist_kernel<decltype(w)::value>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, CH_LDS_MAX);
    });
    if (e != hipSuccess) return hip_fail(e, "hipFuncSetAttribute(conf_hist)");
    attr_done[nv] = true;
  }
  int gx = CH_BLOCKS / groups;
  const int64_t want = cdiv64(pixels, CH_THREADS);
  if (gx > want) gx = (int)want;
  if (gx < 1) gx = 1;
  if (!dispatch_width<8>(nv, [&](auto w) {
        hipLaunchKernelGGL(conf_hist_kernel<decltype(w)::value>, dim3(gx, groups), dim3(CH_THREADS), lds, st, scores, pixels, classes,
                           ldc, probs, bins, cg, tab, (unsigned long long*)hist, (unsigned long long*)nonfinite);
      }))
    return unsupported_width("conf_hist", "classes", classes);
  UDASEG_LAUNCH_CHECK("conf_hist launch");
  return UDASEG_OK;
}

extern "C" int udaseg_pseudo_thresholds(const int64_t* hist, int classes, int bins, const double* portion, int k_floor, int k_cap,
                                        int32_t* thr_bins, int64_t* support, void* stream) {
  UDASEG_CHECK_ARG(hist && portion && thr_bins && support, "pseudo_thresholds: NULL pointer");
  UDASEG_CHECK_ARG(classes > 0 && classes <= 32, "pseudo_thresholds: need 0 < classes <= 32 (classes=%d)", classes);
  UDASEG_CHECK_ARG(hist_bins_supported(bins), "pseudo_thresholds: bins must be 256, 512, 1024, 2048 or 4096 (bins=%d)", bins);
  UDASEG_CHECK_ARG(0 <= k_floor && k_floor <= k_cap && k_cap <= bins - 1,
                   "pseudo_thresholds: need 0 <= k_floor <= k_cap <= bins - 1 (k_floor=%d k_cap=%d bins=%d)", k_floor, k_cap, bins);
  hipLaunchKernelGGL(pseudo_thresholds_kernel, dim3(classes), dim3(PT_THREADS), 0, as_stream(stream), (const unsigned long long*)hist,
                     bins, portion, k_floor, k_cap, thr_bins, (unsigned long long*)support);
  UDASEG_LAUNCH_CHECK("pseudo_thresholds launch");
  return UDASEG_OK;
}

extern "C" int udaseg_pseudo_labels(const float* scores, int64_t pixels, int classes, int ldc, int probs, int bins,
                                    const int32_t* thr_bins, int void_label, uint8_t* labels, float* conf, int64_t* counts,
                                    void* stream) {
  UDASEG_CHECK_ARG(scores && thr_bins && labels && counts, "pseudo_labels: NULL pointer");
  if (!pseudo_args_ok("pseudo_labels", scores, pixels, classes, ldc, probs, bins)) return UDASEG_E_BADARG;
  UDASEG_CHECK_ARG(void_label >= classes && void_label <= 255,
                   "pseudo_labels: need classes <= void_label <= 255 (void_label=%d classes=%d)", void_label, classes);
  const int gx = capped_grid(cdiv64(pixels, 256), PL_THREADS / 64, PL_MAX_BLOCKS);
  const int vec_ok = (reinterpret_cast<uintptr_t>(labels) & 3) == 0;
  if (!dispatch_width<8>(cdiv(classes, 4), [&](auto w) {
        hipLaunchKernelGGL(pseudo_labels_kernel<decltype(w)::value>, dim3(gx), dim3(PL_THREADS), 0, as_stream(stream), scores, pixels,
                           classes, ldc, probs, bins, thr_bins, void_label, labels, conf, (unsigned long long*)counts, vec_ok);
      }))
    return unsupported_width("pseudo_labels", "classes", classes);
  UDASEG_LAUNCH_CHECK("pseudo_labels launch");
  return UDASEG_OK;
}
