// Hard-pixel mining for the per-pixel cross entropy (online hard example mining, Shrivastava et al. 2016, in its per-pixel form;
// bootstrapped / top-k cross entropy, Wu et al. 2016), exact on the device: no sort, no host read, the same bits on every run.
//
// THE definition (include/udaseg.h restates it for callers, tests/_ohem_ref.py in numpy).
//   logits: padded NHWC fp32 [pixels][ldc], ldc % 4 == 0, classes <= ldc <= 32, 0 < pixels < 2^31; target int64; weight optional.
//   valid(p):      ce_valid of loss_reduce.h (target != ignore_index when has_ignore, 0 <= target < classes).
//   non-finite(p): valid, but some z_c, c < classes, is not finite: void, counted on its own, loss and gradient exactly 0.
//   confidence:    m = the first maximum of the row (first_max), S = exp_sum (scores_common.h: pixel_conf's sum and order),
//                  p = expf(z_t - m) / S.  The maximum's term is exactly 1, so 0 <= p <= 1 and the fp32 bits of p are an
//                  order-preserving unsigned integer < 2^30.  conf[pixel] = p; -1.0f at void, invalid and non-finite pixels.
//   selection:     n = number of valid finite pixels; k = min_kept, or ceil(fraction * n) in float64 when fraction >= 0;
//                  q = the k-th smallest p (1-indexed), -inf when k == 0, +inf when k > n (there is no k-th: everything is below it).
//                  kept(p) iff conf >= 0 and (p < thresh or p <= q).  Ties at q are ALL kept: the kept set is a function of the
//                  values alone, not of the pixel order or the launch shape, and at least min(k, n) pixels are kept.
//   loss:          l = w[t] * (lse - z_t) over the kept pixels (ce_row_lse of loss_reduce.h, as the optioned cross entropy);
//                  'mean' divides by D = the fixed-order f64 sum of w[t] over the kept pixels (D == 0: NaN loss, zero gradient).
//   gradient:      (1 / D or 1) * w[t] * (P_c - [c == t]) at a kept pixel, exactly 0 in all ldc lanes of every other pixel.
//
// The k-th smallest is a three-level radix select over the 30 value bits, 10 bits a level (bits 29..20, 19..10, 9..0):
//   udaseg_ohem_conf     one pass over the logits: conf, the level-0 histogram, the void / invalid / non-finite counters
//   udaseg_kth_select 0  n = the histogram's total, k, the bin that holds rank k -> state
//   udaseg_kth_hist 1    one pass over conf (4 B/pixel): histogram of bits 19..10 of the values whose bits 29..20 equal the prefix
//   udaseg_kth_select 1, udaseg_kth_hist 2, udaseg_kth_select 2: state holds all 30 bits of q
//   udaseg_ohem_denom    one pass over conf / target: D, the kept count, the optional keep map
//   udaseg_ce_ohem_fwd_bwd  ce_opt_fwd_bwd_kernel with the keep predicate read from conf and state -- the values the selection
//                        itself used, so mask and selection cannot disagree
// udaseg_kth_hist (levels 0..2) and udaseg_kth_select are the general primitive "k-th smallest of a device buffer of floats in
// [0, 2)" (kernels.kth_smallest); a value whose sign bit is set or that is >= 2 (bits >= 2^30: -1.0f, inf, NaN) is skipped.
//
// Histograms.  A block keeps the 1024 bins as 32-bit LDS counters and flushes its non-empty bins with one 64-bit global atomic
// each.  Easy pixels have p in [0.5, 1]: NINE level-0 bins, so a wave's 64 LDS atomics would pile onto a handful of addresses
// (the serialisation profiles/proto_bench.txt shows for class sums).  wave_hist_add aggregates first: the wave peels one distinct
// bin per round (ballot of the lanes that share the leader's bin) and ONE lane adds the group's size -- as many LDS atomics as
// the wave has distinct bins, one for a smooth field.  All atomics are on integers and every float sum has a fixed order.
#include "launch.h"
#include "loss_reduce.h"

namespace udaseg {

// The pixel kernels launch at most udaseg_ce_partials() blocks (losses.hip's CE_BLOCKS: what the callers' `partials` are sized by).
constexpr int KTH_BINS = 1024;
constexpr int KTH_HIST_BLOCKS = 256;     // x 256 threads x 4 values = the same 262144 items a trip as the pixel kernels
constexpr unsigned KTH_VALUE_LIMIT = 1u << 30;

// state: int64 [UDASEG_KTH_STATE] (include/udaseg.h documents it for callers)
enum { ST_PREFIX = 0, ST_RANK = 1, ST_N = 2, ST_K = 3, ST_FLAGS = 4, ST_LEVELS = 5 };

// q of the definition from a finished state
__device__ __forceinline__ float kth_q(const int64_t* __restrict__ state) {
  const int64_t n = state[ST_N], k = state[ST_K];
  if (k <= 0) return -INFINITY;
  if (k > n) return INFINITY;
  return __builtin_bit_cast(float, (unsigned)state[ST_PREFIX]);
}
// THE keep predicate (udaseg_ohem_denom, udaseg_ce_ohem_fwd_bwd)
__device__ __forceinline__ bool ohem_keep(float c, float thresh, float q) { return c >= 0.f && (c < thresh || c <= q); }

// cells[bin] += 1 for every lane with ok, with one LDS atomic per DISTINCT bin of the wave.  Reached by all 64 lanes of the wave
// (the callers' loops have wave-uniform trip counts); at most 64 rounds, each retiring at least its leader.
__device__ __forceinline__ void wave_hist_add(unsigned int* cells, bool ok, int bin) {
  const int lane = threadIdx.x & 63;
  unsigned long long todo = __ballot(ok);
  while (todo) {
    const int lead = __ffsll((long long)todo) - 1;
    const int lead_bin = __shfl(bin, lead, 64);
    const unsigned long long same = __ballot(ok && bin == lead_bin) & todo;
    if (lane == lead) atomicAdd(&cells[lead_bin], (unsigned int)__popcll(same));
    todo &= ~same;
  }
}
// the block's non-empty bins into the global histogram
__device__ __forceinline__ void flush_cells(const unsigned int* cells, unsigned long long* __restrict__ hist) {
  for (int i = threadIdx.x; i < KTH_BINS; i += blockDim.x) {
    const unsigned int v = cells[i];
    if (v) atomicAdd(&hist[i], (unsigned long long)v);
  }
}

// One thread per pixel of a 256-pixel chunk (consecutive lanes on consecutive rows).  counters: void, invalid, non-finite.
template <int NV>
__global__ __launch_bounds__(256) void ohem_conf_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                                                        int64_t pixels, int classes, int ldc, int has_ignore, int64_t ignore_index,
                                                        float* __restrict__ conf, unsigned long long* __restrict__ hist0,
                                                        unsigned long long* __restrict__ counters) {
  __shared__ unsigned int cells[KTH_BINS];
  __shared__ BlockCounts<3>::Slots cnt;                    // 256 threads: four waves
  const int tid = threadIdx.x;
  for (int i = tid; i < KTH_BINS; i += 256) cells[i] = 0;
  __syncthreads();
  unsigned int ev[3] = {0, 0, 0};                          // void, invalid, non-finite
  const int64_t nchunks = (pixels + 255) / 256;
  for (int64_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
    const int64_t p = chunk * 256 + tid;
    bool ok = false;
    float c = -1.f;
    if (p < pixels) {
      const int64_t t64 = target[p];
      if (has_ignore && t64 == ignore_index) {
        ++ev[0];
      } else if ((uint64_t)t64 >= (uint64_t)classes) {
        ++ev[1];
      } else {
        const int t = (int)t64;
        f32x4 v[NV];
        load_row<NV>(logits + p * ldc, v);
        bool finite = true;
        float zt = 0.f;
#pragma unroll
        for (int q = 0; q < NV; ++q)
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (4 * q + e < classes) {
              finite &= __builtin_isfinite(v[q][e]);
              if (4 * q + e == t) zt = v[q][e];
            }
        if (finite) {
          float m;
          first_max<NV>(v, classes, m);
          c = expf(zt - m) / exp_sum<NV>(v, classes, m);
          ok = true;
        } else {
          ++ev[2];
        }
      }
      conf[p] = c;
    }
    wave_hist_add(cells, ok, (int)(__builtin_bit_cast(unsigned, c) >> 20) & (KTH_BINS - 1));
  }
  BlockCounts<3>::put(cnt, ev);
  __syncthreads();                                         // closes the cells and the slots
  flush_cells(cells, hist0);
  BlockCounts<3>::flush(cnt, counters);
}

// Thread i of a trip holds the four consecutive values 4 i .. 4 i + 3 (VEC: one 16-byte load; values 16-byte aligned).
// level 0 counts every value in [0, 2); levels 1 and 2 the values whose bits above the level's field equal state's prefix.
template <bool VEC>
__global__ __launch_bounds__(256) void kth_hist_kernel(const float* __restrict__ values, int64_t count, int level,
                                                       const int64_t* __restrict__ state, unsigned long long* __restrict__ hist) {
  __shared__ unsigned int cells[KTH_BINS];
  if (level > 0 && state[ST_RANK] <= 0) return;          // k == 0 or nothing to select from: uniform over the whole grid
  const int tid = threadIdx.x;
  for (int i = tid; i < KTH_BINS; i += 256) cells[i] = 0;
  __syncthreads();
  const int shift = 20 - 10 * level;
  const unsigned himask = level == 0 ? 0u : (KTH_VALUE_LIMIT - 1) & ~((1u << (shift + 10)) - 1);
  const unsigned prefix = level == 0 ? 0u : (unsigned)state[ST_PREFIX] & himask;
  const int64_t ntrips = (count + 1023) / 1024;
  for (int64_t trip = blockIdx.x; trip < ntrips; trip += gridDim.x) {
    const int64_t i0 = (trip * 256 + tid) * 4;
    unsigned b[4] = {KTH_VALUE_LIMIT, KTH_VALUE_LIMIT, KTH_VALUE_LIMIT, KTH_VALUE_LIMIT};   // "skipped"
    if (VEC && i0 + 4 <= count) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(values + i0);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float x = v[e];          // a scalar copy: a bit cast of the vector element itself read element 0 four times
        b[e] = __float_as_uint(x);
      }
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (i0 + e < count) b[e] = __float_as_uint(values[i0 + e]);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
      wave_hist_add(cells, b[e] < KTH_VALUE_LIMIT && (b[e] & himask) == prefix, (int)(b[e] >> shift) & (KTH_BINS - 1));
  }
  __syncthreads();
  flush_cells(cells, hist);
}

// ONE block.  Thread j owns bins 4 j .. 4 j + 3; the chunk sums are combined in thread order (bounded loops, nothing waits on
// memory another thread writes).  The bin that holds rank r: the b with  sum_{i < b} hist[i] < r <= sum_{i <= b} hist[i].
__global__ __launch_bounds__(256) void kth_select_kernel(const unsigned long long* __restrict__ hist, int level, int64_t min_kept,
                                                         double fraction, int64_t* __restrict__ state) {
  __shared__ unsigned long long chunk[256];
  const int j = threadIdx.x;
  unsigned long long own[4], s = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    own[i] = hist[4 * j + i];
    s += own[i];
  }
  chunk[j] = s;
  int64_t r = level == 0 ? 0 : state[ST_RANK];           // read before the barrier, written after it
  const unsigned prefix = level == 0 ? 0u : (unsigned)state[ST_PREFIX];
  __syncthreads();
  unsigned long long below = 0, total = 0;
  for (int i = 0; i < 256; ++i) {
    if (i == j) below = total;
    total += chunk[i];
  }
  if (level == 0) {
    const int64_t n = (int64_t)total;
    const int64_t k = fraction < 0.0 ? min_kept : (int64_t)ceil(fraction * (double)n);
    r = k < n ? k : n;
    if (j == 0) {
      state[ST_N] = n;
      state[ST_K] = k;
      state[ST_FLAGS] = (k <= 0 ? 1 : 0) | (k >= n ? 2 : 0);
      if (r <= 0) {
        state[ST_PREFIX] = 0;
        state[ST_RANK] = 0;
      }
    }
  }
  if (j == 0) state[ST_LEVELS] = level + 1;
  if (r >= 1 && below < (unsigned long long)r && (unsigned long long)r <= below + s) {   // exactly one thread
    unsigned long long run = below;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (run + own[i] >= (unsigned long long)r) {
        state[ST_PREFIX] = (int64_t)(prefix | ((unsigned)(4 * j + i) << (20 - 10 * level)));
        state[ST_RANK] = (int64_t)((unsigned long long)r - run);
        break;
      }
      run += own[i];
    }
  }
}

// out[0] = q, out[1] = max(q, thresh): the confidence below which (or at which, where q rules) a pixel is kept
__global__ void kth_value_kernel(const int64_t* __restrict__ state, float thresh, float* __restrict__ out) {
  if (threadIdx.x == 0) {
    const float q = kth_q(state);
    out[0] = q;
    out[1] = fmaxf(q, thresh);
  }
}

// partials[k][block], k = 0: sum of w[t] over the kept pixels (f64), 1: valid finite pixels (conf >= 0), 2: kept pixels.
// ce_target_stats_kernel's pixel-to-thread map and reductions.
__global__ __launch_bounds__(256) void ohem_denom_kernel(const float* __restrict__ conf, const int64_t* __restrict__ target,
                                                         const float* __restrict__ weight, int64_t pixels, int classes, float thresh,
                                                         const int64_t* __restrict__ state, double* __restrict__ partials,
                                                         uint8_t* __restrict__ keep) {
  __shared__ float wsh[32];
  __shared__ double red[3][4];
  if (threadIdx.x < 32) wsh[threadIdx.x] = (int)threadIdx.x < classes ? (weight ? weight[threadIdx.x] : 1.f) : 0.f;
  __syncthreads();
  const float q = kth_q(state);
  const int64_t T = (int64_t)gridDim.x * blockDim.x;
  double d = 0.0;
  int nfinite = 0, nkept = 0;
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < pixels; p += T) {
    const float c = conf[p];
    const bool kept = ohem_keep(c, thresh, q);
    nfinite += c >= 0.f;
    if (kept) {
      ++nkept;
      d += (double)wsh[(int)target[p] & 31];               // conf >= 0 only where the target names a class
    }
    if (keep) keep[p] = kept;
  }
  double v[3] = {d, (double)nfinite, (double)nkept};
  block_partial_rows<3>(v, red, partials);
}

// ce_opt_fwd_bwd_kernel (losses.hip) without label smoothing and with the keep predicate; GRAD == false: the loss alone.
template <int LDC4, bool GRAD>
__global__ __launch_bounds__(256) void ce_ohem_fwd_bwd_kernel(const f32x4* __restrict__ logits, const int64_t* __restrict__ target,
                                                              const float* __restrict__ weight, const float* __restrict__ conf,
                                                              const int64_t* __restrict__ state, float thresh, int64_t pixels,
                                                              int classes, const double* __restrict__ denom,
                                                              double* __restrict__ partials, f32x4* __restrict__ dlogits,
                                                              float* __restrict__ colpart) {
  using Tile = GradTile<LDC4>;
  __shared__ __attribute__((aligned(16))) float tile[GRAD ? 256 * Tile::LDC : 4];
  __shared__ float colred[GRAD ? Tile::NG * Tile::LDC : 1];
  __shared__ double red[4];
  __shared__ float wsh[32];
  const int tid = threadIdx.x;
  if (tid < 32) wsh[tid] = tid < classes ? (weight ? weight[tid] : 1.f) : 0.f;
  __syncthreads();
  const float q = kth_q(state);
  const float scale = denom ? (float)(1.0 / *denom) : 1.f;
  const int64_t nchunks = (pixels + 255) / 256;
  float colacc = 0.f;
  double local = 0.0;
  for (int64_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
    const int64_t p = chunk * 256 + tid;
    const bool kept = p < pixels && ohem_keep(conf[p], thresh, q);
    if (kept) {
      const int t = (int)target[p] & 31;                   // conf >= 0 only where the target names a class
      f32x4 v[LDC4];
#pragma unroll
      for (int k = 0; k < LDC4; ++k) v[k] = logits[p * LDC4 + k];
      float xt;
      const float l = ce_row_lse<LDC4>(v, classes, t, xt);
      const float wt = wsh[t];
      local += (double)(wt * (l - xt));
      if (GRAD) {
        const float a = scale * wt;
#pragma unroll
        for (int k = 0; k < LDC4; ++k) {
          f32x4 g;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int c = k * 4 + e;
            g[e] = c < classes ? expf(v[k][e] - l) * a - (c == t ? a : 0.f) : 0.f;
          }
          Tile::put(*reinterpret_cast<typename Tile::Rows*>(tile), k, g);
        }
      }
    } else if (GRAD) {
      Tile::put_zero(*reinterpret_cast<typename Tile::Rows*>(tile));
    }
    if (GRAD) Tile::flush(*reinterpret_cast<typename Tile::Rows*>(tile), chunk, pixels, dlogits, colpart != nullptr, colacc);
  }
  if (GRAD && colpart) Tile::put_columns(*reinterpret_cast<typename Tile::Cols*>(colred), colacc);
  block_partial(local, red, partials);   // its barrier is the column sums' too
  if (GRAD && colpart) Tile::write_columns(*reinterpret_cast<typename Tile::Cols*>(colred), colpart);
}

static bool kth_level_ok(const char* who, int level) {
  if (level >= 0 && level <= 2) return true;
  set_error("%s: level must be 0, 1 or 2 (level=%d)", who, level);
  return false;
}
static bool ohem_pixels_ok(const char* who, int64_t pixels) {
  if (pixels > 0 && pixels < ((int64_t)1 << 31)) return true;
  set_error("%s: need 0 < pixels < 2^31 (pixels=%lld)", who, (long long)pixels);
  return false;
}

}  // namespace udaseg

using namespace udaseg;

extern "C" int udaseg_ohem_conf(const float* logits, const int64_t* target, int64_t pixels, int classes, int ldc, int has_ignore,
                                int64_t ignore_index, float* conf, int64_t* hist0, int64_t* counters, void* stream) {
  UDASEG_CHECK_ARG(logits && target && conf && hist0 && counters, "ohem_conf: NULL pointer");
  if (!scores_args_ok("ohem_conf", pixels, classes, ldc, 32) || !ohem_pixels_ok("ohem_conf", pixels)) return UDASEG_E_BADARG;
  hipStream_t st = as_stream(stream);
  const int grid = capped_grid(pixels, 256, udaseg_ce_partials());
  static KernelRec rec(nullptr, "ohem_conf_kernel");
  KTimer kt(rec, st, (double)pixels * (4.0 * ldc + 12.0));
  if (!dispatch_width<8>((classes + 3) / 4, [&](auto w) {
        hipLaunchKernelGGL((ohem_conf_kernel<decltype(w)::value>), dim3(grid), dim3(256), 0, st, logits, target, pixels, classes, ldc,
                           has_ignore, ignore_index, conf, (unsigned long long*)hist0, (unsigned long long*)counters);
      }))
    return unsupported_width("ohem_conf", "classes", classes);
  UDASEG_LAUNCH_CHECK("ohem_conf launch");
  return UDASEG_OK;
}

extern "C" int udaseg_kth_hist(const float* values, int64_t count, int level, const int64_t* state, int64_t* hist, void* stream) {
  UDASEG_CHECK_ARG(values && hist, "kth_hist: NULL pointer");
  UDASEG_CHECK_ARG(count > 0, "kth_hist: need count > 0 (count=%lld)", (long long)count);
  if (!kth_level_ok("kth_hist", level)) return UDASEG_E_BADARG;
  UDASEG_CHECK_ARG(level == 0 || state, "kth_hist: levels 1 and 2 need the state of the level before (NULL state)");
  hipStream_t st = as_stream(stream);
  const int grid = capped_grid(count, 1024, KTH_HIST_BLOCKS);
  static KernelRec rec(nullptr, "kth_hist_kernel");
  KTimer kt(rec, st, (double)count * 4.0);
  if (((uintptr_t)values & 15) == 0)
    hipLaunchKernelGGL(kth_hist_kernel<true>, dim3(grid), dim3(256), 0, st, values, count, level, state, (unsigned long long*)hist);
  else
    hipLaunchKernelGGL(kth_hist_kernel<false>, dim3(grid), dim3(256), 0, st, values, count, level, state, (unsigned long long*)hist);
  UDASEG_LAUNCH_CHECK("kth_hist launch");
  return UDASEG_OK;
}

extern "C" int udaseg_kth_select(const int64_t* hist, int level, int64_t min_kept, double fraction, int64_t* state, void* stream) {
  UDASEG_CHECK_ARG(hist, "kth_select: NULL pointer");
  UDASEG_CHECK_ARG(state, "kth_select: NULL state");
  if (!kth_level_ok("kth_select", level)) return UDASEG_E_BADARG;
  UDASEG_CHECK_ARG(level != 0 || (fraction < 0.0 ? min_kept >= 0 : fraction <= 1.0),
                   "kth_select: need min_kept >= 0, or 0 <= fraction <= 1 (min_kept=%lld fraction=%g)", (long long)min_kept, fraction);
  hipLaunchKernelGGL(kth_select_kernel, dim3(1), dim3(256), 0, as_stream(stream), (const unsigned long long*)hist, level, min_kept,
                     fraction, state);
  UDASEG_LAUNCH_CHECK("kth_select launch");
  return UDASEG_OK;
}

extern "C" int udaseg_kth_value(const int64_t* state, float thresh, float* out, void* stream) {
  UDASEG_CHECK_ARG(state && out, "kth_value: NULL pointer");
  hipLaunchKernelGGL(kth_value_kernel, dim3(1), dim3(64), 0, as_stream(stream), state, thresh, out);
  UDASEG_LAUNCH_CHECK("kth_value launch");
  return UDASEG_OK;
}

static int check_ohem_thresh(const char* who, float thresh) {
  UDASEG_CHECK_ARG(thresh >= 0.f && thresh <= 1.f, "%s: thresh must lie in [0, 1], got %g", who, (double)thresh);
  return UDASEG_OK;
}

extern "C" int udaseg_ohem_denom(const float* conf, const int64_t* target, const float* weight, int64_t pixels, int classes,
                                 float thresh, const int64_t* state, double* partials, double* denom, int64_t* counts,
                                 uint8_t* keep, void* stream) {
  UDASEG_CHECK_ARG(conf && target && partials && denom && counts, "ohem_denom: NULL pointer");
  UDASEG_CHECK_ARG(state, "ohem_denom: NULL state");
  UDASEG_CHECK_ARG(classes > 0 && classes <= 32, "ohem_denom: need 0 < classes <= 32 (classes=%d)", classes);
  if (!ohem_pixels_ok("ohem_denom", pixels)) return UDASEG_E_BADARG;
  int rc = check_ohem_thresh("ohem_denom", thresh);
  if (rc) return rc;
  hipStream_t st = as_stream(stream);
  const int grid = capped_grid(pixels, 256, udaseg_ce_partials());
  {
    static KernelRec rec(nullptr, "ohem_denom_kernel");
    KTimer kt(rec, st, (double)pixels * (keep ? 5.0 : 4.0));
    hipLaunchKernelGGL(ohem_denom_kernel, dim3(grid), dim3(256), 0, st, conf, target, weight, pixels, classes, thresh, state, partials,
                       keep);
    UDASEG_LAUNCH_CHECK("ohem_denom launch");
  }
  return launch_rows_finish(3, partials, grid, denom, counts, st, "ohem_denom_finish launch");
}

extern "C" int udaseg_ce_ohem_fwd_bwd(const float* logits, const int64_t* target, const float* weight, const float* conf,
                                      const int64_t* state, float thresh, int64_t pixels, int classes, int ldc, int mean,
                                      const double* denom, double* partials, float* loss, float* dlogits, float* colsum_partials,
                                      float* colsum, void* stream) {
  UDASEG_CHECK_ARG(logits && target && conf && partials && loss, "ce_ohem_fwd_bwd: NULL pointer");
  UDASEG_CHECK_ARG(state, "ce_ohem_fwd_bwd: NULL state");
  if (!scores_args_ok("ce_ohem_fwd_bwd", pixels, classes, ldc, 32) || !ohem_pixels_ok("ce_ohem_fwd_bwd", pixels))
    return UDASEG_E_BADARG;
  int rc = check_ohem_thresh("ce_ohem_fwd_bwd", thresh);
  if (rc) return rc;
  UDASEG_CHECK_ARG(!mean || denom, "ce_ohem_fwd_bwd: the 'mean' reduction needs the denominator of udaseg_ohem_denom");
  UDASEG_CHECK_ARG((colsum == nullptr) == (colsum_partials == nullptr), "ce_ohem_fwd_bwd: colsum and colsum_partials come together");
  UDASEG_CHECK_ARG(dlogits || !colsum, "ce_ohem_fwd_bwd: column sums need dlogits");
  hipStream_t st = as_stream(stream);
  const int grid = capped_grid(pixels, 256, udaseg_ce_partials());
  const double* dn = mean ? denom : nullptr;
  {
    static KernelRec rec(nullptr, "ce_ohem_fwd_bwd_kernel");
    KTimer kt(rec, st, (double)pixels * (4.0 * ldc * (dlogits ? 2.0 : 1.0) + 4.0));
    if (!dispatch_width<8>(ldc / 4, [&](auto w) {
          constexpr int W = decltype(w)::value;
          if (dlogits)
            hipLaunchKernelGGL((ce_ohem_fwd_bwd_kernel<W, true>), dim3(grid), dim3(256), 0, st, (const f32x4*)logits, target, weight, conf,
                               state, thresh, pixels, classes, dn, partials, (f32x4*)dlogits, colsum_partials);
          else
            hipLaunchKernelGGL((ce_ohem_fwd_bwd_kernel<W, false>), dim3(grid), dim3(256), 0, st, (const f32x4*)logits, target, weight,
                               conf, state, thresh, pixels, classes, dn, partials, (f32x4*)nullptr, (float*)nullptr);
        }))
      return unsupported_width("ce_ohem_fwd_bwd", "ldc", ldc);
    UDASEG_LAUNCH_CHECK("ce_ohem_fwd_bwd launch");
  }
  rc = launch_loss_finish(partials, grid, 1.0, dn, loss, 0, st, "ce_ohem_finish launch");
  return rc || !colsum ? rc : launch_colsum_finish(colsum_partials, grid, ldc, colsum, 0, st);
}
