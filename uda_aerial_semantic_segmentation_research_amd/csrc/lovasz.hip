// Lovasz-softmax loss (Berman, Rannen Triki, Blaschko, CVPR 2018): the Lovasz extension of the Jaccard loss, on the device and
// WITHOUT a sort -- on integer histograms of the per-class errors, the way curves.hip builds AUC, with a proved and reported
// bound on what the grid costs (DESIGN.md "Lovasz-softmax on a grid").
//
// THE definition (include/udaseg.h restates it for callers, tests/_lovasz_ref.py in numpy).
//   logits: padded NHWC fp32 [pixels][ldc], ldc % 4 == 0, classes <= ldc <= 32, 0 < pixels < 2^31; target int64.
//   valid(p):      ce_valid of loss_reduce.h.  A valid pixel whose row (channels < classes) is not all finite is void as well.
//   group:         the whole batch (images == 1) or one image (images == N, pixels % images == 0).
//   error:         m = first_max, S = exp_sum (scores_common.h), p_c = expf(z_c - m) / S, e_c = [t == c] ? 1 - p_c : p_c in [0, 1]
//   grid:          bins = B, a power of two in [64, 4096]; bin(e) = min(B - 1, (int)(e * B))  -- lovasz_error below, the ONE
//                  function both passes over the logits take error and bin from, in arithmetic the compiler may not contract
//   tables:        int32 [images][classes][2][B]: row 0 counts the fg pixels (t == c) of each bin, row 1 the bg pixels
//   coefficients:  bins walked from the top; a0, b0 = the fg, bg counts strictly above the bin, p, n = the bin's, G = all fg:
//                    G > 0:   wf = (1 / (G + b0) + 1 / (G + b0 + n)) / 2          per fg pixel of the bin
//                             wb = (G - a0 - p / 2) / ((G + b0) (G + b0 + n))     per bg pixel of the bin
//                    G == 0:  wb = 1 / n in the highest non-empty bin, 0 elsewhere; wf = 0
//                  (the average of the two orders "fg first" / "bg first" inside a bin of tied errors), times the reduction factor:
//                  1 / (images * number of present classes of the group) for a present class and 0 for an absent one, or
//                  1 / (images * classes) with all_classes.  coef: fp32 [images][classes][2][B], computed in float64.
//   slack:         slack[c] = sum over the groups of factor / B * sum over the bins with p + n >= 2 of (p wf + n wb), so that
//                  0 <= (exact sort-based loss) - loss <= sum_c slack[c] <= 1 / B
//   loss:          sum over the valid finite pixels and the classes of e_c * coef[group][c][fg][bin(e_c)]
//   gradient:      d_c = -coef (fg) or +coef (bg), constants; dz_k = p_k (d_k - sum_c p_c d_c)
//   ce_weight:     != 0 adds ce_weight * (mean over the valid finite pixels of -log p_t) and its gradient; the count is
//                  counters[0] of udaseg_lovasz_hist; no such pixel: NaN, CrossEntropyLoss's convention.
// All atomics are on integers, every float sum has a fixed order: the same bits on every run.
#include "launch.h"
#include "loss_reduce.h"

namespace udaseg {

// ---- what the two passes over the logits share ----------------------------------------------------------------------------
enum { LV_LIVE = 0, LV_VOID = 1, LV_INVALID = 2, LV_NONFINITE = 3 };   // the counters' order

// The pixel's kind; a live pixel's row in v, its first maximum m and S = exp_sum.
template <int NV>
__device__ __forceinline__ int lovasz_pixel(const f32x4* __restrict__ row, int64_t t64, int classes, int has_ignore,
                                            int64_t ignore_index, f32x4 (&v)[NV], float& m, float& S) {
  if (has_ignore && t64 == ignore_index) return LV_VOID;
  if ((uint64_t)t64 >= (uint64_t)classes) return LV_INVALID;
  load_row<NV>(row, v);
  bool finite = true;
#pragma unroll
  for (int q = 0; q < NV; ++q)
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (4 * q + e < classes) finite &= __builtin_isfinite(v[q][e]);
  if (!finite) return LV_NONFINITE;
  first_max<NV>(v, classes, m);
  S = exp_sum<NV>(v, classes, m);
  return LV_LIVE;
}

// THE error and bin of one class at one live pixel (both passes).  The explicitly rounded operations keep the compiler from
// fusing 1 - p into the division's last step in one kernel and not in the other; e * B is exact (B is a power of two).
__device__ __forceinline__ float lovasz_error(float z, float m, float S, bool fg, int bins, float& p, int& bin) {
  p = __fdiv_rn(expf(__fsub_rn(z, m)), S);               // <= 1: the numerator is <= 1 and S >= 1
  const float e = fg ? __fsub_rn(1.f, p) : p;
  const int b = (int)__fmul_rn(e, (float)bins);
  bin = b < 0 ? 0 : (b < bins - 1 ? b : bins - 1);
  return e;
}

static inline bool lovasz_bins_ok(int bins) { return bins >= 64 && bins <= 4096 && (bins & (bins - 1)) == 0; }

// ---- pass 1: the error histograms ------------------------------------------------------------------------------------------
// score_hist_kernel's scheme.  A block keeps [cg][2][B] 32-bit counters in 64 KiB of LDS (two blocks a CU on gfx950's 160 KiB):
// cg = min(32, 8192 / B) classes a group -- every class at B <= 256, 16 at 512, 8 at 1024, 4 at 2048, 2 at 4096 -- and the
// groups go over blockIdx.y, each re-reading the logits and redoing the row: 23 classes cost 1 read of the logits at B <= 256,
// 2 at 512, 3 at 1024 (the default), 6 at 2048 and 12 at 4096.  blockIdx.z is the image, so a block stays inside one group.
// Few, long blocks (512 in all): a block flushes one global atomic per NON-EMPTY cell.
// A trained model puts nearly every bg error (p_c ~ 0) and most fg errors (1 - p_t ~ 0) into bin 0, so one LDS address takes most
// of a wave's atomics.  Measured (tools/bench_lovasz.py, 8 x 23 x 512 x 512, bins 1024, one run): the pass takes 218 us on the
// "confident" field (95 % of the pixels with p_t > 0.99) against 219 us on the random one -- the contended case does not
// dominate.  Counting bin 0 per wave with a ballot and a popcount before touching LDS was tried and showed no gain (223 / 230 us
// in its run; two ballots a class and pixel cost what the same-address LDS atomics they save do), so every bin goes to LDS lane
// by lane (profiles/lovasz_bench.txt).
constexpr int LH_CELLS = 16384;
constexpr int LH_THREADS = 512;
constexpr int LH_TOTAL_BLOCKS = 512;
typedef BlockCounts<4, LH_THREADS / 64> LhKinds;          // the four pixel kinds, eight waves a block

template <int LDC4>
__global__ __launch_bounds__(LH_THREADS) void lovasz_hist_kernel(const f32x4* __restrict__ logits, const int64_t* __restrict__ target,
                                                                 int64_t ppi, int classes, int bins, int cg, int has_ignore,
                                                                 int64_t ignore_index, unsigned int* __restrict__ tables,
                                                                 unsigned long long* __restrict__ counters) {
  constexpr int LDC = LDC4 * 4;
  __shared__ unsigned int hist[LH_CELLS];
  __shared__ LhKinds::Slots cnt;
  const int tid = threadIdx.x;
  const int c0 = blockIdx.y * cg;
  const int nc = min(cg, classes - c0);
  const int cells = nc * 2 * bins;                       // <= LH_CELLS
  for (int i = tid; i < cells; i += LH_THREADS) hist[i] = 0;
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.z * ppi;
  unsigned int kinds[4] = {0, 0, 0, 0};
  for (int64_t q0 = (int64_t)blockIdx.x * LH_THREADS; q0 < ppi; q0 += (int64_t)gridDim.x * LH_THREADS) {
    const int64_t q = q0 + tid;
    bool live = false;
    int t = -1;
    f32x4 v[LDC4];
    float m = 0.f, S = 1.f;
    if (q < ppi) {
      const int64_t t64 = target[base + q];
      const int kind = lovasz_pixel<LDC4>(logits + (base + q) * LDC4, t64, classes, has_ignore, ignore_index, v, m, S);
      ++kinds[kind];
      live = kind == LV_LIVE;
      if (live) t = (int)t64;
    }
#pragma unroll
    for (int c = 0; c < LDC; ++c) {
      if (c >= c0 && c < c0 + nc && live) {              // the class test is uniform over the block
        const bool fg = c == t;
        float p;
        int bin;
        lovasz_error(v[c / 4][c % 4], m, S, fg, bins, p, bin);
        atomicAdd(&hist[((c - c0) * 2 + (fg ? 0 : 1)) * bins + bin], 1u);
      }
    }
  }
  if (blockIdx.y == 0) LhKinds::put(cnt, kinds);          // every class group sees the same pixels: the first one counts them
  __syncthreads();                                        // closes the histogram and the slots
  unsigned int* dst = tables + ((size_t)blockIdx.z * classes + c0) * 2 * bins;    // the group's cells are contiguous there
  for (int i = tid; i < cells; i += LH_THREADS) {
    const unsigned int n = hist[i];
    if (n) atomicAdd(&dst[i], n);
  }
  if (blockIdx.y == 0) LhKinds::flush(cnt, counters);
}

// ---- the coefficient tables ------------------------------------------------------------------------------------------------
// Three tiny launches, each reading only what a launch before it wrote (no flags, no waits between blocks):
//   lovasz_present_kernel   one wave per (class, group): present = the fg row has a pixel
//   lovasz_table_kernel     one wave per (class, group): curve_finish_kernel's scheme -- lane j owns the j-th run of B / 64 bins from
//                           the top, the run sums are scanned in lane order, the closed forms are evaluated in float64
//   lovasz_slack_kernel     slack[c] = the groups' parts in group order
constexpr int LT_THREADS = 64;

__global__ __launch_bounds__(LT_THREADS) void lovasz_present_kernel(const unsigned int* __restrict__ tables, int classes, int bins,
                                                                    int* __restrict__ present) {
  const int c = blockIdx.x, g = blockIdx.y;
  const unsigned int* pos = tables + ((size_t)g * classes + c) * 2 * bins;
  unsigned int any = 0;
  for (int i = threadIdx.x; i < bins; i += LT_THREADS) any |= pos[i];
  const unsigned long long b = __ballot(any != 0);
  if (threadIdx.x == 0) present[g * classes + c] = b != 0;
}

__global__ __launch_bounds__(LT_THREADS) void lovasz_table_kernel(const unsigned int* __restrict__ tables,
                                                                  const int* __restrict__ present, int images, int classes, int bins,
                                                                  int all_classes, float* __restrict__ coef,
                                                                  double* __restrict__ slack_parts) {
  __shared__ unsigned long long sp[LT_THREADS], sn[LT_THREADS];
  const int c = blockIdx.x, g = blockIdx.y, j = threadIdx.x;
  const int per = bins / LT_THREADS;
  const size_t row = ((size_t)g * classes + c) * 2 * bins;
  const unsigned int* pos = tables + row;
  const unsigned int* neg = pos + bins;
  const int hi = bins - 1 - j * per;                     // this lane's bins: hi, hi - 1, ..., hi - per + 1
  unsigned long long a = 0, b = 0;
  for (int i = 0; i < per; ++i) {
    a += pos[hi - i];
    b += neg[hi - i];
  }
  sp[j] = a;
  sn[j] = b;
  __syncthreads();
  unsigned long long a0 = 0, b0 = 0, G = 0, N = 0;
  for (int i = 0; i < LT_THREADS; ++i) {
    if (i == j) { a0 = G; b0 = N; }
    G += sp[i];
    N += sn[i];
  }
  int npresent = 0;
  for (int k = 0; k < classes; ++k) npresent += present[g * classes + k];
  double factor;
  if (all_classes)
    factor = 1.0 / ((double)images * (double)classes);
  else
    factor = G > 0 ? 1.0 / ((double)images * (double)npresent) : 0.0;
  const double Gd = (double)G;
  double sl = 0.0;
  for (int i = 0; i < per; ++i) {
    const int bin = hi - i;
    const unsigned long long p = pos[bin], n = neg[bin];
    double wf = 0.0, wb = 0.0;
    if (G > 0) {
      const double d0 = Gd + (double)b0, d1 = d0 + (double)n;
      wf = 0.5 * (1.0 / d0 + 1.0 / d1);
      wb = (Gd - (double)a0 - 0.5 * (double)p) / (d0 * d1);
    } else if (n > 0 && b0 == 0) {
      wb = 1.0 / (double)n;
    }
    coef[row + bin] = (float)(factor * wf);
    coef[row + bins + bin] = (float)(factor * wb);
    if (p + n >= 2) sl += (double)p * wf + (double)n * wb;
    a0 += p;
    b0 += n;
  }
  sl = wave_sum_d(sl);
  if (j == 0) slack_parts[g * classes + c] = factor * sl / (double)bins;
}

__global__ __launch_bounds__(LT_THREADS) void lovasz_slack_kernel(const double* __restrict__ slack_parts, int images, int classes,
                                                                  double* __restrict__ slack) {
  const int c = threadIdx.x;
  if (c >= classes) return;
  double s = 0.0;
  for (int g = 0; g < images; ++g) s += slack_parts[g * classes + c];
  slack[c] = s;
}

// ---- pass 2: loss and gradient ----------------------------------------------------------------------------------------------
// The 256-pixel chunks, the grid and the reductions of the other loss kernels (loss_reduce.h).  Per live pixel: the row, the C
// errors and bins (lovasz_error: the bins of pass 1), C coefficient loads from global memory (the tables of a group are
// classes * 2 * B * 4 bytes: 188 KiB at 23 classes and 1024 bins, and the loads of a trained model gather in bin 0 -- L2 hits).
template <int LDC4, bool GRAD>
__global__ __launch_bounds__(256) void lovasz_fwd_bwd_kernel(const f32x4* __restrict__ logits, const int64_t* __restrict__ target,
                                                             const float* __restrict__ coef, const int64_t* __restrict__ counters,
                                                             int64_t pixels, int64_t ppi, int classes, int bins, int has_ignore,
                                                             int64_t ignore_index, float ce_weight, double* __restrict__ partials,
                                                             f32x4* __restrict__ dlogits, float* __restrict__ colpart) {
  using Tile = GradTile<LDC4>;
  constexpr int LDC = LDC4 * 4;
  __shared__ __attribute__((aligned(16))) float tile[GRAD ? 256 * Tile::LDC : 4];
  __shared__ float colred[GRAD ? Tile::NG * Tile::LDC : 1];
  __shared__ double red[4];
  const int tid = threadIdx.x;
  const bool ce = ce_weight != 0.f;
  const int64_t nlive = ce ? counters[LV_LIVE] : 1;
  const float s = ce && nlive > 0 ? (float)((double)ce_weight / (double)nlive) : 0.f;
  const bool one_group = ppi == pixels;
  const int64_t nchunks = (pixels + 255) / 256;
  float colacc = 0.f;
  double local = 0.0;
  for (int64_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
    const int64_t px = chunk * 256 + tid;
    bool live = false;
    if (px < pixels) {
      const int64_t t64 = target[px];
      f32x4 v[LDC4];
      float m = 0.f, S = 1.f;
      live = lovasz_pixel<LDC4>(logits + px * LDC4, t64, classes, has_ignore, ignore_index, v, m, S) == LV_LIVE;
      if (live) {
        const int t = (int)t64;
        const float* cf = coef + (one_group ? (size_t)0 : (size_t)(px / ppi) * classes * 2 * bins);
        float pr[LDC], d[LDC];
        float lpx = 0.f, dot = 0.f, zt = 0.f;
#pragma unroll
        for (int c = 0; c < LDC; ++c) {
          pr[c] = 0.f;
          d[c] = 0.f;
          if (c < classes) {
            const bool fg = c == t;
            int bin;
            const float e = lovasz_error(v[c / 4][c % 4], m, S, fg, bins, pr[c], bin);
            const float w = cf[(c * 2 + (fg ? 0 : 1)) * bins + bin];
            lpx += e * w;
            d[c] = fg ? -w : w;
            dot += pr[c] * d[c];
            if (fg) zt = v[c / 4][c % 4];
          }
        }
        local += (double)lpx;
        if (ce) local += (double)(s * (logf(S) - (zt - m)));
        if (GRAD) {
#pragma unroll
          for (int k = 0; k < LDC4; ++k) {
            f32x4 gk;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const int c = k * 4 + e;
              float gv = pr[c] * (d[c] - dot);
              if (ce) gv += s * (pr[c] - (c == t ? 1.f : 0.f));
              gk[e] = c < classes ? gv : 0.f;
            }
            Tile::put(*reinterpret_cast<typename Tile::Rows*>(tile), k, gk);
          }
        }
      }
    }
    if (GRAD) {
      if (!live) Tile::put_zero(*reinterpret_cast<typename Tile::Rows*>(tile));
      Tile::flush(*reinterpret_cast<typename Tile::Rows*>(tile), chunk, pixels, dlogits, colpart != nullptr, colacc);
    }
  }
  if (ce && nlive == 0 && blockIdx.x == 0 && tid == 0) local = __longlong_as_double(0x7ff8000000000000LL);
  if (GRAD && colpart) Tile::put_columns(*reinterpret_cast<typename Tile::Cols*>(colred), colacc);
  block_partial(local, red, partials);   // its barrier is the column sums' too
  if (GRAD && colpart) Tile::write_columns(*reinterpret_cast<typename Tile::Cols*>(colred), colpart);
}

// the shape all three calls share
static bool lovasz_shape_ok(const char* who, int images, int classes, int bins) {
  if (images > 0 && images <= 65535 && classes > 0 && classes <= 32 && lovasz_bins_ok(bins)) return true;
  set_error("%s: need 0 < images <= 65535, 0 < classes <= 32, bins a power of two in [64, 4096] (images=%d classes=%d bins=%d)", who,
            images, classes, bins);
  return false;
}
static bool lovasz_pixels_ok(const char* who, int64_t pixels, int images) {
  if (pixels > 0 && pixels < ((int64_t)1 << 31) && pixels % images == 0) return true;
  set_error("%s: need 0 < pixels < 2^31, a multiple of images (pixels=%lld images=%d)", who, (long long)pixels, images);
  return false;
}

}  // namespace udaseg

using namespace udaseg;

extern "C" int udaseg_lovasz_hist(const float* logits, const int64_t* target, int64_t pixels, int classes, int ldc, int has_ignore,
                                  int64_t ignore_index, int images, int bins, int32_t* tables, int64_t* counters, void* stream) {
  UDASEG_CHECK_ARG(logits && target && tables && counters, "lovasz_hist: NULL pointer");
  if (!scores_args_ok("lovasz_hist", pixels, classes, ldc, 32) || !lovasz_shape_ok("lovasz_hist", images, classes, bins) ||
      !lovasz_pixels_ok("lovasz_hist", pixels, images))
    return UDASEG_E_BADARG;
  hipStream_t st = as_stream(stream);
  const int64_t ppi = pixels / images;
  const int cg = LH_CELLS / (2 * bins) < 32 ? LH_CELLS / (2 * bins) : 32;
  const int groups = cdiv(classes, cg);
  int64_t gx = LH_TOTAL_BLOCKS / ((int64_t)groups * images);
  const int64_t want = cdiv64(ppi, LH_THREADS);
  if (gx > want) gx = want;
  if (gx < 1) gx = 1;
  static KernelRec rec(nullptr, "lovasz_hist_kernel");
  KTimer kt(rec, st, (double)pixels * groups * (4.0 * ldc + 8.0));
  if (!dispatch_width<8>(ldc / 4, [&](auto w) {
        hipLaunchKernelGGL(lovasz_hist_kernel<decltype(w)::value>, dim3((unsigned)gx, groups, images), dim3(LH_THREADS), 0, st,
                           (const f32x4*)logits, target, ppi, classes, bins, cg, has_ignore, ignore_index, (unsigned int*)tables,
                           (unsigned long long*)counters);
      }))
    return unsupported_width("lovasz_hist", "ldc", ldc);
  UDASEG_LAUNCH_CHECK("lovasz_hist launch");
  return UDASEG_OK;
}

extern "C" int udaseg_lovasz_table(const int32_t* tables, int images, int classes, int bins, int all_classes, float* coef,
                                   int32_t* present, double* slack_parts, double* slack, void* stream) {
  UDASEG_CHECK_ARG(tables && coef && present && slack_parts && slack, "lovasz_table: NULL pointer");
  if (!lovasz_shape_ok("lovasz_table", images, classes, bins)) return UDASEG_E_BADARG;
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(lovasz_present_kernel, dim3(classes, images), dim3(LT_THREADS), 0, st, (const unsigned int*)tables, classes, bins,
                     present);
  UDASEG_LAUNCH_CHECK("lovasz_present launch");
  hipLaunchKernelGGL(lovasz_table_kernel, dim3(classes, images), dim3(LT_THREADS), 0, st, (const unsigned int*)tables, present, images,
                     classes, bins, all_classes != 0, coef, slack_parts);
  UDASEG_LAUNCH_CHECK("lovasz_table launch");
  hipLaunchKernelGGL(lovasz_slack_kernel, dim3(1), dim3(LT_THREADS), 0, st, slack_parts, images, classes, slack);
  UDASEG_LAUNCH_CHECK("lovasz_slack launch");
  return UDASEG_OK;
}

extern "C" int udaseg_lovasz_fwd_bwd(const float* logits, const int64_t* target, const float* coef, const int64_t* counters,
                                     int64_t pixels, int classes, int ldc, int has_ignore, int64_t ignore_index, int images, int bins,
                                     float ce_weight, double* partials, float* loss, float* dlogits, float* colsum_partials,
                                     float* colsum, void* stream) {
  UDASEG_CHECK_ARG(logits && target && coef && counters && partials && loss, "lovasz_fwd_bwd: NULL pointer");
  if (!scores_args_ok("lovasz_fwd_bwd", pixels, classes, ldc, 32) || !lovasz_shape_ok("lovasz_fwd_bwd", images, classes, bins) ||
      !lovasz_pixels_ok("lovasz_fwd_bwd", pixels, images))
    return UDASEG_E_BADARG;
  UDASEG_CHECK_ARG(ce_weight == ce_weight && ce_weight - ce_weight == 0.f, "lovasz_fwd_bwd: ce_weight must be finite");
  UDASEG_CHECK_ARG((colsum == nullptr) == (colsum_partials == nullptr), "lovasz_fwd_bwd: colsum and colsum_partials come together");
  UDASEG_CHECK_ARG(dlogits || !colsum, "lovasz_fwd_bwd: column sums need dlogits");
  hipStream_t st = as_stream(stream);
  const int grid = capped_grid(pixels, 256, udaseg_ce_partials());
  const int64_t ppi = pixels / images;
  {
    static KernelRec rec(nullptr, "lovasz_fwd_bwd_kernel");
    KTimer kt(rec, st, (double)pixels * (4.0 * ldc * (dlogits ? 2.0 : 1.0) + 8.0 + 4.0 * classes));
    if (!dispatch_width<8>(ldc / 4, [&](auto w) {
          constexpr int W = decltype(w)::value;
          if (dlogits)
            hipLaunchKernelGGL((lovasz_fwd_bwd_kernel<W, true>), dim3(grid), dim3(256), 0, st, (const f32x4*)logits, target, coef,
                               counters, pixels, ppi, classes, bins, has_ignore, ignore_index, ce_weight, partials, (f32x4*)dlogits,
                               colsum_partials);
          else
            hipLaunchKernelGGL((lovasz_fwd_bwd_kernel<W, false>), dim3(grid), dim3(256), 0, st, (const f32x4*)logits, target, coef,
                               counters, pixels, ppi, classes, bins, has_ignore, ignore_index, ce_weight, partials, (f32x4*)nullptr,
                               (float*)nullptr);
        }))
      return unsupported_width("lovasz_fwd_bwd", "ldc", ldc);
    UDASEG_LAUNCH_CHECK("lovasz_fwd_bwd launch");
  }
  const int rc = launch_loss_finish(partials, grid, 1.0, nullptr, loss, 0, st, "lovasz_finish launch");
  return rc || !colsum ? rc : launch_colsum_finish(colsum_partials, grid, ldc, colsum, 0, st);
}
