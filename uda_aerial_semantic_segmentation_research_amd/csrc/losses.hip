// Loss kernels (no MFMA; wavefront reductions), fp32 (gfx950).
//
//  * per-pixel cross entropy, mean reduction, no class weights / ignore_index:
//      nn.CrossEntropyLoss() constructed at reference src/models/train.py:208, applied at :342,:403 and at
//      src/models/adversarial_trainer.py:105,155.
//  * discriminator tail  AdaptiveAvgPool2d(1) -> Flatten -> Linear(512,1) -> Sigmoid
//      (src/models/discriminator.py:37-42) and its autograd.
//  * AdversarialLoss' nn.BCEWithLogitsLoss terms (src/models/losses.py:16,33-36,51).  The reference feeds the
//      discriminator's *probabilities* into the with-logits loss; these kernels are agnostic: they compute
//      mean(softplus(x) - x*label) of whatever x is.
// The block partials, the LDS gradient tile and the finish kernels of the cross-entropy kernels are loss_reduce.h's.
#include "loss_reduce.h"

namespace udaseg {

constexpr int CE_BLOCKS = 1024;
constexpr int CE_SIMPLE_BLOCKS = 4096;   // the one-thread-per-pixel backward kernels of ldc > 32
constexpr int CE_MAXC = 64;

// One thread per pixel, logits row in registers (classes <= 64, ldc % 4 == 0).  HBM-bound: 4*ldc B/pixel read.
template <int LDC4>
__global__ __launch_bounds__(256) void ce_fwd_kernel(const f32x4* __restrict__ logits, const int64_t* __restrict__ target,
                                                     int64_t pixels, int classes, float* __restrict__ lse,
                                                     double* __restrict__ partials) {
  __shared__ double red[4];
  const int64_t T = (int64_t)gridDim.x * blockDim.x;
  double local = 0.0;
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < pixels; p += T) {
    f32x4 v[LDC4];
#pragma unroll
    for (int k = 0; k < LDC4; ++k) v[k] = logits[p * LDC4 + k];
    float mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < LDC4; ++k)
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (k * 4 + e < classes) mx = fmaxf(mx, v[k][e]);
    float sum = 0.f;
    const int t = (int)target[p];
    float xt = 0.f;
#pragma unroll
    for (int k = 0; k < LDC4; ++k)
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (k * 4 + e < classes) {
          sum += expf(v[k][e] - mx);
          if (k * 4 + e == t) xt = v[k][e];
        }
    const float l = mx + logf(sum);
    lse[p] = l;
    local += (double)(l - xt);
  }
  block_partial(local, red, partials);
}

// Generic fallback (ldc > 32): one thread per pixel, strided 16-B stores.
template <int LDC4>
__global__ __launch_bounds__(256) void ce_bwd_simple_kernel(const f32x4* __restrict__ logits, const int64_t* __restrict__ target,
                                                            const float* __restrict__ lse, const float* __restrict__ grad_out,
                                                            int64_t pixels, int classes, f32x4* __restrict__ dlogits) {
  const float scale = (grad_out ? *grad_out : 1.f) / (float)pixels;
  const int64_t T = (int64_t)gridDim.x * blockDim.x;
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < pixels; p += T) {
    const float l = lse[p];
    const int t = (int)target[p];
#pragma unroll
    for (int k = 0; k < LDC4; ++k) {
      const f32x4 v = logits[p * LDC4 + k];
      f32x4 g;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int c = k * 4 + e;
        g[e] = c < classes ? (expf(v[e] - l) - (c == t ? 1.f : 0.f)) * scale : 0.f;
      }
      dlogits[p * LDC4 + k] = g;
    }
  }
}

// ldc <= 32: blocks walk 256-pixel chunks; gradients go out through the LDS tile (GradTile, loss_reduce.h), which also yields
// the per-class column sums.  colpart: [gridDim.x][LDC] or null.
template <int LDC4>
__global__ __launch_bounds__(256) void ce_bwd_kernel(const f32x4* __restrict__ logits, const int64_t* __restrict__ target,
                                                     const float* __restrict__ lse, const float* __restrict__ grad_out,
                                                     int64_t pixels, int classes, f32x4* __restrict__ dlogits,
                                                     float* __restrict__ colpart) {
  using Tile = GradTile<LDC4>;
  __shared__ __attribute__((aligned(16))) float tile[256 * Tile::LDC];
  __shared__ float colred[Tile::NG * Tile::LDC];
  const int tid = threadIdx.x;
  const float scale = (grad_out ? *grad_out : 1.f) / (float)pixels;
  const int64_t nchunks = (pixels + 255) / 256;
  float colacc = 0.f;
  for (int64_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
    const int64_t p = chunk * 256 + tid;
    if (p < pixels) {
      const float l = lse[p];
      const int t = (int)target[p];
#pragma unroll
      for (int k = 0; k < LDC4; ++k) {
        const f32x4 v = logits[p * LDC4 + k];
        f32x4 g;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int c = k * 4 + e;
          g[e] = c < classes ? (expf(v[e] - l) - (c == t ? 1.f : 0.f)) * scale : 0.f;
        }
        Tile::put(tile, k, g);
      }
    } else {
      Tile::put_zero(tile);
    }
    Tile::flush(tile, chunk, pixels, dlogits, colpart != nullptr, colacc);
  }
  if (colpart) Tile::finish(colred, colpart, colacc);
}

// Forward and backward in ONE pass over the logits (round 5): the loss partials of ce_fwd_kernel (same pixel-to-thread map, same
// block reduction: the loss is bit-identical) and the gradient of ce_bwd_kernel for an upstream gradient of 1 (scale 1 / pixels; same
// expressions: bit-identical), through the same LDS tile with the same column sums.  The training step read the 200 MB of logits
// twice (ce_fwd for the loss, ce_bwd for the gradient); loss.backward() hands this loss a gradient of exactly 1, and
// scale_unless_one_kernel below covers every other caller.
template <int LDC4>
__global__ __launch_bounds__(256) void ce_fwd_bwd_kernel(const f32x4* __restrict__ logits, const int64_t* __restrict__ target,
                                                         int64_t pixels, int classes, double* __restrict__ partials,
                                                         f32x4* __restrict__ dlogits, float* __restrict__ colpart) {
  using Tile = GradTile<LDC4>;
  __shared__ __attribute__((aligned(16))) float tile[256 * Tile::LDC];
  __shared__ float colred[Tile::NG * Tile::LDC];
  __shared__ double red[4];
  const int tid = threadIdx.x;
  const float scale = 1.f / (float)pixels;
  const int64_t nchunks = (pixels + 255) / 256;
  float colacc = 0.f;
  double local = 0.0;
  for (int64_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
    const int64_t p = chunk * 256 + tid;
    if (p < pixels) {
      f32x4 v[LDC4];
#pragma unroll
      for (int k = 0; k < LDC4; ++k) v[k] = logits[p * LDC4 + k];
      float mx = -INFINITY;
#pragma unroll
      for (int k = 0; k < LDC4; ++k)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (k * 4 + e < classes) mx = fmaxf(mx, v[k][e]);
      float sum = 0.f;
      const int t = (int)target[p];
      float xt = 0.f;
#pragma unroll
      for (int k = 0; k < LDC4; ++k)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (k * 4 + e < classes) {
            sum += expf(v[k][e] - mx);
            if (k * 4 + e == t) xt = v[k][e];
          }
      const float l = mx + logf(sum);
      local += (double)(l - xt);
#pragma unroll
      for (int k = 0; k < LDC4; ++k) {
        f32x4 g;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int c = k * 4 + e;
          g[e] = c < classes ? (expf(v[k][e] - l) - (c == t ? 1.f : 0.f)) * scale : 0.f;
        }
        Tile::put(tile, k, g);
      }
    } else {
      Tile::put_zero(tile);
    }
    Tile::flush(tile, chunk, pixels, dlogits, colpart != nullptr, colacc);
  }
  if (colpart) Tile::put_columns(colred, colacc);
  block_partial(local, red, partials);   // its barrier is the column sums' too
  if (colpart) Tile::write_columns(colred, colpart);
}

// x[i] *= *g unless *g == 1 (then the launch returns at once: the gradient made for an upstream gradient of 1 is already right)
__global__ void scale_unless_one_kernel(f32x4* __restrict__ x, int64_t n4, float* __restrict__ x2, int n2, const float* __restrict__ g) {
  const float s = *g;
  if (s == 1.f) return;
  const int64_t T = (int64_t)gridDim.x * blockDim.x;
  const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (int64_t i = i0; i < n4; i += T) x[i] = x[i] * s;
  if (x2 != nullptr && i0 < n2) x2[i0] *= s;
}

// ---- cross entropy with options: class weights w, ignore_index, label smoothing eps, reductions none / sum / mean --------------
// (torch.nn.functional.cross_entropy's definition).  A second set of kernels: the plain ones above stay as they are.
//   valid(p):  t != ignore_index and 0 <= t < classes   (an out-of-range t that is not ignore_index is void too, and counted)
//   l_p      = (1-eps) * w[t] * (lse - z_t) + (eps/C) * sum_c w[c] * (lse - z_c)            for a valid pixel, exactly 0 otherwise
//   dl_p/dz_k = (1-eps) * w[t] * (P_k - [k==t]) + (eps/C) * (P_k * sum_c w[c] - w[k])       exactly 0 at void pixels, all ldc lanes
//   'mean' divides both by D = sum over valid p of w[t_p], which ce_target_stats_kernel makes from the targets alone (8 B/pixel)
//   BEFORE the one pass over the logits, so that pass writes the gradient already scaled.
// partials[k][block], k = 0: sum of w[t] over valid pixels (f64), 1..3: valid / void (== ignore_index) / invalid pixel counts
// (whole numbers < 2^53: exact in f64).  Fixed pixel-to-thread map and fixed-order reductions: two calls give the same bits.
__global__ __launch_bounds__(256) void ce_target_stats_kernel(const int64_t* __restrict__ target, const float* __restrict__ weight,
                                                              int64_t pixels, int classes, int has_ignore, int64_t ignore_index,
                                                              double* __restrict__ partials) {
  __shared__ float wsh[CE_MAXC];
  __shared__ double red[4][4];
  if ((int)threadIdx.x < classes) wsh[threadIdx.x] = weight ? weight[threadIdx.x] : 1.f;
  __syncthreads();
  const int64_t T = (int64_t)gridDim.x * blockDim.x;
  double d = 0.0;
  int nvalid = 0, nvoid = 0, ninvalid = 0;
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < pixels; p += T) {
    const int64_t t = target[p];
    if (has_ignore && t == ignore_index) {
      ++nvoid;
    } else if ((uint64_t)t < (uint64_t)classes) {
      ++nvalid;
      d += (double)wsh[(int)t];
    } else {
      ++ninvalid;
    }
  }
  double v[4] = {d, (double)nvalid, (double)nvoid, (double)ninvalid};
  block_partial_rows<4>(v, red, partials);
}

// The per-pixel terms shared by the optioned kernels (ce_valid and ce_row_lse: loss_reduce.h, shared with ohem.hip).
// wsh: the class weights in LDS (1 where no weights were given).
template <int LDC4, bool SMOOTH>
__device__ __forceinline__ float ce_opt_pixel_loss(const f32x4 (&v)[LDC4], int classes, float l, float xt, float wt, float om, float es,
                                                   const float* wsh) {
  float lp = om * wt * (l - xt);
  if (SMOOTH) {
    float S = 0.f;
#pragma unroll
    for (int k = 0; k < LDC4; ++k)
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (k * 4 + e < classes) S += wsh[k * 4 + e] * (l - v[k][e]);
    lp += es * S;
  }
  return lp;
}

// g_c = s * [ (1-eps) w_t (P_c - [c==t]) + (eps/C) (P_c * wsum - w_c) ]   (s: everything the gradient is scaled by)
template <bool SMOOTH>
__device__ __forceinline__ float ce_opt_grad(float z, float l, bool is_t, float a /* s*(1-eps)*w_t */, float pk /* a + s*es*wsum */,
                                             float ek /* s*es */, float wc) {
  float g = expf(z - l) * (SMOOTH ? pk : a) - (is_t ? a : 0.f);
  if (SMOOTH) g -= ek * wc;
  return g;
}

// ONE pass over the logits, as ce_fwd_bwd_kernel: loss partials, the gradient (already scaled by 1/D for 'mean') through the LDS tile
// as whole contiguous lines, and the per-class column sums (the head conv's bias gradient).
template <int LDC4, bool SMOOTH>
__global__ __launch_bounds__(256) void ce_opt_fwd_bwd_kernel(const f32x4* __restrict__ logits, const int64_t* __restrict__ target,
                                                             const float* __restrict__ weight, int64_t pixels, int classes,
                                                             int has_ignore, int64_t ignore_index, float eps,
                                                             const double* __restrict__ denom, double* __restrict__ partials,
                                                             f32x4* __restrict__ dlogits, float* __restrict__ colpart) {
  using Tile = GradTile<LDC4>;
  __shared__ __attribute__((aligned(16))) float tile[256 * Tile::LDC];
  __shared__ float colred[Tile::NG * Tile::LDC];
  __shared__ double red[4];
  __shared__ float wsh[32];
  const int tid = threadIdx.x;
  if (tid < 32) wsh[tid] = tid < classes ? (weight ? weight[tid] : 1.f) : 0.f;
  __syncthreads();
  float wsum = 0.f;
  if (SMOOTH)
    for (int c = 0; c < classes; ++c) wsum += wsh[c];
  const float scale = denom ? (float)(1.0 / *denom) : 1.f;
  const float om = SMOOTH ? 1.f - eps : 1.f, es = SMOOTH ? eps / (float)classes : 0.f;
  const int64_t nchunks = (pixels + 255) / 256;
  float colacc = 0.f;
  double local = 0.0;
  for (int64_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
    const int64_t p = chunk * 256 + tid;
    bool ok = p < pixels;
    int t = 0;
    if (ok) {
      const int64_t t64 = target[p];
      ok = ce_valid(t64, classes, has_ignore, ignore_index);
      t = ok ? (int)t64 : 0;
    }
    if (ok) {
      f32x4 v[LDC4];
#pragma unroll
      for (int k = 0; k < LDC4; ++k) v[k] = logits[p * LDC4 + k];
      float xt;
      const float l = ce_row_lse<LDC4>(v, classes, t, xt);
      const float wt = wsh[t];
      local += (double)ce_opt_pixel_loss<LDC4, SMOOTH>(v, classes, l, xt, wt, om, es, wsh);
      const float a = scale * om * wt, pk = a + scale * es * wsum, ek = scale * es;
#pragma unroll
      for (int k = 0; k < LDC4; ++k) {
        f32x4 g;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int c = k * 4 + e;
          g[e] = c < classes ? ce_opt_grad<SMOOTH>(v[k][e], l, c == t, a, pk, ek, wsh[c]) : 0.f;
        }
        Tile::put(tile, k, g);
      }
    } else {
      Tile::put_zero(tile);
    }
    Tile::flush(tile, chunk, pixels, dlogits, colpart != nullptr, colacc);
  }
  if (colpart) Tile::put_columns(colred, colacc);
  block_partial(local, red, partials);   // its barrier is the column sums' too
  if (colpart) Tile::write_columns(colred, colpart);
}

// Two-pass route, forward: lse[p] kept for the backward, loss_px[p] = l_p ('none'; may be null), block partials of sum l_p.
template <int LDC4, bool SMOOTH>
__global__ __launch_bounds__(256) void ce_opt_fwd_kernel(const f32x4* __restrict__ logits, const int64_t* __restrict__ target,
                                                         const float* __restrict__ weight, int64_t pixels, int classes,
                                                         int has_ignore, int64_t ignore_index, float eps, float* __restrict__ lse,
                                                         float* __restrict__ loss_px, double* __restrict__ partials) {
  __shared__ double red[4];
  __shared__ float wsh[CE_MAXC];
  if (threadIdx.x < CE_MAXC) wsh[threadIdx.x] = (int)threadIdx.x < classes ? (weight ? weight[threadIdx.x] : 1.f) : 0.f;
  __syncthreads();
  const float om = SMOOTH ? 1.f - eps : 1.f, es = SMOOTH ? eps / (float)classes : 0.f;
  const int64_t T = (int64_t)gridDim.x * blockDim.x;
  double local = 0.0;
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < pixels; p += T) {
    const int64_t t64 = target[p];
    float l = 0.f, lp = 0.f;
    if (ce_valid(t64, classes, has_ignore, ignore_index)) {
      const int t = (int)t64;
      f32x4 v[LDC4];
#pragma unroll
      for (int k = 0; k < LDC4; ++k) v[k] = logits[p * LDC4 + k];
      float xt;
      l = ce_row_lse<LDC4>(v, classes, t, xt);
      lp = ce_opt_pixel_loss<LDC4, SMOOTH>(v, classes, l, xt, wsh[t], om, es, wsh);
    }
    lse[p] = l;
    if (loss_px) loss_px[p] = lp;
    local += (double)lp;
  }
  block_partial(local, red, partials);
}

// Two-pass route, backward.  The upstream gradient is the scalar *grad_out (null = 1) times, for 'none', grad_px[p].
// TILED (ldc <= 32): through the LDS tile with column sums, as ce_bwd_kernel; otherwise one thread per pixel, strided stores.
template <int LDC4, bool SMOOTH, bool TILED>
__global__ __launch_bounds__(256) void ce_opt_bwd_kernel(const f32x4* __restrict__ logits, const int64_t* __restrict__ target,
                                                         const float* __restrict__ weight, const float* __restrict__ lse,
                                                         const float* __restrict__ grad_out, const float* __restrict__ grad_px,
                                                         int64_t pixels, int classes, int has_ignore, int64_t ignore_index, float eps,
                                                         const double* __restrict__ denom, f32x4* __restrict__ dlogits,
                                                         float* __restrict__ colpart) {
  using Tile = GradTile<LDC4>;
  __shared__ __attribute__((aligned(16))) float tile[256 * Tile::LDC];   // !TILED: nothing touches the two, and they take no LDS
  __shared__ float colred[Tile::NG * Tile::LDC];
  __shared__ float wsh[CE_MAXC];
  const int tid = threadIdx.x;
  if (tid < CE_MAXC) wsh[tid] = tid < classes ? (weight ? weight[tid] : 1.f) : 0.f;
  __syncthreads();
  float wsum = 0.f;
  if (SMOOTH)
    for (int c = 0; c < classes; ++c) wsum += wsh[c];
  const float scale = (grad_out ? *grad_out : 1.f) * (denom ? (float)(1.0 / *denom) : 1.f);
  const float om = SMOOTH ? 1.f - eps : 1.f, es = SMOOTH ? eps / (float)classes : 0.f;
  const int64_t nchunks = (pixels + 255) / 256;
  float colacc = 0.f;
  for (int64_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
    const int64_t p = chunk * 256 + tid;
    bool ok = p < pixels;
    int t = 0;
    if (ok) {
      const int64_t t64 = target[p];
      ok = ce_valid(t64, classes, has_ignore, ignore_index);
      t = ok ? (int)t64 : 0;
    }
    if (ok) {
      const float l = lse[p];
      const float s = grad_px ? scale * grad_px[p] : scale;
      const float a = s * om * wsh[t], pk = a + s * es * wsum, ek = s * es;
#pragma unroll
      for (int k = 0; k < LDC4; ++k) {
        const f32x4 v = logits[p * LDC4 + k];
        f32x4 g;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int c = k * 4 + e;
          g[e] = c < classes ? ce_opt_grad<SMOOTH>(v[e], l, c == t, a, pk, ek, wsh[c]) : 0.f;
        }
        if (TILED) Tile::put(tile, k, g);
        else dlogits[p * LDC4 + k] = g;
      }
    } else if (TILED) {
      Tile::put_zero(tile);
    } else if (p < pixels) {
#pragma unroll
      for (int k = 0; k < LDC4; ++k) dlogits[p * LDC4 + k] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    if (TILED) Tile::flush(tile, chunk, pixels, dlogits, colpart != nullptr, colacc);
  }
  if (TILED && colpart) Tile::finish(colred, colpart, colacc);
}

// ---- validation metrics: per-pixel argmax + confusion matrix (SegmentationTrainer.calculate_metrics, reference
// src/models/train.py:225-243; confusion-matrix definition src/analysis/metrics.py:17-29: bincount(C*true + pred)).
// One thread per pixel, row in registers; the block's histogram lives in LDS (classes <= 32 -> 4 KiB of counters), one
// global atomic per non-empty cell per block.  argmax tie rule = first_max (scores_common.h).
template <int LDC4>
__global__ __launch_bounds__(256) void argmax_confusion_kernel(const f32x4* __restrict__ logits, const int64_t* __restrict__ target,
                                                               int64_t pixels, int classes, unsigned long long* __restrict__ cm,
                                                               int64_t* __restrict__ pred_out) {
  __shared__ unsigned int hist[32 * 32];
  for (int i = threadIdx.x; i < classes * classes; i += 256) hist[i] = 0;
  __syncthreads();
  const int64_t T = (int64_t)gridDim.x * blockDim.x;
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < pixels; p += T) {
    f32x4 v[LDC4];
    load_row<LDC4>(logits + p * LDC4, v);
    float best;
    const int bi = first_max<LDC4>(v, classes, best);
    if (pred_out) pred_out[p] = bi;
    const int t = (int)target[p];
    if ((unsigned)t < (unsigned)classes) atomicAdd(&hist[t * classes + bi], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < classes * classes; i += 256)
    if (hist[i]) atomicAdd(&cm[i], (unsigned long long)hist[i]);
}

// ---- discriminator tail ---------------------------------------------------------------------------------------
constexpr int GAP_SPLITS = 32;

// partial[n][s][c] = sum over the s-th slice of the hw pixels of z[n][p][c]
__global__ void gap_partial_kernel(const f32x4* __restrict__ z, f32x4* __restrict__ partial, int hw, int c4, int splits) {
  const int ni = blockIdx.y, s = blockIdx.x;
  const int per = (hw + splits - 1) / splits;
  const int p0 = s * per, p1 = min(hw, p0 + per);
  for (int q = threadIdx.x; q < c4; q += blockDim.x) {
    f32x4 acc = {0, 0, 0, 0};
    for (int p = p0; p < p1; ++p) acc += z[((int64_t)ni * hw + p) * c4 + q];
    partial[((int64_t)ni * splits + s) * c4 + q] = acc;
  }
}

// one block per image: pooled = sum_s partial / hw ; p = sigmoid(dot(pooled, w) + b)
__global__ __launch_bounds__(256) void gap_linear_sigmoid_kernel(const float* __restrict__ partial, const float* __restrict__ w,
                                                                 const float* __restrict__ b, float* __restrict__ pooled,
                                                                 float* __restrict__ p, int hw, int c, int splits,
                                                                 int sigmoid) {
  __shared__ float red[4];
  const int ni = blockIdx.x;
  float dot = 0.f;
  const float inv = 1.f / (float)hw;
  for (int ch = threadIdx.x; ch < c; ch += blockDim.x) {
    float s = 0.f;
    for (int k = 0; k < splits; ++k) s += partial[((int64_t)ni * splits + k) * c + ch];
    s *= inv;
    pooled[(int64_t)ni * c + ch] = s;
    dot += s * w[ch];
  }
  dot = wave_sum(dot);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = dot;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float t = red[0] + red[1] + red[2] + red[3] + b[0];
    p[ni] = sigmoid ? 1.f / (1.f + expf(-t)) : t;
  }
}

// dz[n][p][c] = dlogit[n] * w[c] / hw, broadcast over the hw pixels
__global__ void gap_bwd_broadcast_kernel(const float* __restrict__ dp, const float* __restrict__ p, const f32x4* __restrict__ w,
                                         f32x4* __restrict__ dz, int n, int hw, int c4, int sigmoid) {
  const int64_t total = (int64_t)n * hw * c4;
  const int64_t T = (int64_t)gridDim.x * blockDim.x;
  const float inv = 1.f / (float)hw;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += T) {
    const int q = (int)(i % c4);
    const int ni = (int)(i / ((int64_t)hw * c4));
    const float pv = sigmoid ? p[ni] : 0.f;
    const float dl = dp[ni] * (sigmoid ? pv * (1.f - pv) : 1.f) * inv;
    dz[i] = w[q] * dl;
  }
}

// dw[c] (+)= sum_n dlogit[n]*pooled[n][c] ; db (+)= sum_n dlogit[n]
__global__ void gap_bwd_param_kernel(const float* __restrict__ dp, const float* __restrict__ p, const float* __restrict__ pooled,
                                     float* __restrict__ dw, float* __restrict__ db, int n, int c, int accumulate, int sigmoid) {
  for (int ch = blockIdx.x * blockDim.x + threadIdx.x; ch < c; ch += gridDim.x * blockDim.x) {
    float s = 0.f;
    for (int ni = 0; ni < n; ++ni) s += dp[ni] * (sigmoid ? p[ni] * (1.f - p[ni]) : 1.f) * pooled[(int64_t)ni * c + ch];
    dw[ch] = accumulate ? dw[ch] + s : s;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    float s = 0.f;
    for (int ni = 0; ni < n; ++ni) s += dp[ni] * (sigmoid ? p[ni] * (1.f - p[ni]) : 1.f);
    db[0] = accumulate ? db[0] + s : s;
  }
}

// ---- BCE with logits on a short vector: single wave -------------------------------------------------------------
__device__ __forceinline__ float softplus_f(float x) {
  // log(1 + exp(x)) = max(x,0) + log1p(exp(-|x|))
  return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x)));
}

__global__ void bce_fwd_kernel(const float* __restrict__ x, int n, float label, float weight, float* __restrict__ loss,
                               int accumulate) {
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += 64) {
    const float v = x[i];
    // torch: (1 - y) * x + softplus(-x)   [= max(-x,0) + log1p(exp(-|x|)) form]
    s += (1.f - label) * v + softplus_f(-v);
  }
  s = wave_sum(s);
  if (threadIdx.x == 0) {
    const float l = weight * (s / (float)n);
    *loss = accumulate ? *loss + l : l;
  }
}

__global__ void bce_bwd_kernel(const float* __restrict__ x, int n, float label, float weight, const float* __restrict__ grad_out,
                               float* __restrict__ dx, int accumulate) {
  const float g = (grad_out ? *grad_out : 1.f) * weight / (float)n;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const float v = x[i];
    const float sg = 1.f / (1.f + expf(-v));
    const float d = (sg - label) * g;
    dx[i] = accumulate ? dx[i] + d : d;
  }
}

// per-sample targets (nn.BCEWithLogitsLoss()(x, y), reference src/models/uda.py:85,96)
__global__ void bce_target_fwd_kernel(const float* __restrict__ x, const float* __restrict__ y, int n, float weight,
                                      float* __restrict__ loss, int accumulate) {
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += 64) s += (1.f - y[i]) * x[i] + softplus_f(-x[i]);
  s = wave_sum(s);
  if (threadIdx.x == 0) {
    const float l = weight * (s / (float)n);
    *loss = accumulate ? *loss + l : l;
  }
}

__global__ void bce_target_bwd_kernel(const float* __restrict__ x, const float* __restrict__ y, int n, float weight,
                                      const float* __restrict__ grad_out, float* __restrict__ dx, int accumulate) {
  const float g = (grad_out ? *grad_out : 1.f) * weight / (float)n;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const float d = (1.f / (1.f + expf(-x[i])) - y[i]) * g;
    dx[i] = accumulate ? dx[i] + d : d;
  }
}

}  // namespace udaseg

using namespace udaseg;

extern "C" int udaseg_ce_partials(void) { return CE_BLOCKS; }

extern "C" int udaseg_ce_fwd(const float* logits, const int64_t* target, int64_t pixels, int classes, int ldc, float* lse,
                             double* partials, float* loss, void* stream) {
  UDASEG_CHECK_ARG(logits && target && lse && partials && loss, "ce_fwd: NULL pointer");
  UDASEG_CHECK_ARG(pixels > 0 && classes > 0 && classes <= ldc && ldc % 4 == 0 && ldc <= CE_MAXC,
                   "ce_fwd: need 0 < classes <= ldc <= %d, ldc %% 4 == 0 (classes=%d ldc=%d)", CE_MAXC, classes, ldc);
  hipStream_t st = as_stream(stream);
  const int grid = capped_grid(pixels, 256, CE_BLOCKS);
  if (!dispatch_width<16>(ldc / 4, [&](auto w) {
        hipLaunchKernelGGL(ce_fwd_kernel<decltype(w)::value>, dim3(grid), dim3(256), 0, st, (const f32x4*)logits, target, pixels,
                           classes, lse, partials);
      }))
    return unsupported_width("ce_fwd", "ldc", ldc);
  UDASEG_LAUNCH_CHECK("ce_fwd launch");
  return launch_loss_finish(partials, grid, (double)pixels, nullptr, loss, 0, st, "ce_finish launch");
}

extern "C" int udaseg_ce_fwd_bwd(const float* logits, const int64_t* target, int64_t pixels, int classes, int ldc, double* partials,
                                 float* loss, float* dlogits, float* colsum_partials, float* colsum, void* stream) {
  UDASEG_CHECK_ARG(logits && target && partials && loss && dlogits, "ce_fwd_bwd: NULL pointer");
  UDASEG_CHECK_ARG(pixels > 0 && classes > 0 && classes <= ldc && ldc % 4 == 0 && ldc <= 32,
                   "ce_fwd_bwd: need 0 < classes <= ldc <= 32, ldc %% 4 == 0 (classes=%d ldc=%d)", classes, ldc);
  UDASEG_CHECK_ARG((colsum == nullptr) == (colsum_partials == nullptr), "ce_fwd_bwd: colsum and colsum_partials come together");
  hipStream_t st = as_stream(stream);
  const int grid = capped_grid(pixels, 256, CE_BLOCKS);
  if (!dispatch_width<8>(ldc / 4, [&](auto w) {
        hipLaunchKernelGGL(ce_fwd_bwd_kernel<decltype(w)::value>, dim3(grid), dim3(256), 0, st, (const f32x4*)logits, target, pixels,
                           classes, partials, (f32x4*)dlogits, colsum_partials);
      }))
    return unsupported_width("ce_fwd_bwd", "ldc", ldc);
  UDASEG_LAUNCH_CHECK("ce_fwd_bwd launch");
  const int rc = launch_loss_finish(partials, grid, (double)pixels, nullptr, loss, 0, st, "ce_finish launch");
  return rc || !colsum ? rc : launch_colsum_finish(colsum_partials, grid, ldc, colsum, 0, st);
}

extern "C" int udaseg_scale_unless_one(float* x, int64_t count, float* x2, int count2, const float* g, void* stream) {
  UDASEG_CHECK_ARG(x && g && count > 0 && count % 4 == 0 && count2 >= 0 && count2 <= 256 && (x2 != nullptr || count2 == 0),
                   "scale_unless_one: bad arguments");
  const int64_t n4 = count / 4;
  int64_t grid = (n4 + 1023) / 1024;
  if (grid > 2048) grid = 2048;
  if (grid < 1) grid = 1;
  hipLaunchKernelGGL(scale_unless_one_kernel, dim3((unsigned)grid), dim3(256), 0, as_stream(stream), (f32x4*)x, n4, x2, count2, g);
  UDASEG_LAUNCH_CHECK("scale_unless_one launch");
  return UDASEG_OK;
}

extern "C" int udaseg_ce_bwd(const float* logits, const int64_t* target, const float* lse, const float* grad_out,
                             int64_t pixels, int classes, int ldc, float* dlogits, float* colsum_partials, float* colsum,
                             void* stream) {
  UDASEG_CHECK_ARG(logits && target && lse && dlogits, "ce_bwd: NULL pointer");
  UDASEG_CHECK_ARG(pixels > 0 && classes > 0 && classes <= ldc && ldc % 4 == 0 && ldc <= CE_MAXC, "ce_bwd: bad shape");
  UDASEG_CHECK_ARG((colsum == nullptr) == (colsum_partials == nullptr), "ce_bwd: colsum and colsum_partials come together");
  UDASEG_CHECK_ARG(colsum == nullptr || ldc <= 32, "ce_bwd: fused column sums need ldc <= 32");
  hipStream_t st = as_stream(stream);
  const int grid = capped_grid(pixels, 256, ldc <= 32 ? CE_BLOCKS : CE_SIMPLE_BLOCKS);
  if (!dispatch_width<16>(ldc / 4, [&](auto w) {
        constexpr int W = decltype(w)::value;
        if constexpr (W <= 8)
          hipLaunchKernelGGL(ce_bwd_kernel<W>, dim3(grid), dim3(256), 0, st, (const f32x4*)logits, target, lse, grad_out, pixels,
                             classes, (f32x4*)dlogits, colsum_partials);
        else
          hipLaunchKernelGGL(ce_bwd_simple_kernel<W>, dim3(grid), dim3(256), 0, st, (const f32x4*)logits, target, lse, grad_out,
                             pixels, classes, (f32x4*)dlogits);
      }))
    return unsupported_width("ce_bwd", "ldc", ldc);
  UDASEG_LAUNCH_CHECK("ce_bwd launch");
  return colsum ? launch_colsum_finish(colsum_partials, grid, ldc, colsum, 0, st) : UDASEG_OK;
}

extern "C" int udaseg_argmax_confusion(const float* logits, const int64_t* target, int64_t pixels, int classes, int ldc,
                                       int64_t* confusion, int64_t* pred, void* stream) {
  UDASEG_CHECK_ARG(logits && target && confusion, "argmax_confusion: NULL pointer");
  if (!scores_args_ok("argmax_confusion", pixels, classes, ldc, 32)) return UDASEG_E_BADARG;
  const int grid = capped_grid(pixels, 256, 1024);
  if (!dispatch_width<8>(ldc / 4, [&](auto w) {
        hipLaunchKernelGGL(argmax_confusion_kernel<decltype(w)::value>, dim3(grid), dim3(256), 0, as_stream(stream),
                           (const f32x4*)logits, target, pixels, classes, (unsigned long long*)confusion, pred);
      }))
    return unsupported_width("argmax_confusion", "ldc", ldc);
  UDASEG_LAUNCH_CHECK("argmax_confusion launch");
  return UDASEG_OK;
}

extern "C" int udaseg_gap_splits(int hw) {
  int s = GAP_SPLITS;
  if (s > hw) s = hw;
  return s < 1 ? 1 : s;
}

extern "C" int udaseg_gap_linear_sigmoid_fwd(const float* z, const float* w, const float* b, float* partial, float* pooled,
                                             float* p, int n, int hw, int c, void* stream) {
  UDASEG_CHECK_ARG(z && w && b && partial && pooled && p, "gap_linear_sigmoid_fwd: NULL pointer");
  UDASEG_CHECK_ARG(n > 0 && hw > 0 && c > 0 && c % 4 == 0, "gap_linear_sigmoid_fwd: bad shape");
  hipStream_t st = as_stream(stream);
  const int splits = udaseg_gap_splits(hw);
  const int bs = (c / 4) < 256 ? (((c / 4) + 63) / 64) * 64 : 256;
  hipLaunchKernelGGL(gap_partial_kernel, dim3(splits, n), dim3(bs), 0, st, (const f32x4*)z, (f32x4*)partial, hw, c / 4, splits);
  UDASEG_LAUNCH_CHECK("gap_partial launch");
  hipLaunchKernelGGL(gap_linear_sigmoid_kernel, dim3(n), dim3(256), 0, st, partial, w, b, pooled, p, hw, c, splits, 1);
  UDASEG_LAUNCH_CHECK("gap_linear_sigmoid launch");
  return UDASEG_OK;
}

extern "C" int udaseg_gap_linear_sigmoid_bwd(const float* dp, const float* p, const float* pooled, const float* w, float* dz,
                                             float* dw, float* db, int n, int hw, int c, int accumulate_param, void* stream) {
  UDASEG_CHECK_ARG(dp && p && pooled && w && dz && dw && db, "gap_linear_sigmoid_bwd: NULL pointer");
  UDASEG_CHECK_ARG(n > 0 && hw > 0 && c > 0 && c % 4 == 0, "gap_linear_sigmoid_bwd: bad shape");
  hipStream_t st = as_stream(stream);
  const int64_t total = (int64_t)n * hw * (c / 4);
  const int grid = capped_grid(total, 512, 2048);
  hipLaunchKernelGGL(gap_bwd_broadcast_kernel, dim3(grid), dim3(256), 0, st, dp, p, (const f32x4*)w, (f32x4*)dz, n, hw, c / 4, 1);
  UDASEG_LAUNCH_CHECK("gap_bwd_broadcast launch");
  hipLaunchKernelGGL(gap_bwd_param_kernel, dim3((c + 255) / 256), dim3(256), 0, st, dp, p, pooled, dw, db, n, c, accumulate_param, 1);
  UDASEG_LAUNCH_CHECK("gap_bwd_param launch");
  return UDASEG_OK;
}

// dtype-independent stages of the tail, for the bf16 path (its pooling partials / broadcast live in elem_bf16.hip)
extern "C" int udaseg_gap_finish(const float* partial, const float* w, const float* b, float* pooled, float* p, int n, int hw,
                                 int c, void* stream) {
  UDASEG_CHECK_ARG(partial && w && b && pooled && p && n > 0 && hw > 0 && c > 0, "gap_finish: bad arguments");
  hipLaunchKernelGGL(gap_linear_sigmoid_kernel, dim3(n), dim3(256), 0, as_stream(stream), partial, w, b, pooled, p, hw, c,
                     udaseg_gap_splits(hw), 1);
  UDASEG_LAUNCH_CHECK("gap_finish launch");
  return UDASEG_OK;
}

extern "C" int udaseg_gap_bwd_param(const float* dp, const float* p, const float* pooled, float* dw, float* db, int n, int c,
                                    int accumulate_param, void* stream) {
  UDASEG_CHECK_ARG(dp && p && pooled && dw && db && n > 0 && c > 0, "gap_bwd_param: bad arguments");
  hipLaunchKernelGGL(gap_bwd_param_kernel, dim3((c + 255) / 256), dim3(256), 0, as_stream(stream), dp, p, pooled, dw, db, n, c,
                     accumulate_param, 1);
  UDASEG_LAUNCH_CHECK("gap_bwd_param launch");
  return UDASEG_OK;
}

extern "C" int udaseg_bce_logits_fwd(const float* x, int n, float label, float weight, float* loss, int accumulate,
                                     void* stream) {
  UDASEG_CHECK_ARG(x && loss && n > 0, "bce_logits_fwd: bad arguments");
  hipLaunchKernelGGL(bce_fwd_kernel, dim3(1), dim3(64), 0, as_stream(stream), x, n, label, weight, loss, accumulate);
  UDASEG_LAUNCH_CHECK("bce_fwd launch");
  return UDASEG_OK;
}

extern "C" int udaseg_bce_logits_bwd(const float* x, int n, float label, float weight, const float* grad_out, float* dx,
                                     int accumulate, void* stream) {
  UDASEG_CHECK_ARG(x && dx && n > 0, "bce_logits_bwd: bad arguments");
  hipLaunchKernelGGL(bce_bwd_kernel, dim3((n + 255) / 256), dim3(256), 0, as_stream(stream), x, n, label, weight, grad_out, dx,
                     accumulate);
  UDASEG_LAUNCH_CHECK("bce_bwd launch");
  return UDASEG_OK;
}

// ---- feature-level discriminator tail: Conv2d(c, 1, 1) -> AdaptiveAvgPool2d(1) (reference src/models/uda.py:22-23).
// The two are linear, so mean_hw(w.x + b) = w.mean_hw(x) + b: same kernels as the image-level tail, no sigmoid.
extern "C" int udaseg_gap_linear_fwd(const float* z, const float* w, const float* b, float* partial, float* pooled, float* logit,
                                     int n, int hw, int c, void* stream) {
  UDASEG_CHECK_ARG(z && w && b && partial && pooled && logit, "gap_linear_fwd: NULL pointer");
  UDASEG_CHECK_ARG(n > 0 && hw > 0 && c > 0 && c % 4 == 0, "gap_linear_fwd: bad shape");
  hipStream_t st = as_stream(stream);
  const int splits = udaseg_gap_splits(hw);
  const int bs = (c / 4) < 256 ? (((c / 4) + 63) / 64) * 64 : 256;
  hipLaunchKernelGGL(gap_partial_kernel, dim3(splits, n), dim3(bs), 0, st, (const f32x4*)z, (f32x4*)partial, hw, c / 4, splits);
  UDASEG_LAUNCH_CHECK("gap_partial launch");
  hipLaunchKernelGGL(gap_linear_sigmoid_kernel, dim3(n), dim3(256), 0, st, partial, w, b, pooled, logit, hw, c, splits, 0);
  UDASEG_LAUNCH_CHECK("gap_linear launch");
  return UDASEG_OK;
}

extern "C" int udaseg_gap_linear_bwd(const float* dlogit, const float* pooled, const float* w, float* dz, float* dw, float* db,
                                     int n, int hw, int c, int accumulate_param, void* stream) {
  UDASEG_CHECK_ARG(dlogit && pooled && w && dz && dw && db, "gap_linear_bwd: NULL pointer");
  UDASEG_CHECK_ARG(n > 0 && hw > 0 && c > 0 && c % 4 == 0, "gap_linear_bwd: bad shape");
  hipStream_t st = as_stream(stream);
  const int64_t total = (int64_t)n * hw * (c / 4);
  const int grid = capped_grid(total, 512, 2048);
  hipLaunchKernelGGL(gap_bwd_broadcast_kernel, dim3(grid), dim3(256), 0, st, dlogit, (const float*)nullptr, (const f32x4*)w,
                     (f32x4*)dz, n, hw, c / 4, 0);
  UDASEG_LAUNCH_CHECK("gap_bwd_broadcast launch");
  hipLaunchKernelGGL(gap_bwd_param_kernel, dim3((c + 255) / 256), dim3(256), 0, st, dlogit, (const float*)nullptr, pooled, dw, db,
                     n, c, accumulate_param, 0);
  UDASEG_LAUNCH_CHECK("gap_bwd_param launch");
  return UDASEG_OK;
}

extern "C" int udaseg_bce_logits_target_fwd(const float* x, const float* target, int n, float weight, float* loss, int accumulate,
                                            void* stream) {
  UDASEG_CHECK_ARG(x && target && loss && n > 0, "bce_logits_target_fwd: bad arguments");
  hipLaunchKernelGGL(bce_target_fwd_kernel, dim3(1), dim3(64), 0, as_stream(stream), x, target, n, weight, loss, accumulate);
  UDASEG_LAUNCH_CHECK("bce_target_fwd launch");
  return UDASEG_OK;
}

extern "C" int udaseg_bce_logits_target_bwd(const float* x, const float* target, int n, float weight, const float* grad_out,
                                            float* dx, int accumulate, void* stream) {
  UDASEG_CHECK_ARG(x && target && dx && n > 0, "bce_logits_target_bwd: bad arguments");
  hipLaunchKernelGGL(bce_target_bwd_kernel, dim3((n + 255) / 256), dim3(256), 0, as_stream(stream), x, target, n, weight, grad_out,
                     dx, accumulate);
  UDASEG_LAUNCH_CHECK("bce_target_bwd launch");
  return UDASEG_OK;
}

// ---- cross entropy with options (class weights / ignore_index / label smoothing / reductions) ---------------------------------
static int check_ce_opt(const char* who, const void* logits, const void* target, int64_t pixels, int classes, int ldc, int maxldc,
                        float eps) {
  UDASEG_CHECK_ARG(logits && target, "%s: NULL pointer", who);
  UDASEG_CHECK_ARG(pixels > 0 && classes > 0 && classes <= ldc && ldc % 4 == 0 && ldc <= maxldc,
                   "%s: need 0 < classes <= ldc <= %d, ldc %% 4 == 0 (classes=%d ldc=%d)", who, maxldc, classes, ldc);
  UDASEG_CHECK_ARG(eps >= 0.f && eps <= 1.f, "%s: label smoothing must lie in [0, 1], got %g", who, (double)eps);
  return UDASEG_OK;
}

extern "C" int udaseg_ce_target_stats(const int64_t* target, const float* weight, int64_t pixels, int classes, int has_ignore,
                                      int64_t ignore_index, double* partials, double* denom, int64_t* stats, void* stream) {
  UDASEG_CHECK_ARG(target && partials && denom && stats, "ce_target_stats: NULL pointer");
  UDASEG_CHECK_ARG(pixels > 0 && classes > 0 && classes <= CE_MAXC, "ce_target_stats: need 0 < classes <= %d (classes=%d)", CE_MAXC,
                   classes);
  hipStream_t st = as_stream(stream);
  const int grid = capped_grid(pixels, 256, CE_BLOCKS);
  hipLaunchKernelGGL(ce_target_stats_kernel, dim3(grid), dim3(256), 0, st, target, weight, pixels, classes, has_ignore, ignore_index,
                     partials);
  UDASEG_LAUNCH_CHECK("ce_target_stats launch");
  return launch_rows_finish(4, partials, grid, denom, stats, st, "ce_target_stats_finish launch");
}

extern "C" int udaseg_ce_opt_fwd_bwd(const float* logits, const int64_t* target, const float* weight, int64_t pixels, int classes,
                                     int ldc, int has_ignore, int64_t ignore_index, float eps, int mean, const double* denom,
                                     double* partials, float* loss, float* dlogits, float* colsum_partials, float* colsum,
                                     void* stream) {
  int rc = check_ce_opt("ce_opt_fwd_bwd", logits, target, pixels, classes, ldc, 32, eps);
  if (rc) return rc;
  UDASEG_CHECK_ARG(partials && loss && dlogits, "ce_opt_fwd_bwd: NULL pointer");
  UDASEG_CHECK_ARG(!mean || denom, "ce_opt_fwd_bwd: the 'mean' reduction needs the denominator of udaseg_ce_target_stats");
  UDASEG_CHECK_ARG((colsum == nullptr) == (colsum_partials == nullptr), "ce_opt_fwd_bwd: colsum and colsum_partials come together");
  hipStream_t st = as_stream(stream);
  const int grid = capped_grid(pixels, 256, CE_BLOCKS);
  const double* dn = mean ? denom : nullptr;
  if (!dispatch_width<8>(ldc / 4, [&](auto w) {
        constexpr int W = decltype(w)::value;
        if (eps != 0.f)
          hipLaunchKernelGGL((ce_opt_fwd_bwd_kernel<W, true>), dim3(grid), dim3(256), 0, st, (const f32x4*)logits, target, weight,
                             pixels, classes, has_ignore, ignore_index, eps, dn, partials, (f32x4*)dlogits, colsum_partials);
        else
          hipLaunchKernelGGL((ce_opt_fwd_bwd_kernel<W, false>), dim3(grid), dim3(256), 0, st, (const f32x4*)logits, target, weight,
                             pixels, classes, has_ignore, ignore_index, eps, dn, partials, (f32x4*)dlogits, colsum_partials);
      }))
    return unsupported_width("ce_opt_fwd_bwd", "ldc", ldc);
  UDASEG_LAUNCH_CHECK("ce_opt_fwd_bwd launch");
  rc = launch_loss_finish(partials, grid, 1.0, dn, loss, 0, st, "ce_opt_finish launch");
  return rc || !colsum ? rc : launch_colsum_finish(colsum_partials, grid, ldc, colsum, 0, st);
}

extern "C" int udaseg_ce_opt_fwd(const float* logits, const int64_t* target, const float* weight, int64_t pixels, int classes,
                                 int ldc, int has_ignore, int64_t ignore_index, float eps, int mean, const double* denom, float* lse,
                                 double* partials, float* loss, float* loss_px, void* stream) {
  int rc = check_ce_opt("ce_opt_fwd", logits, target, pixels, classes, ldc, CE_MAXC, eps);
  if (rc) return rc;
  UDASEG_CHECK_ARG(lse && partials && (loss || loss_px), "ce_opt_fwd: NULL pointer");
  UDASEG_CHECK_ARG(!mean || denom, "ce_opt_fwd: the 'mean' reduction needs the denominator of udaseg_ce_target_stats");
  hipStream_t st = as_stream(stream);
  const int grid = capped_grid(pixels, 256, CE_BLOCKS);
  if (!dispatch_width<16>(ldc / 4, [&](auto w) {
        constexpr int W = decltype(w)::value;
        if (eps != 0.f)
          hipLaunchKernelGGL((ce_opt_fwd_kernel<W, true>), dim3(grid), dim3(256), 0, st, (const f32x4*)logits, target, weight, pixels,
                             classes, has_ignore, ignore_index, eps, lse, loss_px, partials);
        else
          hipLaunchKernelGGL((ce_opt_fwd_kernel<W, false>), dim3(grid), dim3(256), 0, st, (const f32x4*)logits, target, weight, pixels,
                             classes, has_ignore, ignore_index, eps, lse, loss_px, partials);
      }))
    return unsupported_width("ce_opt_fwd", "ldc", ldc);
  UDASEG_LAUNCH_CHECK("ce_opt_fwd launch");
  return loss ? launch_loss_finish(partials, grid, 1.0, mean ? denom : nullptr, loss, 0, st, "ce_opt_finish launch") : UDASEG_OK;
}

extern "C" int udaseg_ce_opt_bwd(const float* logits, const int64_t* target, const float* weight, const float* lse,
                                 const float* grad_out, const float* grad_px, int64_t pixels, int classes, int ldc, int has_ignore,
                                 int64_t ignore_index, float eps, int mean, const double* denom, float* dlogits,
                                 float* colsum_partials, float* colsum, void* stream) {
  int rc = check_ce_opt("ce_opt_bwd", logits, target, pixels, classes, ldc, CE_MAXC, eps);
  if (rc) return rc;
  UDASEG_CHECK_ARG(lse && dlogits, "ce_opt_bwd: NULL pointer");
  UDASEG_CHECK_ARG(!mean || denom, "ce_opt_bwd: the 'mean' reduction needs the denominator of udaseg_ce_target_stats");
  UDASEG_CHECK_ARG((colsum == nullptr) == (colsum_partials == nullptr), "ce_opt_bwd: colsum and colsum_partials come together");
  UDASEG_CHECK_ARG(colsum == nullptr || ldc <= 32, "ce_opt_bwd: fused column sums need ldc <= 32");
  hipStream_t st = as_stream(stream);
  const double* dn = mean ? denom : nullptr;
  const int grid = capped_grid(pixels, 256, ldc <= 32 ? CE_BLOCKS : CE_SIMPLE_BLOCKS);
  if (!dispatch_width<16>(ldc / 4, [&](auto w) {
        constexpr int W = decltype(w)::value;
        constexpr bool TILED = W <= 8;
        if (eps != 0.f)
          hipLaunchKernelGGL((ce_opt_bwd_kernel<W, true, TILED>), dim3(grid), dim3(256), 0, st, (const f32x4*)logits, target, weight,
                             lse, grad_out, grad_px, pixels, classes, has_ignore, ignore_index, eps, dn, (f32x4*)dlogits,
                             colsum_partials);
        else
          hipLaunchKernelGGL((ce_opt_bwd_kernel<W, false, TILED>), dim3(grid), dim3(256), 0, st, (const f32x4*)logits, target, weight,
                             lse, grad_out, grad_px, pixels, classes, has_ignore, ignore_index, eps, dn, (f32x4*)dlogits,
                             colsum_partials);
      }))
    return unsupported_width("ce_opt_bwd", "ldc", ldc);
  UDASEG_LAUNCH_CHECK("ce_opt_bwd launch");
  return colsum ? launch_colsum_finish(colsum_partials, grid, ldc, colsum, 0, st) : UDASEG_OK;
}
