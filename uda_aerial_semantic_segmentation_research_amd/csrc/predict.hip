// Prediction (reference src/models/predict.py:70-130, plus tiled large-frame inference): the memory-bound passes around the
// eval forward of the Unet.
//   gather     one uint8 HWC frame -> [tiles*V][th][tw][cpad] model input: crop on the regular tile grid, numpy-"reflect"
//              padding where the tile overhangs the frame, one D4 view per image, A.Normalize -- one pass, the same arithmetic
//              as prepare_batch_kernel (data_prep.hip), so a code-0 crop inside the frame is bit-identical to prepare_batch.
//   blend      the batch's logits (fp32, padded NHWC) -> acc += w(ty,tx) * sum_v softmax(logits_v), wsum += w * V.  Pixel-
//              centric: one thread owns one frame pixel of the batch's bounding box and adds the batch's tiles that cover it
//              in raster tile order, the views in code order -- the order of the fp32 adds is the same for every batching,
//              with no atomics.  The inverse D4 map is applied in the read.
//   finish     probs = acc / wsum in place (padding lanes 0) and the argmax into int64 labels (first maximum on ties, as
//              argmax_confusion_kernel / torch.argmax); without wsum, the argmax of logits alone (predict_batch).
//   threshold  sigmoid(logits) > 0.5 as float 0/1 written NCHW (predict_mask's multi-class thresholding).
//
// Tile grid (one axis of length L, effective tile t, stride s): origin o_i = max(0, min(i*s, L - t)) for i = 0 .. n-1,
// n = 1 if L <= t else ceil((L - t) / s) + 1.  Tiles are numbered raster, row-major: k = i*cols + j.
#include "scores_common.h"

namespace udaseg {

__device__ __forceinline__ int grid_origin(int i, int s, int L, int t) { return max(0, min(i * s, L - t)); }

// numpy.pad(mode="reflect") index for i >= 0 (the tile origins are >= 0, so only the far edge is ever crossed)
__device__ __forceinline__ int reflect_index(int i, int L) {
  if (L == 1) return 0;
  const int period = 2 * (L - 1);
  i %= period;
  return i < L ? i : period - i;
}

// views: up to 8 D4 codes packed 4 bits each, ascending (code of view v = (packed >> 4v) & 7)
__device__ __forceinline__ int view_code(uint32_t packed, int v) { return (int)((packed >> (4 * v)) & 7u); }

template <bool BF16>
__global__ __launch_bounds__(256) void predict_gather_kernel(const uint8_t* __restrict__ img, int h, int w, int th, int tw, int cols,
                                                             int sy, int sx, int first, uint32_t codes, int nv, float m0, float m1,
                                                             float m2, float r0, float r1, float r2, void* __restrict__ out,
                                                             int cpad) {
  const int b = blockIdx.y;                                  // image of the batch = tile * nv + view
  const int k = first + b / nv;
  const int code = view_code(codes, b % nv);
  const int oy = grid_origin(k / cols, sy, h, th), ox = grid_origin(k % cols, sx, w, tw);
  const int tp = th * tw;
  for (int p = blockIdx.x * 256 + threadIdx.x; p < tp; p += gridDim.x * 256) {
    int y = p / tw, x = p - y * tw;
    // the view's pixel (y, x) is the tile's pixel fliph^b2(flipv^b1(transpose^b0)) -- data_prep.hip's convention
    if (code & 2) y = th - 1 - y;
    if (code & 4) x = tw - 1 - x;
    const int ty = (code & 1) ? x : y, tx = (code & 1) ? y : x;   // transposing codes need th == tw (checked by the caller)
    const int fy = reflect_index(oy + ty, h), fx = reflect_index(ox + tx, w);
    const uint8_t* src = img + ((size_t)fy * w + fx) * 3;
    // A.Normalize exactly as prepare_batch_kernel: (x - mean255) * inv_std255 in fp32, bf16 rounded once
    const float v0 = ((float)src[0] - m0) * r0;
    const float v1 = ((float)src[1] - m1) * r1;
    const float v2 = ((float)src[2] - m2) * r2;
    const size_t o = ((size_t)b * tp + p) * cpad;
    if (BF16) {
      typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));
      u16x8 v = {__builtin_bit_cast(unsigned short, (__bf16)v0), __builtin_bit_cast(unsigned short, (__bf16)v1),
                 __builtin_bit_cast(unsigned short, (__bf16)v2), 0, 0, 0, 0, 0};
      __bf16* dst = reinterpret_cast<__bf16*>(out) + o;
      *reinterpret_cast<u16x8*>(dst) = v;
      for (int c = 8; c < cpad; ++c) dst[c] = (__bf16)0.f;
    } else {
      float* dst = reinterpret_cast<float*>(out) + o;
      *reinterpret_cast<f32x4*>(dst) = f32x4{v0, v1, v2, 0.f};
      for (int c = 4; c < cpad; ++c) dst[c] = 0.f;
    }
  }
}

constexpr int BLEND_BX = 16, BLEND_BY = 16;      // square blocks: transposing views read 16-pixel runs down columns,
                                                 // the others along rows

template <int NV>
__global__ __launch_bounds__(BLEND_BX * BLEND_BY) void predict_blend_kernel(
    const float* __restrict__ logits, int ldc, int h, int w, int th, int tw, int rows, int cols, int sy, int sx, int first,
    int tiles, uint32_t codes, int nv, int classes, const float* __restrict__ wy, const float* __restrict__ wx,
    float* __restrict__ acc, int ldp, float* __restrict__ wsum, int y0, int x0, int y1, int x1) {
  const int x = x0 + blockIdx.x * BLEND_BX + threadIdx.x;
  const int y = y0 + blockIdx.y * BLEND_BY + threadIdx.y;
  if (x >= x1 || y >= y1) return;
  const size_t pix = (size_t)y * w + x;
  f32x4 a[NV];
  load_row<NV>(acc + pix * ldp, a);
  float ws = wsum[pix];
  bool touched = false;
  // candidate tile rows / columns: every i with o_i <= y < o_i + th lies in [ (y-th)/s , y/s + 1 ] (the +1 catches the flush
  // last tile, whose origin is pulled back below i*s); at most 3-4 per axis for overlap <= 0.5
  const int ilo = y >= th ? (y - th) / sy : 0, ihi = min(rows - 1, y / sy + 1);
  const int jlo = x >= tw ? (x - tw) / sx : 0, jhi = min(cols - 1, x / sx + 1);
  for (int i = ilo; i <= ihi; ++i) {
    const int oy = grid_origin(i, sy, h, th);
    if (y < oy || y >= oy + th) continue;
    for (int j = jlo; j <= jhi; ++j) {
      const int ox = grid_origin(j, sx, w, tw);
      if (x < ox || x >= ox + tw) continue;
      const int k = i * cols + j;
      if (k < first || k >= first + tiles) continue;
      const int ty = y - oy, tx = x - ox;
      f32x4 s[NV];
#pragma unroll
      for (int q = 0; q < NV; ++q) s[q] = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int v = 0; v < nv; ++v) {
        const int code = view_code(codes, v);
        // inverse D4: the model's pixel (yy, xx) of view `code` holds tile pixel (ty, tx)
        const int ay = (code & 1) ? tx : ty, ax = (code & 1) ? ty : tx;
        const int yy = (code & 2) ? th - 1 - ay : ay, xx = (code & 4) ? tw - 1 - ax : ax;
        const float* row = logits + ((((size_t)(k - first) * nv + v) * th + yy) * tw + xx) * ldc;
        f32x4 l[NV];
        load_row<NV>(row, l);
        float m = -INFINITY;
#pragma unroll
        for (int q = 0; q < NV; ++q)
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (4 * q + e < classes) m = fmaxf(m, l[q][e]);
        float sum = 0.f;
#pragma unroll
        for (int q = 0; q < NV; ++q)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float ex = 4 * q + e < classes ? expf(l[q][e] - m) : 0.f;   // padding lanes of the logits are ignored
            l[q][e] = ex;
            sum += ex;
          }
#pragma unroll
        for (int q = 0; q < NV; ++q)
#pragma unroll
          for (int e = 0; e < 4; ++e) s[q][e] += l[q][e] / sum;
      }
      const float wt = wy[ty] * wx[tx];
#pragma unroll
      for (int q = 0; q < NV; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) a[q][e] += wt * s[q][e];
      ws += wt * (float)nv;
      touched = true;
    }
  }
  if (!touched) return;
#pragma unroll
  for (int q = 0; q < NV; ++q) *reinterpret_cast<f32x4*>(acc + pix * ldp + 4 * q) = a[q];
  wsum[pix] = ws;
}

// The row is read, divided and written back in place, so its load stays written out here: with load_row the compiler no longer splits
// the pixel loop on `wsum`, and the kernel is 8 % slower at a 4000 x 6000 frame (profiles/score_dispatch_refactor.txt).
template <int NV>
__global__ __launch_bounds__(256) void predict_finish_kernel(float* __restrict__ probs, int ldc, const float* __restrict__ wsum,
                                                             int64_t pixels, int classes, int64_t* __restrict__ labels) {
  const int64_t T = (int64_t)gridDim.x * blockDim.x;
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < pixels; p += T) {
    float* row = probs + p * ldc;
    f32x4 v[NV];
#pragma unroll
    for (int q = 0; q < NV; ++q) v[q] = *reinterpret_cast<const f32x4*>(row + 4 * q);   // not load_row: see above
    if (wsum) {
      const float ws = wsum[p];
#pragma unroll
      for (int q = 0; q < NV; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) v[q][e] = 4 * q + e < classes ? v[q][e] / ws : 0.f;
    }
    float best;
    labels[p] = first_max<NV>(v, classes, best);
    if (wsum) {
#pragma unroll
      for (int q = 0; q < NV; ++q) *reinterpret_cast<f32x4*>(row + 4 * q) = v[q];
      for (int q = NV; q < ldc / 4; ++q) *reinterpret_cast<f32x4*>(row + 4 * q) = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  }
}

template <int NV>
__global__ __launch_bounds__(256) void predict_threshold_kernel(const float* __restrict__ logits, int ldc, int hw, int classes,
                                                                float* __restrict__ out) {
  const int ni = blockIdx.y;
  for (int p = blockIdx.x * 256 + threadIdx.x; p < hw; p += gridDim.x * 256) {
    const float* row = logits + ((size_t)ni * hw + p) * ldc;
    float* dst = out + (size_t)ni * classes * hw + p;
#pragma unroll
    for (int q = 0; q < NV; ++q) {
      const f32x4 l = *reinterpret_cast<const f32x4*>(row + 4 * q);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int c = 4 * q + e;
        if (c < classes) dst[(size_t)c * hw] = 1.f / (1.f + expf(-l[e])) > 0.5f ? 1.f : 0.f;   // (sigmoid(x) > 0.5).float()
      }
    }
  }
}

// ---- host side

static int grid_count(int L, int t, int s) { return L <= t ? 1 : (L - t + s - 1) / s + 1; }

static uint32_t pack_views(int views, int* nv) {
  uint32_t packed = 0;
  int n = 0;
  for (int c = 0; c < 8; ++c)
    if (views >> c & 1) packed |= (uint32_t)c << (4 * n++);
  *nv = n;
  return packed;
}

#define PREDICT_CHECK_GRID(what)                                                                                              \
  UDASEG_CHECK_ARG(h > 0 && w > 0 && (int64_t)h * w < (1LL << 31), what ": bad frame size %dx%d", h, w);                     \
  UDASEG_CHECK_ARG(th >= 32 && tw >= 32 && th % 32 == 0 && tw % 32 == 0, what ": tile sides must be positive multiples of "  \
                   "32, got %dx%d", th, tw);                                                                                   \
  UDASEG_CHECK_ARG(sy >= 1 && sx >= 1 && sy <= th && sx <= tw, what ": strides must lie in [1, tile]");                      \
  UDASEG_CHECK_ARG(rows == grid_count(h, th, sy) && cols == grid_count(w, tw, sx),                                           \
                   what ": rows x cols = %dx%d is not the tile grid of this frame (%dx%d)", rows, cols, grid_count(h, th, sy), \
                   grid_count(w, tw, sx));                                                                                     \
  UDASEG_CHECK_ARG(first >= 0 && tiles >= 1 && (int64_t)first + tiles <= (int64_t)rows * cols,                               \
                   what ": tiles [%d, %d) outside the grid of %d", first, first + tiles, rows * cols);                         \
  UDASEG_CHECK_ARG(views > 0 && views < 256, what ": views must be a non-empty bitmask of D4 codes 0..7");                   \
  UDASEG_CHECK_ARG(th == tw || (views & 0xAA) == 0, what ": transposing views (odd codes) need square tiles, got %dx%d", th,  \
                   tw)

}  // namespace udaseg

using namespace udaseg;

extern "C" int udaseg_predict_gather_u8(const uint8_t* image, int h, int w, int th, int tw, int rows, int cols, int sy, int sx,
                                        int first, int tiles, int views, const float* mean255, const float* inv_std255,
                                        void* out, int cpad, int out_bf16, void* stream) {
  UDASEG_CHECK_ARG(image && out && mean255 && inv_std255, "predict_gather_u8: bad arguments");
  PREDICT_CHECK_GRID("predict_gather_u8");
  UDASEG_CHECK_ARG(cpad >= (out_bf16 ? 8 : 4) && cpad % (out_bf16 ? 8 : 4) == 0, "predict_gather_u8: cpad must be a multiple "
                   "of %d", out_bf16 ? 8 : 4);
  int nv;
  const uint32_t codes = pack_views(views, &nv);
  const int tp = th * tw;
  const int gx = capped_grid(tp, 256, 256);
  hipStream_t st = as_stream(stream);
  if (out_bf16)
    hipLaunchKernelGGL(predict_gather_kernel<true>, dim3(gx, tiles * nv), dim3(256), 0, st, image, h, w, th, tw, cols, sy, sx,
                       first, codes, nv, mean255[0], mean255[1], mean255[2], inv_std255[0], inv_std255[1], inv_std255[2], out,
                       cpad);
  else
    hipLaunchKernelGGL(predict_gather_kernel<false>, dim3(gx, tiles * nv), dim3(256), 0, st, image, h, w, th, tw, cols, sy, sx,
                       first, codes, nv, mean255[0], mean255[1], mean255[2], inv_std255[0], inv_std255[1], inv_std255[2], out,
                       cpad);
  UDASEG_LAUNCH_CHECK("predict_gather launch");
  return UDASEG_OK;
}

extern "C" int udaseg_predict_blend(const float* logits, int ldc, int h, int w, int th, int tw, int rows, int cols, int sy, int sx,
                                    int first, int tiles, int views, int classes, const float* win_y, const float* win_x,
                                    float* acc, int ldp, float* wsum, void* stream) {
  UDASEG_CHECK_ARG(logits && win_y && win_x && acc && wsum, "predict_blend: bad arguments");
  PREDICT_CHECK_GRID("predict_blend");
  if (!scores_args_ok("predict_blend", (int64_t)h * w, classes, ldc)) return UDASEG_E_BADARG;
  if (!scores_args_ok("predict_blend", (int64_t)h * w, classes, ldp, INT_MAX, "ldp")) return UDASEG_E_BADARG;
  int nv;
  const uint32_t codes = pack_views(views, &nv);
  // the batch's bounding box inside the frame: its tile rows, and its tile columns when it lies in one row
  const int k0 = first, k1 = first + tiles - 1;
  const int i0 = k0 / cols, i1 = k1 / cols;
  const int y0 = std::max(0, std::min(i0 * sy, h - th)), y1 = std::min(h, std::max(0, std::min(i1 * sy, h - th)) + th);
  int x0 = 0, x1 = w;
  if (i0 == i1) {
    x0 = std::max(0, std::min((k0 % cols) * sx, w - tw));
    x1 = std::min(w, std::max(0, std::min((k1 % cols) * sx, w - tw)) + tw);
  }
  const dim3 grid(cdiv(x1 - x0, BLEND_BX), cdiv(y1 - y0, BLEND_BY));
  if (!dispatch_width<8>(cdiv(classes, 4), [&](auto nw) {
        hipLaunchKernelGGL(predict_blend_kernel<decltype(nw)::value>, grid, dim3(BLEND_BX, BLEND_BY), 0, as_stream(stream), logits,
                           ldc, h, w, th, tw, rows, cols, sy, sx, first, tiles, codes, nv, classes, win_y, win_x, acc, ldp, wsum, y0,
                           x0, y1, x1);
      }))
    return unsupported_width("predict_blend", "classes", classes);
  UDASEG_LAUNCH_CHECK("predict_blend launch");
  return UDASEG_OK;
}

extern "C" int udaseg_predict_finish(float* probs, const float* wsum, int64_t pixels, int classes, int ldc, int64_t* labels,
                                     void* stream) {
  UDASEG_CHECK_ARG(probs && labels, "predict_finish: bad arguments");
  if (!scores_args_ok("predict_finish", pixels, classes, ldc)) return UDASEG_E_BADARG;
  const int blocks = capped_grid(pixels, 256, 8192);
  if (!dispatch_width<8>(cdiv(classes, 4), [&](auto nw) {
        hipLaunchKernelGGL(predict_finish_kernel<decltype(nw)::value>, dim3(blocks), dim3(256), 0, as_stream(stream), probs, ldc, wsum,
                           pixels, classes, labels);
      }))
    return unsupported_width("predict_finish", "classes", classes);
  UDASEG_LAUNCH_CHECK("predict_finish launch");
  return UDASEG_OK;
}

extern "C" int udaseg_predict_threshold(const float* logits, int n, int hw, int classes, int ldc, float* out, void* stream) {
  UDASEG_CHECK_ARG(logits && out && n > 0 && hw > 0 && n < 65536, "predict_threshold: bad arguments");
  if (!scores_args_ok("predict_threshold", (int64_t)n * hw, classes, ldc)) return UDASEG_E_BADARG;
  const int gx = capped_grid(hw, 256, 1024);
  if (!dispatch_width<8>(cdiv(classes, 4), [&](auto nw) {
        hipLaunchKernelGGL(predict_threshold_kernel<decltype(nw)::value>, dim3(gx, n), dim3(256), 0, as_stream(stream), logits, ldc, hw,
                           classes, out);
      }))
    return unsupported_width("predict_threshold", "classes", classes);
  UDASEG_LAUNCH_CHECK("predict_threshold launch");
  return UDASEG_OK;
}
