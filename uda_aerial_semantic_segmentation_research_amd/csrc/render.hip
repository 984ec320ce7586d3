// Rendering of label maps on the device: colour masks, overlays on a frame, error maps, outlines and per-image class counts in
// ONE pass (reference predict.py create_colored_mask / create_overlay / the np.unique block of test_model, train.py
// _log_predictions).  With torch this is table[labels.long()], a float blend, a clamp, a cast, four shifted compares and a
// bincount: a dozen passes over int64 / float intermediates.  Here a pixel costs its label (1 or 8 bytes), an optional truth
// label, 3 bytes of frame (or the 16-byte pixel of the model input) and 3 bytes written.
//
// The rule, per pixel of image n (include/udaseg.h states it in full; tests/_render_ref.py is its numpy mirror, bit for bit):
//   L   = the label, an int64 value outside [0, 255] read as 255;   c = table[L]  (uint8 [256][3], made on the host)
//   b   = the base pixel: a uint8 frame, or the de-normalised model input clip(rint(x * scale + shift), 0, 255) (fp32 multiply,
//         fp32 add, round half to even, NaN -> 0), or none
//   k   = 3 truth void | 2 truth == L | 1 L void (L >= classes) | 0 otherwise          (first match wins; 0 / 1 without truth)
//   out = (b * (256 - a[k]) + c * a[k] + 128) >> 8 per channel (integers), c without a base; outline colour where the label
//         differs from a 4-neighbour inside the same image
//   counts[n][L] += 1;  agreement[n][agree, differ, truth void] += 1
//
// Shape.  blockIdx.y is the image, so a block's 256-bin LDS histogram belongs to one image and is flushed with one 64-bit
// global atomic per non-empty bin.  A lane takes a group of four consecutive pixels of its image: one 32-bit load of four uint8
// labels, three 32-bit loads of the frame, three 32-bit stores.  H*W*3 is in general no multiple of 4 and a contiguous tensor
// may start at any byte, so whether an image's labels / frame / output can be moved in words is decided PER IMAGE AND OPERAND
// from the image's own start address (uniform over the block); the others, and the last group of an image whose H*W is no
// multiple of four, move bytes.  The table sits in LDS as 256 packed words (one ds_read_b32 per pixel).  The outline reads the
// rows above and below straight from memory: they were, or are about to be, read by a neighbouring lane or block and hit cache
// (one word each for uint8 labels when the width is a multiple of four, label by label otherwise).
// The kernel is templated over (int64 labels, base kind, outline, counts, truth): the colour-mask instantiation carries no
// blend, no neighbour loads and no atomics.
#include "label_maps.h"

namespace udaseg {

constexpr int RD_THREADS = 256;
static_assert(RD_THREADS == 64 * 4, "BlockCounts<K>: four waves a block");
constexpr int RD_MAX_BLOCKS = 2048;
constexpr int RD_GROUPS_PER_THREAD = 2;

struct RenderArgs {
  const void* labels;
  const void* truth;
  const void* base;
  const uint8_t* table;
  uint8_t* out;
  unsigned long long* counts;
  unsigned long long* agreement;
  int h, w, classes, has_ignore, ignore_index;
  int a0, a1, a2, a3;
  float sc0, sc1, sc2, sh0, sh1, sh2;
  unsigned int outline;          // r | g << 8 | b << 16
};

// clip(rint(x * scale + shift), 0, 255): two separately rounded fp32 operations (no fused multiply-add: numpy has none), NaN -> 0
__device__ __forceinline__ unsigned int denorm_level(float x, float scale, float shift) {
  float v = rintf(__fadd_rn(__fmul_rn(x, scale), shift));
  if (!(v >= 0.f)) v = 0.f;
  if (v > 255.f) v = 255.f;
  return (unsigned int)v;
}

__device__ __forceinline__ unsigned int blend_px(unsigned int b, unsigned int c, unsigned int a) {
  const unsigned int ia = 256u - a;
  const unsigned int r = ((b & 255u) * ia + (c & 255u) * a + 128u) >> 8;
  const unsigned int g = (((b >> 8) & 255u) * ia + ((c >> 8) & 255u) * a + 128u) >> 8;
  const unsigned int bl = (((b >> 16) & 255u) * ia + ((c >> 16) & 255u) * a + 128u) >> 8;
  return r | (g << 8) | (bl << 16);
}

// BASE: UDASEG_RENDER_BASE_*.  Pixels are held as packed words r | g << 8 | b << 16.
template <bool I64, int BASE, bool OUTLINE, bool COUNTS, bool TRUTH>
__global__ __launch_bounds__(RD_THREADS) void render_kernel(RenderArgs A) {
  __shared__ unsigned int tab[256];
  __shared__ unsigned int hist[COUNTS ? 256 : 1];
  __shared__ BlockCounts<3>::Slots agr;
  const int tid = threadIdx.x;
  const int n = blockIdx.y;
  const int w = A.w, h = A.h, classes = A.classes;
  const int64_t HW = (int64_t)h * w;
  tab[tid] = (unsigned int)A.table[3 * tid] | ((unsigned int)A.table[3 * tid + 1] << 8) | ((unsigned int)A.table[3 * tid + 2] << 16);
  if (COUNTS) hist[tid] = 0;
  __syncthreads();

  const uint8_t* lab_img = reinterpret_cast<const uint8_t*>(A.labels) + (size_t)n * HW * (I64 ? 8 : 1);
  const uint8_t* tru_img = TRUTH ? reinterpret_cast<const uint8_t*>(A.truth) + (size_t)n * HW * (I64 ? 8 : 1) : nullptr;
  const uint8_t* base_img = BASE == UDASEG_RENDER_BASE_NONE ? nullptr
                            : reinterpret_cast<const uint8_t*>(A.base) + (size_t)n * HW * (BASE == UDASEG_RENDER_BASE_U8 ? 3 : 16);
  uint8_t* out_img = A.out + (size_t)n * HW * 3;
  const bool lab_vec = !I64 && (reinterpret_cast<uintptr_t>(lab_img) & 3) == 0;
  const bool tru_vec = TRUTH && !I64 && (reinterpret_cast<uintptr_t>(tru_img) & 3) == 0;
  const bool base_vec = BASE == UDASEG_RENDER_BASE_U8 && (reinterpret_cast<uintptr_t>(base_img) & 3) == 0;
  const bool out_vec = (reinterpret_cast<uintptr_t>(out_img) & 3) == 0;

  unsigned int ev[3] = {0, 0, 0};                              // agree, differ, truth void
  const int64_t groups = (HW + 3) >> 2;
  for (int64_t g = (int64_t)blockIdx.x * RD_THREADS + tid; g < groups; g += (int64_t)gridDim.x * RD_THREADS) {
    const int64_t p0 = 4 * g;
    const int cnt = HW - p0 >= 4 ? 4 : (int)(HW - p0);       // pixels p0 .. p0 + cnt - 1 exist; every access below stays inside them
    const bool full = cnt == 4;

    int L[4];
    if (!I64 && lab_vec && full) {
      const unsigned int v = *reinterpret_cast<const unsigned int*>(lab_img + p0);
#pragma unroll
      for (int e = 0; e < 4; ++e) L[e] = (int)((v >> (8 * e)) & 255u);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) L[e] = e < cnt ? label_at<I64>(lab_img, p0 + e) : 0;
    }

    int k[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) k[e] = L[e] >= classes ? 1 : 0;
    if (TRUTH) {
      int T[4];
      bool tv[4];
      if (I64) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const long long v = e < cnt ? reinterpret_cast<const long long*>(tru_img)[p0 + e] : 0;
          T[e] = (v < 0 || v > 255) ? 255 : (int)v;
          tv[e] = (A.has_ignore && v == (long long)A.ignore_index) || T[e] >= classes;
        }
      } else {
        if (tru_vec && full) {
          const unsigned int v = *reinterpret_cast<const unsigned int*>(tru_img + p0);
#pragma unroll
          for (int e = 0; e < 4; ++e) T[e] = (int)((v >> (8 * e)) & 255u);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) T[e] = e < cnt ? (int)tru_img[p0 + e] : 0;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) tv[e] = (A.has_ignore && T[e] == A.ignore_index) || T[e] >= classes;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (e < cnt) {
          if (tv[e]) {
            k[e] = 3;
            ++ev[2];
          } else if (T[e] == L[e]) {
            k[e] = 2;
            ++ev[0];
          } else {
            ++ev[1];
          }
        }
      }
    }

    if (COUNTS) {
      if (full && L[0] == L[1] && L[1] == L[2] && L[2] == L[3]) {      // the usual case inside a region: one LDS atomic for the four
        atomicAdd(&hist[L[0]], 4u);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (e < cnt) atomicAdd(&hist[L[e]], 1u);
      }
    }

    bool edge[4] = {false, false, false, false};
    if (OUTLINE) {
      int y = (int)(p0 / w);
      int x = (int)(p0 - (int64_t)y * w);
      if (!I64 && lab_vec && (w & 3) == 0) {
        // w, p0 and the image's start are multiples of four: the group lies in ONE row (and is full), and the four labels above
        // and below it are one aligned word each
        unsigned int up = 0, dn = 0;
        const bool has_up = y > 0, has_dn = y + 1 < h;
        if (has_up) up = *reinterpret_cast<const unsigned int*>(lab_img + p0 - w);
        if (has_dn) dn = *reinterpret_cast<const unsigned int*>(lab_img + p0 + w);
        const int left = x > 0 ? (int)lab_img[p0 - 1] : L[0];
        const int right = x + 4 < w ? (int)lab_img[p0 + 4] : L[3];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int l = L[e];
          bool d = (e > 0 ? L[e > 0 ? e - 1 : 0] : left) != l || (e < 3 ? L[e < 3 ? e + 1 : 3] : right) != l;
          d |= has_up && (int)((up >> (8 * e)) & 255u) != l;
          d |= has_dn && (int)((dn >> (8 * e)) & 255u) != l;
          edge[e] = d;
        }
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (e < cnt) {
            const int64_t p = p0 + e;
            const int l = L[e];
            bool d = false;
            if (x > 0) d |= (e > 0 ? L[e > 0 ? e - 1 : 0] : label_at<I64>(lab_img, p - 1)) != l;      // p - 1 is in this row
            if (x + 1 < w) d |= (e < 3 ? L[e < 3 ? e + 1 : 3] : label_at<I64>(lab_img, p + 1)) != l;  // p + 1 < HW, so e + 1 < cnt
            if (y > 0) d |= label_at<I64>(lab_img, p - w) != l;
            if (y + 1 < h) d |= label_at<I64>(lab_img, p + w) != l;
            edge[e] = d;
            if (++x == w) {
              x = 0;
              ++y;
            }
          }
        }
      }
    }

    unsigned int B[4] = {0u, 0u, 0u, 0u};
    if (BASE == UDASEG_RENDER_BASE_U8) {
      const uint8_t* src = base_img + 3 * p0;
      if (base_vec && full) {
        const unsigned int* s = reinterpret_cast<const unsigned int*>(src);
        const unsigned int w0 = s[0], w1 = s[1], w2 = s[2];
        B[0] = w0 & 0xffffffu;
        B[1] = (w0 >> 24) | ((w1 & 0xffffu) << 8);
        B[2] = (w1 >> 16) | ((w2 & 0xffu) << 16);
        B[3] = w2 >> 8;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (e < cnt)
            B[e] = (unsigned int)src[3 * e] | ((unsigned int)src[3 * e + 1] << 8) | ((unsigned int)src[3 * e + 2] << 16);
      }
    } else if (BASE == UDASEG_RENDER_BASE_F32) {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (e < cnt) {
          const f32x4 v = reinterpret_cast<const f32x4*>(base_img)[p0 + e];
          B[e] = denorm_level(v[0], A.sc0, A.sh0) | (denorm_level(v[1], A.sc1, A.sh1) << 8) | (denorm_level(v[2], A.sc2, A.sh2) << 16);
        }
    } else if (BASE == UDASEG_RENDER_BASE_BF16) {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (e < cnt) {
          const uint2 v = *reinterpret_cast<const uint2*>(base_img + 16 * (p0 + e));      // channels 0..2 of the 8 bf16
          const float x0 = __uint_as_float(v.x << 16), x1 = __uint_as_float(v.x & 0xffff0000u), x2 = __uint_as_float(v.y << 16);
          B[e] = denorm_level(x0, A.sc0, A.sh0) | (denorm_level(x1, A.sc1, A.sh1) << 8) | (denorm_level(x2, A.sc2, A.sh2) << 16);
        }
    }

    unsigned int O[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const unsigned int c = tab[L[e]];
      unsigned int o = c;
      if (BASE != UDASEG_RENDER_BASE_NONE) {
        const int a = k[e] == 0 ? A.a0 : (k[e] == 1 ? A.a1 : (k[e] == 2 ? A.a2 : A.a3));
        o = blend_px(B[e], c, (unsigned int)a);
      }
      if (OUTLINE && edge[e]) o = A.outline;
      O[e] = o;
    }

    uint8_t* dst = out_img + 3 * p0;
    if (out_vec && full) {
      unsigned int* d = reinterpret_cast<unsigned int*>(dst);
      d[0] = O[0] | (O[1] << 24);
      d[1] = (O[1] >> 8) | (O[2] << 16);
      d[2] = (O[2] >> 16) | (O[3] << 8);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (e < cnt) {
          dst[3 * e] = (uint8_t)(O[e] & 255u);
          dst[3 * e + 1] = (uint8_t)((O[e] >> 8) & 255u);
          dst[3 * e + 2] = (uint8_t)((O[e] >> 16) & 255u);
        }
    }
  }

  if (TRUTH && A.agreement) BlockCounts<3>::put(agr, ev);
  if (COUNTS || TRUTH) __syncthreads();                        // closes the histogram and the agreement slots
  if (COUNTS) {
    const unsigned int v = hist[tid];
    if (v) atomicAdd(&A.counts[(size_t)n * 256 + tid], (unsigned long long)v);
  }
  if (TRUTH && A.agreement) BlockCounts<3>::flush(agr, A.agreement + (size_t)n * 3);
}

}  // namespace udaseg

using namespace udaseg;

extern "C" int udaseg_render_u8(const void* labels, const void* truth, int labels_i64, const void* base, int base_kind,
                                const uint8_t* table, int n, int h, int w, int classes, int has_ignore, int ignore_index,
                                const int32_t* alpha, const float* denorm, int outline, uint8_t* out, int64_t* counts,
                                int64_t* agreement, void* stream) {
  UDASEG_CHECK_ARG(labels && table && out && alpha, "render_u8: NULL pointer (labels, table, out and alpha are required)");
  if (int rc = map_storage_ok("render_u8", "labels_i64", labels_i64)) return rc;
  UDASEG_CHECK_ARG(n > 0 && n <= 65535 && h > 0 && w > 0 && (int64_t)h * w < ((int64_t)1 << 31) - 4,
                   "render_u8: need 0 < n <= 65535, h, w > 0, h * w < 2^31 - 4 (n=%d h=%d w=%d)", n, h, w);
  UDASEG_CHECK_ARG(classes >= 1 && classes <= 256, "render_u8: need 1 <= classes <= 256 (classes=%d)", classes);
  UDASEG_CHECK_ARG(base_kind >= UDASEG_RENDER_BASE_NONE && base_kind <= UDASEG_RENDER_BASE_BF16 &&
                       (base != nullptr) == (base_kind != UDASEG_RENDER_BASE_NONE),
                   "render_u8: base_kind must be 0..3 and base given exactly when it is not 0 (base_kind=%d)", base_kind);
  UDASEG_CHECK_ARG(has_ignore == 0 || has_ignore == 1, "render_u8: has_ignore must be 0 or 1, got %d", has_ignore);
  for (int i = 0; i < 4; ++i)
    UDASEG_CHECK_ARG(alpha[i] >= 0 && alpha[i] <= 256, "render_u8: alpha[%d] = %d is outside [0, 256]", i, alpha[i]);
  UDASEG_CHECK_ARG(outline >= -1 && outline <= 0xffffff, "render_u8: outline must be -1 (none) or r | g << 8 | b << 16, got %d", outline);
  UDASEG_CHECK_ARG(!agreement || truth, "render_u8: agreement needs truth");
  if (int rc = map_aligned_ok("render_u8", "labels / truth", labels_i64, labels, truth)) return rc;
  const bool model_input = base_kind == UDASEG_RENDER_BASE_F32 || base_kind == UDASEG_RENDER_BASE_BF16;
  if (model_input) {
    UDASEG_CHECK_ARG(denorm, "render_u8: a model-input base needs the de-normalisation constants");
    UDASEG_CHECK_ARG((reinterpret_cast<uintptr_t>(base) & 15) == 0, "render_u8: a model-input base must be 16-byte aligned");
  }
  RenderArgs A;
  A.labels = labels;
  A.truth = truth;
  A.base = base;
  A.table = table;
  A.out = out;
  A.counts = reinterpret_cast<unsigned long long*>(counts);
  A.agreement = reinterpret_cast<unsigned long long*>(agreement);
  A.h = h;
  A.w = w;
  A.classes = classes;
  A.has_ignore = has_ignore;
  A.ignore_index = ignore_index;
  A.a0 = alpha[0];
  A.a1 = alpha[1];
  A.a2 = alpha[2];
  A.a3 = alpha[3];
  A.sc0 = model_input ? denorm[0] : 0.f;
  A.sc1 = model_input ? denorm[1] : 0.f;
  A.sc2 = model_input ? denorm[2] : 0.f;
  A.sh0 = model_input ? denorm[3] : 0.f;
  A.sh1 = model_input ? denorm[4] : 0.f;
  A.sh2 = model_input ? denorm[5] : 0.f;
  A.outline = outline < 0 ? 0u : (unsigned int)outline;
  const int64_t groups = ((int64_t)h * w + 3) >> 2;
  int64_t gx = cdiv64(groups, (int64_t)RD_THREADS * RD_GROUPS_PER_THREAD);
  const int64_t cap = RD_MAX_BLOCKS / n > 0 ? RD_MAX_BLOCKS / n : 1;
  if (gx > cap) gx = cap;
  const dim3 grid((unsigned int)gx, (unsigned int)n);
  hipStream_t st = as_stream(stream);
  const auto launch = [&](auto base) {
    dispatch_flags(
        [&](auto i64, auto ol, auto cn, auto tr) {
          hipLaunchKernelGGL((render_kernel<decltype(i64)::value, decltype(base)::value, decltype(ol)::value, decltype(cn)::value,
                                            decltype(tr)::value>),
                             grid, dim3(RD_THREADS), 0, st, A);
        },
        labels_i64 != 0, outline >= 0, counts != nullptr, truth != nullptr);
  };
  switch (base_kind) {
    case UDASEG_RENDER_BASE_NONE: launch(std::integral_constant<int, UDASEG_RENDER_BASE_NONE>{}); break;
    case UDASEG_RENDER_BASE_U8: launch(std::integral_constant<int, UDASEG_RENDER_BASE_U8>{}); break;
    case UDASEG_RENDER_BASE_F32: launch(std::integral_constant<int, UDASEG_RENDER_BASE_F32>{}); break;
    default: launch(std::integral_constant<int, UDASEG_RENDER_BASE_BF16>{}); break;
  }
  UDASEG_LAUNCH_CHECK("render_u8 launch");
  return UDASEG_OK;
}
