// Shared by every kernel that walks a padded NHWC buffer of per-pixel class scores: [pixels][ldc] fp32, classes <= ldc,
// ldc % 4 == 0, only channels < classes count (losses.hip, losses_seg.hip, advent.hip, distill.hip, curves.hip, pseudo.hip, predict.hip,
// proto.hip, proto_contrast.hip, ohem.hip; loss_reduce.h builds on it for what follows a loss kernel's row arithmetic).  Such a kernel is a
// template on its row width in f32x4 vectors -- LDC4 = ldc / 4 where the width is also the row stride, NV = cdiv(classes, 4) where
// ldc stays a runtime argument -- so here are the one width dispatcher, the one row reader and the one tie rule of the winner.
#pragma once
#include <limits.h>
#include <type_traits>
#include <utility>

#include "common.h"

namespace udaseg {

template <typename F, int... I>
static inline bool dispatch_width_seq(int width, F& f, std::integer_sequence<int, I...>) {
  return ((width == I + 1 && (f(std::integral_constant<int, I + 1>{}), true)) || ...);
}
// f(std::integral_constant<int, W>{}) for the W in 1..MAXW equal to width; false (and no call) when there is none.
template <int MAXW, typename F>
static inline bool dispatch_width(int width, F&& f) {
  return dispatch_width_seq(width, f, std::make_integer_sequence<int, MAXW>{});
}
static inline int unsupported_width(const char* who, const char* what, int value) {
  set_error("%s: unsupported %s %d", who, what, value);
  return UDASEG_E_UNSUPPORTED;
}

// The first NV vectors of one pixel's row, from a typed pointer (the LDC4 kernels: row = logits + p * LDC4) or a float one.
template <int NV>
__device__ __forceinline__ void load_row(const f32x4* row, f32x4 (&v)[NV]) {
#pragma unroll
  for (int q = 0; q < NV; ++q) v[q] = row[q];
}
template <int NV>
__device__ __forceinline__ void load_row(const float* row, f32x4 (&v)[NV]) {
#pragma unroll
  for (int q = 0; q < NV; ++q) v[q] = *reinterpret_cast<const f32x4*>(row + 4 * q);
}

// THE tie rule of PseudoLabeler, confusion_matrix, ScoreHistogram and predict_large, torch.argmax's: the first maximal channel
// below `classes`.  Channel 0 seeds the maximum whatever it holds; a NaN beyond channel 0 never compares greater and is stepped over.
// (The running maximum is a local and every score is read once: written on `best` directly the compiler kept branches where the
// kernels' own loops had selects, profiles/score_dispatch_refactor.txt.)
template <int NV>
__device__ __forceinline__ int first_max(const f32x4 (&v)[NV], int classes, float& best) {
  float m = -INFINITY;
  int am = 0;
#pragma unroll
  for (int q = 0; q < NV; ++q)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int c = 4 * q + e;
      const float x = v[q][e];
      if (c < classes && (c == 0 || x > m)) { m = x; am = c; }
    }
  best = m;
  return am;
}

// S = sum over c < classes of expf(z_c - m), m the row's maximum: channel c adds into partial sum c % 4 (four short chains), folded
// as (s0 + s1) + (s2 + s3).  The maximum's term is exactly 1, so S >= 1 whenever it is a number (pixel_conf below, ohem.hip).
template <int NV>
__device__ __forceinline__ float exp_sum(const f32x4 (&v)[NV], int classes, float m) {
  f32x4 s4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int q = 0; q < NV; ++q)
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (4 * q + e < classes) s4[e] += expf(v[q][e] - m);
  return (s4[0] + s4[1]) + (s4[2] + s4[3]);
}

// The winner of one pixel and its confidence, THE definition of pseudo.hip (its header comment states it) and of
// udaseg_conf_share (distill.hip): one function, so that a histogram, a labelling and a share cannot disagree.
struct PixelConf {
  int cls;        // c^
  float p;        // confidence
  bool finite;
};

template <int NV>
__device__ __forceinline__ PixelConf pixel_conf(const float* __restrict__ row, int classes, int probs) {
  f32x4 v[NV];
  load_row<NV>(row, v);
  float m;
  PixelConf r;
  r.cls = first_max<NV>(v, classes, m);
  if (probs) {
    bool nan = false;                                      // first_max steps over a NaN beyond channel 0
#pragma unroll
    for (int q = 0; q < NV; ++q)
#pragma unroll
      for (int e = 0; e < 4; ++e) nan |= 4 * q + e < classes && v[q][e] != v[q][e];
    r.p = m;
    r.finite = !nan && m >= 0.f && m <= 1.f;
  } else {
    r.p = 1.f / exp_sum<NV>(v, classes, m);
    r.finite = __builtin_isfinite(r.p);
  }
  return r;
}

// The shape of a score buffer whose winner is taken (at most 32 classes: the per-block class tables are that long).
// ld_name: what the entry point calls the row stride.
static inline bool scores_args_ok(const char* who, int64_t pixels, int classes, int ld, int max_ld = INT_MAX,
                                  const char* ld_name = "ldc") {
  if (pixels > 0 && classes > 0 && classes <= 32 && classes <= ld && ld % 4 == 0 && ld <= max_ld) return true;
  char limit[16] = "";
  if (max_ld != INT_MAX) snprintf(limit, sizeof limit, " <= %d", max_ld);
  set_error("%s: need 0 < pixels, 0 < classes <= 32, classes <= %s%s, %s %% 4 == 0 (pixels=%lld classes=%d %s=%d)", who, ld_name,
            limit, ld_name, (long long)pixels, classes, ld_name, ld);
  return false;
}

// The prototype table [classes][dim] and the feature rows [pixels][ldf] of proto.hip and proto_contrast.hip.
static inline bool proto_dims_ok(const char* who, int classes, int dim) {
  if (classes > 0 && classes <= 32 && dim >= 4 && dim <= 64 && dim % 4 == 0) return true;
  set_error("%s: need 0 < classes <= 32, 4 <= dim <= 64, dim %% 4 == 0 (classes=%d dim=%d)", who, classes, dim);
  return false;
}
static inline bool proto_feat_ok(const char* who, int64_t pixels, int classes, int dim, int ldf) {
  if (!proto_dims_ok(who, classes, dim)) return false;
  if (pixels > 0 && pixels < ((int64_t)1 << 31) && ldf >= dim && ldf % 4 == 0) return true;
  set_error("%s: need 0 < pixels < 2^31, dim <= ldf, ldf %% 4 == 0 (pixels=%lld dim=%d ldf=%d)", who, (long long)pixels, dim, ldf);
  return false;
}

// batch images of pix_per_image pixels each (distill.hip, proto_contrast.hip): the product fits an int64
static inline bool image_grid_ok(const char* who, int batch, int64_t ppi) {
  if (batch > 0 && ppi > 0 && ppi <= INT64_MAX / batch) return true;
  set_error("%s: need batch > 0, pix_per_image > 0 (batch=%d pix_per_image=%lld)", who, batch, (long long)ppi);
  return false;
}

}  // namespace udaseg
