// What a label map is, stated once (window.hip, boundary.hip, regions.hip, superpixels.hip, render.hip): [n][h][w] labels as uint8,
// or as int64 with every value outside [0, 255] read as 255; a storage flag says which, and a has_ignore / ignore_index pair names
// the void label.  Here are the one reader, the host-side rules of such an argument list -- each returns UDASEG_OK, or
// UDASEG_E_BADARG with the message set, the shape of scores_common.h's scores_args_ok:
//   if (int rc = map_storage_ok(who, "labels_i64", labels_i64)) return rc;
// -- and the dispatcher from runtime flags to the bool template parameters of the kernels.  An entry point calls a rule only
// where that rule is its own, in the order of its refusals, and adds its extra rules (a radius, a class count, a side limit) itself.
#pragma once
#include <type_traits>

#include "common.h"

namespace udaseg {

// Pixel p of a label map, uint8 or int64: an int64 value outside [0, 255] reads as 255.
template <bool I64>
__device__ __forceinline__ int label_at(const void* __restrict__ img, int64_t p) {
  if (I64) {
    const long long v = reinterpret_cast<const long long*>(img)[p];
    return (v < 0 || v > 255) ? 255 : (int)v;
  }
  return reinterpret_cast<const uint8_t*>(img)[p];
}

// the storage flag; `name` is what the entry point calls it
static inline int map_storage_ok(const char* who, const char* name, int i64) {
  UDASEG_CHECK_ARG(i64 == 0 || i64 == 1, "%s: %s must be 0 (uint8) or 1 (int64), got %d", who, name, i64);
  return UDASEG_OK;
}
// the batch: blockIdx.y is the image
static inline int map_batch_ok(const char* who, int n) {
  UDASEG_CHECK_ARG(n > 0 && n <= 65535, "%s: need 0 < n <= 65535 (n=%d)", who, n);
  return UDASEG_OK;
}
// the batch and the image extent: a pixel index of one image fits an int
static inline int map_extent_ok(const char* who, int n, int h, int w) {
  if (int rc = map_batch_ok(who, n)) return rc;
  UDASEG_CHECK_ARG(h >= 1 && w >= 1 && (int64_t)h * w < ((int64_t)1 << 31), "%s: need h, w >= 1 and h * w < 2^31 (h=%d w=%d)", who, h, w);
  return UDASEG_OK;
}
static inline int map_ignore_ok(const char* who, int has_ignore, int ignore_index) {
  UDASEG_CHECK_ARG(has_ignore == 0 || has_ignore == 1, "%s: has_ignore must be 0 or 1, got %d", who, has_ignore);
  UDASEG_CHECK_ARG(ignore_index >= 0 && ignore_index <= 255, "%s: ignore_index must lie in [0, 255] (ignore_index=%d)", who, ignore_index);
  return UDASEG_OK;
}
// one or two maps of the int64 storage start on 8 bytes; `what` names them in the message ("labels", "pred / truth")
static inline int map_aligned_ok(const char* who, const char* what, int i64, const void* a, const void* b = nullptr) {
  UDASEG_CHECK_ARG(!i64 || ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 7) == 0,
                   "%s: int64 %s must be 8-byte aligned", who, what);
  return UDASEG_OK;
}

// f(std::bool_constant<b0>{}, std::bool_constant<b1>{}, ...) for the runtime flags given, and what it returns: the boolean twin of
// scores_common.h's dispatch_width.  A launcher names the instantiation once: kernel<decltype(i64)::value, ...>.
template <typename F>
static inline auto dispatch_flags(F&& f) {
  return f();
}
template <typename F, typename... B>
static inline auto dispatch_flags(F&& f, bool b0, B... rest) {
  return b0 ? dispatch_flags([&](auto... t) { return f(std::true_type{}, t...); }, rest...)
            : dispatch_flags([&](auto... t) { return f(std::false_type{}, t...); }, rest...);
}

}  // namespace udaseg
