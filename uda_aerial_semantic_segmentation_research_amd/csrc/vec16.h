// One 16-byte vector of an NHWC tensor in either storage: 4 fp32 or 8 bf16 channels, widened to fp32 for arithmetic.
// The HBM-bound kernels of norm_act.hip, pool_resize.hip, bilinear.hip and elem_bf16.hip are written once over it and
// instantiated per storage; tensors travel as f32x4 (or void) pointers whatever they hold.
#pragma once
#include "common.h"

namespace udaseg {

template <bool BF>
struct Vec16 {
  static constexpr int N = BF ? 8 : 4;
  float v[N];
  // widen one raw vector (bf16 -> fp32 is exact)
  __device__ __forceinline__ static Vec16 from(const f32x4& raw) {
    Vec16 r;
    if constexpr (BF) {
      typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
      const bf16x8 h = __builtin_bit_cast(bf16x8, raw);
#pragma unroll
      for (int e = 0; e < 8; ++e) r.v[e] = (float)h[e];
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) r.v[e] = raw[e];
    }
    return r;
  }
  // narrow back to the storage (fp32 -> bf16 rounds to nearest even)
  __device__ __forceinline__ f32x4 raw() const {
    if constexpr (BF) {
      typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
      bf16x8 h;
#pragma unroll
      for (int e = 0; e < 8; ++e) h[e] = (__bf16)v[e];
      return __builtin_bit_cast(f32x4, h);
    } else {
      return f32x4{v[0], v[1], v[2], v[3]};
    }
  }
  __device__ __forceinline__ static Vec16 zero() {
    Vec16 r;
#pragma unroll
    for (int e = 0; e < N; ++e) r.v[e] = 0.f;
    return r;
  }
  // The same two through memory.  Their fp32 copies are written out, not routed through from() / raw(): with that extra level
  // of inlining the compiler fused other multiply-adds in bilinear.hip's fp32 kernels, and their results moved by an ulp.
  __device__ __forceinline__ static Vec16 load(const void* base, int64_t idx) {
    const f32x4 raw = static_cast<const f32x4*>(base)[idx];
    if constexpr (BF) {
      return from(raw);
    } else {
      Vec16 r;
#pragma unroll
      for (int e = 0; e < 4; ++e) r.v[e] = raw[e];
      return r;
    }
  }
  __device__ __forceinline__ void store(void* base, int64_t idx) const {
    if constexpr (BF) {
      static_cast<f32x4*>(base)[idx] = raw();
    } else {
      f32x4 raw;
#pragma unroll
      for (int e = 0; e < 4; ++e) raw[e] = v[e];
      static_cast<f32x4*>(base)[idx] = raw;
    }
  }
  __device__ __forceinline__ Vec16& operator+=(const Vec16& o) {
#pragma unroll
    for (int e = 0; e < N; ++e) v[e] += o.v[e];
    return *this;
  }
};

}  // namespace udaseg
