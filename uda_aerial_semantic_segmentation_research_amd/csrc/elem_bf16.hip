// bf16-storage kernels that have no fp32 twin written over the same body (the twinned ones live in norm_act.hip and
// pool_resize.hip, once per operation over Vec16<BF>): the fp32 -> bf16 cast, the discriminator tail's pooling partials and
// gradient broadcast (fp32: losses.hip, which reduces and broadcasts quads in another shape), and the bf16 data-gradient weight
// packing (fp32: conv_wgrad.hip).  8 channels = one 16-byte vector per thread per step, arithmetic in fp32.
#include "vec16.h"

namespace udaseg {

__global__ void cast_f32_bf16_kernel(const f32x4* __restrict__ x, f32x4* __restrict__ y, int64_t n8) {
  const int64_t T = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += T) {
    const f32x4 a = x[2 * i], b = x[2 * i + 1];
    const Vec16<true> v = {{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]}};
    y[i] = v.raw();
  }
}

// ---------------------------------------------------------------------------------------- discriminator tail, bf16
__global__ void gap_partial_bf16_kernel(const f32x4* __restrict__ z, float* __restrict__ partial, int hw, int c8, int splits) {
  const int ni = blockIdx.y, s = blockIdx.x;
  const int per = (hw + splits - 1) / splits;
  const int p0 = s * per, p1 = min(hw, p0 + per);
  for (int q = threadIdx.x; q < c8; q += blockDim.x) {
    Vec16<true> acc = Vec16<true>::zero();
    for (int p = p0; p < p1; ++p) acc += Vec16<true>::from(z[((int64_t)ni * hw + p) * c8 + q]);
#pragma unroll
    for (int e = 0; e < 8; ++e) partial[((int64_t)ni * splits + s) * c8 * 8 + q * 8 + e] = acc.v[e];
  }
}

__global__ void gap_bwd_broadcast_bf16_kernel(const float* __restrict__ dp, const float* __restrict__ p, const float* __restrict__ w,
                                              f32x4* __restrict__ dz, int n, int hw, int c8) {
  const int64_t total = (int64_t)n * hw * c8;
  const int64_t T = (int64_t)gridDim.x * blockDim.x;
  const float inv = 1.f / (float)hw;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += T) {
    const int q = (int)(i % c8);
    const int ni = (int)(i / ((int64_t)hw * c8));
    const float pv = p[ni];
    const float dl = dp[ni] * pv * (1.f - pv) * inv;
    Vec16<true> v;
#pragma unroll
    for (int e = 0; e < 8; ++e) v.v[e] = w[q * 8 + e] * dl;
    dz[i] = v.raw();
  }
}

// weights: fp32 arena -> bf16 copy (same layout) happens through cast_f32_bf16; the dgrad packing [ci][taps][co] in bf16:
__global__ void pack_dgrad_batched_bf16_kernel(const float* __restrict__ arena, __bf16* __restrict__ packed,
                                               const int* __restrict__ table) {
  const int* e = table + 5 * blockIdx.y;
  const float* w = arena + e[0];
  __bf16* wt = packed + e[1];
  if ((e[2] | e[4]) & 3) {
    const int co = e[2], T = e[3], ci = e[4];
    const int total = co * T * ci;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
      const int o = i % co;
      const int r = i / co;
      const int t = r % T;
      const int c = r / T;
      wt[i] = (__bf16)w[(o * T + t) * ci + c];
    }
    return;
  }
  pack_dgrad_tiles<__bf16>(w, wt, e[2], e[3], e[4]);
}

}  // namespace udaseg

using namespace udaseg;

extern "C" int udaseg_cast_f32_to_bf16(const float* x, void* y, int64_t count, void* stream) {
  UDASEG_CHECK_ARG(x && y && count > 0 && count % 8 == 0, "cast_f32_to_bf16: count must be a positive multiple of 8");
  hipLaunchKernelGGL(cast_f32_bf16_kernel, dim3(grid_for(count / 8, 4)), dim3(256), 0, as_stream(stream), (const f32x4*)x,
                     (f32x4*)y, count / 8);
  UDASEG_LAUNCH_CHECK("cast_f32_to_bf16 launch");
  return UDASEG_OK;
}

extern "C" int udaseg_gap_partial_bf16(const void* z, float* partial, int n, int hw, int c, void* stream) {
  UDASEG_CHECK_ARG(z && partial && n > 0 && hw > 0 && c > 0 && c % 8 == 0, "gap_partial_bf16: bad arguments");
  const int splits = udaseg_gap_splits(hw);
  const int bs = (c / 8) < 256 ? (((c / 8) + 63) / 64) * 64 : 256;
  hipLaunchKernelGGL(gap_partial_bf16_kernel, dim3(splits, n), dim3(bs), 0, as_stream(stream), (const f32x4*)z, partial, hw,
                     c / 8, splits);
  UDASEG_LAUNCH_CHECK("gap_partial_bf16 launch");
  return UDASEG_OK;
}

extern "C" int udaseg_gap_bwd_broadcast_bf16(const float* dp, const float* p, const float* w, void* dz, int n, int hw, int c,
                                             void* stream) {
  UDASEG_CHECK_ARG(dp && p && w && dz && n > 0 && hw > 0 && c > 0 && c % 8 == 0, "gap_bwd_broadcast_bf16: bad arguments");
  const int64_t total = (int64_t)n * hw * (c / 8);
  hipLaunchKernelGGL(gap_bwd_broadcast_bf16_kernel, dim3(grid_for(total)), dim3(256), 0, as_stream(stream), dp, p, w,
                     (f32x4*)dz, n, hw, c / 8);
  UDASEG_LAUNCH_CHECK("gap_bwd_broadcast_bf16 launch");
  return UDASEG_OK;
}

extern "C" int udaseg_pack_dgrad_batched_bf16(const float* arena, void* packed, const int* table, int entries, void* stream) {
  UDASEG_CHECK_ARG(arena && packed && table && entries > 0, "pack_dgrad_batched_bf16: bad arguments");
  hipLaunchKernelGGL(pack_dgrad_batched_bf16_kernel, dim3(PACK_DGRAD_GRID_X, entries), dim3(256), 0, as_stream(stream), arena, (__bf16*)packed,
                     table);
  UDASEG_LAUNCH_CHECK("pack_dgrad_batched_bf16 launch");
  return UDASEG_OK;
}
