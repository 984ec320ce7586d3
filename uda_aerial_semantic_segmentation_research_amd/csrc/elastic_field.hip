// The elastic field pass of the labelled training augmentation ("Training augmentation", stage 4b): the
// smoothed displacement field of the samples on elastic distortion, float2 [n][h][w].  The training call (augment.hip) runs it
// in front of its source pass; udaseg_elastic_field_f32 is the pass alone, for tests and tools.
#include "aug_common.h"

namespace udaseg {

// G = separable Gaussian (radius R, reflect-101 at any distance) of the raw field (2 u0 - 1, 2 u1 - 1), u = the first two
// uniforms of Philox4x32-10 at counter (y w + x, 1, 0, 0) under the record's elastic key.  One kernel, no global intermediate:
// a block owns a 32 x 32 tile; the raw values of the tile and its R-wide halo go into one LDS plane ((32 + 2R)^2 float2), the
// horizontal pass writes a second plane ((32 + 2R) x 32 float2), the vertical pass goes to global.  At R = 18 the planes take
// 36 992 + 17 408 bytes, next to each other below the 64 KiB a block may have.  The halo is recomputed, not exchanged: a block
// evaluates (32 + 2R)^2 / 32^2 generator calls per output pixel, 4.5 at R = 18 (a Philox call is ~70 integer operations; the two
// filter passes cost 2 x (3.1 + 1) x (2R + 1) = 230 multiply-adds per pixel there and dominate).  A wider tile would recompute
// less but the two planes no longer fit side by side (64 x 32: 68 KiB).  Only samples on elastic pay for any of it.
__global__ __launch_bounds__(256) void elastic_field_kernel(const int32_t* __restrict__ table, int h, int w, TaWeights gw, int radius,
                                                            ta_f2* __restrict__ field) {
  __shared__ ta_f2 raw[TA_FS * TA_FS];
  __shared__ ta_f2 hp[TA_FS * TA_FT];
  __shared__ float wt[2 * TA_MAX_RADIUS + 1];
  const int ni = blockIdx.y;
  const int32_t* t = table + (size_t)ni * TA_WORDS;
  if (!((t[SA_W_FLAGS] & TA_DISTORT) && t[TA_W_DISTORT_KIND] == TA_ELASTIC)) return;      // block-uniform
  const uint32_t k0 = (uint32_t)t[TA_W_ELASTIC_KEY], k1 = (uint32_t)t[TA_W_ELASTIC_KEY + 1];
  const int taps = 2 * radius + 1, side = TA_FT + 2 * radius;
  if ((int)threadIdx.x < taps) wt[threadIdx.x] = gw.w[threadIdx.x];
  const int tiles_x = (w + TA_FT - 1) / TA_FT;
  const int ty0 = (blockIdx.x / tiles_x) * TA_FT, tx0 = (blockIdx.x % tiles_x) * TA_FT;
  for (int i = threadIdx.x; i < side * side; i += 256) {
    const int ly = i / side, lx = i - ly * side;
    const int y = reflect101(ty0 - radius + ly, h), x = reflect101(tx0 - radius + lx, w);
    uint32_t r[4];
    philox4x32_10((uint32_t)(y * w + x), 1u, 0u, 0u, k0, k1, r);
    raw[i] = ta_f2{2.f * sa_uniform(r[0]) - 1.f, 2.f * sa_uniform(r[1]) - 1.f};
  }
  __syncthreads();
  for (int i = threadIdx.x; i < side * TA_FT; i += 256) {        // horizontal: every row of the plane, the tile's 32 columns
    const int ly = i / TA_FT, lx = i - ly * TA_FT;
    const ta_f2* src = raw + ly * side + lx;
    ta_f2 acc = {0.f, 0.f};
    for (int k = 0; k < taps; ++k) acc += wt[k] * src[k];
    hp[i] = acc;
  }
  __syncthreads();
  const int lx = threadIdx.x & (TA_FT - 1);
  const int x = tx0 + lx;
  for (int ly = threadIdx.x / TA_FT; ly < TA_FT; ly += 256 / TA_FT) {   // vertical
    const int y = ty0 + ly;
    if (y >= h || x >= w) continue;
    const ta_f2* src = hp + ly * TA_FT + lx;
    ta_f2 acc = {0.f, 0.f};
    for (int k = 0; k < taps; ++k) acc += wt[k] * src[k * TA_FT];
    field[((size_t)ni * h + y) * w + x] = acc;
  }
}

void elastic_launch_field(const int32_t* table, int n, int h, int w, const float* gauss_weights, int radius, float* field,
                          hipStream_t st) {
  TaWeights gw;
  for (int i = 0; i < 2 * TA_MAX_RADIUS + 1; ++i) gw.w[i] = i < 2 * radius + 1 ? gauss_weights[i] : 0.f;
  const int tiles = cdiv(h, TA_FT) * cdiv(w, TA_FT);
  hipLaunchKernelGGL(elastic_field_kernel, dim3(tiles, n), dim3(256), 0, st, table, h, w, gw, radius, (ta_f2*)field);
}

}  // namespace udaseg

using namespace udaseg;

extern "C" int udaseg_elastic_field_f32(const int32_t* table, int n, int h, int w, const float* gauss_weights, int radius,
                                        float* field, void* stream) {
  UDASEG_CHECK_ARG(table && field && gauss_weights && n > 0 && h > 0 && w > 0, "elastic_field_f32: bad arguments");
  UDASEG_CHECK_ARG(radius >= 0 && radius <= TA_MAX_RADIUS, "elastic_field_f32: radius must be 0..%d", TA_MAX_RADIUS);
  UDASEG_CHECK_ARG((int64_t)h * w < (1LL << 30) && n <= 65535, "elastic_field_f32: batch too large");
  UDASEG_CHECK_ARG(((uintptr_t)field & 7) == 0, "elastic_field_f32: the field must be 8-byte aligned");
  elastic_launch_field(table, n, h, w, gauss_weights, radius, field, as_stream(stream));
  UDASEG_LAUNCH_CHECK("elastic_field launch");
  return UDASEG_OK;
}
