// Fused Adam over a flat fp32 arena (gfx950).  HBM-bound: 16 B read + 12 B written per parameter.
//
// Replaces torch.optim.Adam(...).step() (reference src/models/train.py:344,461;
// src/models/adversarial_trainer.py:56-59,98,114): lr from the caller, betas (0.9, 0.999), eps 1e-8,
// no weight decay, no amsgrad.  Arithmetic order follows torch's single-tensor Adam:
//   m = m + (g - m)*(1-b1);  v = v*b2 + (1-b2)*g*g;  p -= (lr/bc1) * m / (sqrt(v)/sqrt(bc2) + eps)
// The betas arrive as doubles and 1-b1, 1-b2 are formed in double and rounded once, as torch forms them: 1.f - 0.999f is
// 0.00099998713, 1.3e-5 off 0.001, and v carried that error (tests/test_gpu_norm_grade.py).
#include "common.h"

namespace udaseg {

__global__ void adam_flat_kernel(f32x4* __restrict__ p, const f32x4* __restrict__ g, f32x4* __restrict__ m,
                                 f32x4* __restrict__ v, int64_t n4, float* __restrict__ ptail, const float* __restrict__ gtail,
                                 float* __restrict__ mtail, float* __restrict__ vtail, int tail, float step_size, float omb1,
                                 float beta2, float omb2, float eps, float inv_sqrt_bc2) {
  const int64_t T = (int64_t)gridDim.x * blockDim.x;
  const int64_t g0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (int64_t i = g0; i < n4; i += T) {
    const f32x4 gg = g[i];
    f32x4 mm = m[i], vv = v[i], pp = p[i];
    mm = mm + (gg - mm) * omb1;
    vv = vv * beta2 + gg * gg * omb2;
    f32x4 upd;
#pragma unroll
    for (int e = 0; e < 4; ++e) upd[e] = mm[e] / (sqrtf(vv[e]) * inv_sqrt_bc2 + eps);
    pp = pp - upd * step_size;
    m[i] = mm;
    v[i] = vv;
    p[i] = pp;
  }
  if (g0 < tail) {
    const float gg = gtail[g0];
    float mm = mtail[g0], vv = vtail[g0];
    mm = mm + (gg - mm) * omb1;
    vv = vv * beta2 + gg * gg * omb2;
    ptail[g0] -= step_size * (mm / (sqrtf(vv) * inv_sqrt_bc2 + eps));
    mtail[g0] = mm;
    vtail[g0] = vv;
  }
}

// ---- global-norm gradient clipping (torch.nn.utils.clip_grad_norm_, reference src/models/unsupervised_trainer.py:144) ----
// Sum of squares in fp64: every block folds its grid-stride share (fixed order: per thread, then across the wave, then across
// the block's waves) and stores ONE partial; the block that finishes last adds the partials in index order.  No floating-point
// atomics: two runs over the same data give the same bits.  The arrival counter is an integer in the word after the partials;
// the last block clears it again, so the caller zeroes the buffer once, when it allocates it.
constexpr int SUMSQ_BLOCKS = UDASEG_SUMSQ_PARTIALS;

__global__ __launch_bounds__(256) void sumsq_kernel(const float* __restrict__ g, int64_t n4, int64_t count, double* __restrict__ partials,
                                                    double* __restrict__ out, int accumulate) {
  __shared__ double red[4];
  __shared__ bool last;
  const int64_t T = (int64_t)gridDim.x * blockDim.x;
  const int64_t g0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  double s = 0.0;
  const f32x4* g4 = reinterpret_cast<const f32x4*>(g);
  for (int64_t i = g0; i < n4; i += T) {
    const f32x4 v = g4[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) s += (double)v[e] * (double)v[e];
  }
  for (int64_t i = n4 * 4 + g0; i < count; i += T) s += (double)g[i] * (double)g[i];
  s = wave_sum_d(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  unsigned int* counter = reinterpret_cast<unsigned int*>(partials + SUMSQ_BLOCKS);
  if (threadIdx.x == 0) {
    partials[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
    __threadfence();
    last = atomicAdd(counter, 1u) == gridDim.x - 1;
  }
  __syncthreads();
  if (!last) return;
  __threadfence();
  if (threadIdx.x < 64) {
    double t = 0.0;
    for (int i = threadIdx.x; i < (int)gridDim.x; i += 64) t += __hip_atomic_load(partials + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    t = wave_sum_d(t);
    if (threadIdx.x == 0) {
      *out = accumulate ? *out + t : t;
      *counter = 0u;
    }
  }
}

// g *= min(1, max_norm / (sqrt(sumsq) + eps)), the coefficient in fp64 from the device scalar and the product rounded once; a
// coefficient of 1 leaves the gradients untouched, a NaN norm propagates (torch's error_if_nonfinite=False behaviour)
__global__ __launch_bounds__(256) void scale_by_clip_kernel(float* __restrict__ g, int64_t n4, int64_t count, const double* __restrict__ sumsq,
                                                            double max_norm, double eps) {
  const double coef = max_norm / (sqrt(*sumsq) + eps);
  if (coef >= 1.0) return;
  const int64_t T = (int64_t)gridDim.x * blockDim.x;
  const int64_t g0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  f32x4* g4 = reinterpret_cast<f32x4*>(g);
  for (int64_t i = g0; i < n4; i += T) {
    f32x4 v = g4[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = (float)((double)v[e] * coef);
    g4[i] = v;
  }
  for (int64_t i = n4 * 4 + g0; i < count; i += T) g[i] = (float)((double)g[i] * coef);
}

static inline int flat_blocks(int64_t count, int cap) {
  int64_t want = (count / 4 + 1023) / 1024;
  return (int)(want > cap ? cap : (want < 1 ? 1 : want));
}

}  // namespace udaseg

using namespace udaseg;

extern "C" int udaseg_sumsq_f32(const float* g, int64_t count, double* partials, double* out, int accumulate, void* stream) {
  UDASEG_CHECK_ARG(g && partials && out && count > 0, "sumsq_f32: bad arguments");
  UDASEG_CHECK_ARG(((uintptr_t)g & 3) == 0 && ((uintptr_t)partials & 7) == 0 && ((uintptr_t)out & 7) == 0, "sumsq_f32: misaligned pointers");
  const int64_t n4 = ((uintptr_t)g & 15) == 0 ? count / 4 : 0;       // 16-byte loads when the pointer allows them
  hipLaunchKernelGGL(sumsq_kernel, dim3(flat_blocks(count, SUMSQ_BLOCKS)), dim3(256), 0, as_stream(stream), g, n4, count, partials, out,
                     accumulate);
  UDASEG_LAUNCH_CHECK("sumsq_f32 launch");
  return UDASEG_OK;
}

extern "C" int udaseg_scale_by_clip_f32(float* g, int64_t count, const double* sumsq, float max_norm, float eps, void* stream) {
  UDASEG_CHECK_ARG(g && sumsq && count > 0, "scale_by_clip_f32: bad arguments");
  UDASEG_CHECK_ARG(max_norm >= 0.f && eps >= 0.f, "scale_by_clip_f32: max_norm and eps must not be negative");
  UDASEG_CHECK_ARG(((uintptr_t)g & 3) == 0 && ((uintptr_t)sumsq & 7) == 0, "scale_by_clip_f32: misaligned pointers");
  const int64_t n4 = ((uintptr_t)g & 15) == 0 ? count / 4 : 0;
  hipLaunchKernelGGL(scale_by_clip_kernel, dim3(flat_blocks(count, 2048)), dim3(256), 0, as_stream(stream), g, n4, count, sumsq,
                     (double)max_norm, (double)eps);
  UDASEG_LAUNCH_CHECK("scale_by_clip_f32 launch");
  return UDASEG_OK;
}

extern "C" int udaseg_adam_flat(float* p, const float* g, float* m, float* v, int64_t count, float lr, double beta1,
                                double beta2, float eps, float bc1, float bc2, void* stream) {
  UDASEG_CHECK_ARG(p && g && m && v && count > 0, "adam_flat: bad arguments");
  UDASEG_CHECK_ARG(bc1 > 0.f && bc2 > 0.f, "adam_flat: bias corrections must be positive");
  UDASEG_CHECK_ARG((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0, "adam_flat: pointers must be 16-byte aligned");
  const int64_t n4 = count / 4;
  const int tail = (int)(count - n4 * 4);
  int64_t want = (n4 + 511) / 512;
  if (want > 2048) want = 2048;
  if (want < 1) want = 1;
  hipLaunchKernelGGL(adam_flat_kernel, dim3((int)want), dim3(256), 0, as_stream(stream), (f32x4*)p, (const f32x4*)g, (f32x4*)m,
                     (f32x4*)v, n4, p + n4 * 4, g + n4 * 4, m + n4 * 4, v + n4 * 4, tail, lr / bc1, (float)(1.0 - beta1), (float)beta2,
                     (float)(1.0 - beta2), eps, 1.0f / sqrtf(bc2));
  UDASEG_LAUNCH_CHECK("adam_flat launch");
  return UDASEG_OK;
}
