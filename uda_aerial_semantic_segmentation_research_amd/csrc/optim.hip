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

// ---- mean teacher: t <- t + (1 - decay) * (s - t) over two flat fp32 arenas (Tarvainen & Valpola 2017; teacher.py) ----
// One streaming pass, 12 B per element (8 read, 4 written).  Arithmetic contract (include/udaseg.h, INTEGRATION.md "Mean
// teacher"): w = (float)(1.0 - decay) formed in double and rounded once; per element d = s - t in fp32, t = fmaf(w, d, t) -- an
// explicit fmaf, so the bits do not depend on whether the compiler contracts; d == 0 keeps t's bits (a -0 stays -0).  The host
// picks the MODE from the uniform scalar: decay == 0 is a copy (t + (s - t) is not s in general), decay == 1 writes nothing.
// DIST: the fp64 sum of (s - t_new)^2 of the same pass, folded as sumsq_kernel folds its sum (per thread, wave, block; the block
// that arrives last adds the partials in index order; no floating-point atomics), in the same caller-owned scratch.
// A thread keeps four 16-byte vectors of each arena in flight and the grid gives it two rounds of that.  With DIST the grid is
// capped at the partials buffer, one wave per SIMD at best: 36 us against 26 us without DIST on the r18 arena, a device copy of
// one arena at 17 us (profiles/teacher_bench.txt; all three resident in the Infinity Cache).
enum { EMA_LERP = 0, EMA_COPY = 1, EMA_KEEP = 2 };
constexpr int EMA_UNROLL = 4;
static inline int ema_blocks(int64_t count, int cap) {
  const int64_t per_block = 256 * 2 * EMA_UNROLL, want = (count / 4 + per_block - 1) / per_block;
  return (int)(want > cap ? cap : (want < 1 ? 1 : want));
}

template <int MODE>
__device__ __forceinline__ float ema_elem(float t, float s, float w) {
  if (MODE == EMA_COPY) return s;
  if (MODE == EMA_KEEP) return t;
  const float d = s - t;
  return d == 0.f ? t : fmaf(w, d, t);
}

template <int MODE, bool DIST>
__global__ __launch_bounds__(256) void ema_flat_kernel(float* __restrict__ t, const float* __restrict__ s, int64_t n4, int64_t count,
                                                       float w, double* __restrict__ partials, double* __restrict__ dist2,
                                                       int accumulate) {
  const int64_t T = (int64_t)gridDim.x * blockDim.x;
  const int64_t g0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  double acc = 0.0;
  f32x4* t4 = reinterpret_cast<f32x4*>(t);
  const f32x4* s4 = reinterpret_cast<const f32x4*>(s);
  for (int64_t i = g0; i < n4; i += EMA_UNROLL * T) {
    f32x4 tv[EMA_UNROLL], sv[EMA_UNROLL];
#pragma unroll
    for (int u = 0; u < EMA_UNROLL; ++u) {
      const int64_t j = i + u * T;
      if (j < n4) {
        sv[u] = s4[j];
        if (MODE != EMA_COPY) tv[u] = t4[j];
      }
    }
#pragma unroll
    for (int u = 0; u < EMA_UNROLL; ++u) {
      const int64_t j = i + u * T;
      if (j < n4) {
        f32x4 r;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          r[e] = ema_elem<MODE>(MODE == EMA_COPY ? 0.f : tv[u][e], sv[u][e], w);
          if (DIST) {
            const double q = (double)sv[u][e] - (double)r[e];
            acc += q * q;
          }
        }
        if (MODE != EMA_KEEP) t4[j] = r;
      }
    }
  }
  for (int64_t i = n4 * 4 + g0; i < count; i += T) {
    const float sv = s[i];
    const float r = ema_elem<MODE>(MODE == EMA_COPY ? 0.f : t[i], sv, w);
    if (DIST) {
      const double q = (double)sv - (double)r;
      acc += q * q;
    }
    if (MODE != EMA_KEEP) t[i] = r;
  }
  if (!DIST) return;
  __shared__ double red[4];
  __shared__ bool last;
  acc = wave_sum_d(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
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
    double p = 0.0;
    for (int i = threadIdx.x; i < (int)gridDim.x; i += 64) p += __hip_atomic_load(partials + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    p = wave_sum_d(p);
    if (threadIdx.x == 0) {
      *dist2 = accumulate ? *dist2 + p : p;
      *counter = 0u;
    }
  }
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

extern "C" int udaseg_ema_flat(float* t, const float* s, int64_t count, double decay, double* partials, double* dist2, int accumulate,
                               void* stream) {
  UDASEG_CHECK_ARG(t && s && count > 0, "ema_flat: bad arguments");
  UDASEG_CHECK_ARG(decay >= 0.0 && decay <= 1.0, "ema_flat: decay must lie in [0, 1], got %g", decay);      // false for a NaN
  UDASEG_CHECK_ARG((((uintptr_t)t | (uintptr_t)s) & 3) == 0, "ema_flat: pointers must be 4-byte aligned");
  UDASEG_CHECK_ARG(!dist2 || partials, "ema_flat: dist2 needs the partials scratch");
  UDASEG_CHECK_ARG(!dist2 || ((((uintptr_t)partials | (uintptr_t)dist2) & 7) == 0), "ema_flat: misaligned fp64 pointers");
  const uintptr_t ta = (uintptr_t)t, sa = (uintptr_t)s, bytes = (uintptr_t)count * 4;
  UDASEG_CHECK_ARG(ta + bytes <= sa || sa + bytes <= ta, "ema_flat: t and s overlap");
  const int mode = decay == 0.0 ? EMA_COPY : decay == 1.0 ? EMA_KEEP : EMA_LERP;
  if (mode == EMA_KEEP && !dist2) return UDASEG_OK;                    // nothing to write, nothing to sum
  const int64_t n4 = ((ta | sa) & 15) == 0 ? count / 4 : 0;            // 16-byte vectors when both pointers allow them
  const float w = (float)(1.0 - decay);
  const dim3 grid(ema_blocks(count, dist2 ? SUMSQ_BLOCKS : 2048)), block(256);
  hipStream_t st = as_stream(stream);
#define EMA_LAUNCH(MODE, DIST) \
  hipLaunchKernelGGL((ema_flat_kernel<MODE, DIST>), grid, block, 0, st, t, s, n4, count, w, partials, dist2, accumulate)
  if (dist2) {
    if (mode == EMA_COPY) EMA_LAUNCH(EMA_COPY, true);
    else if (mode == EMA_KEEP) EMA_LAUNCH(EMA_KEEP, true);
    else EMA_LAUNCH(EMA_LERP, true);
  } else {
    if (mode == EMA_COPY) EMA_LAUNCH(EMA_COPY, false);
    else EMA_LAUNCH(EMA_LERP, false);
  }
#undef EMA_LAUNCH
  UDASEG_LAUNCH_CHECK("ema_flat launch");
  return UDASEG_OK;
}
