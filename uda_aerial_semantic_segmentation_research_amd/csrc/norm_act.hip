// Training-mode batch norm (+ReLU / LeakyReLU / residual add) forward and backward, the activation backward and the channel
// sums, NHWC in fp32 or bf16 storage (gfx950).
//
// Replaces torch.nn.BatchNorm2d / ReLU / LeakyReLU / `out += identity` and their autograd inside smp.Unet
// (reference src/models/train.py:341,343) and DomainDiscriminator (src/models/discriminator.py:21-33).
//
// All kernels here are HBM-bound streams over a [pixels][C] tensor read as 16-byte vectors (Vec16<BF>: 4 fp32 or 8 bf16
// channels, arithmetic and all statistics in fp32 / f64).  Each is written once and instantiated per storage by its two
// extern "C" entry points (BASELINE configs 3 / 5 run the bf16 ones).  The launch is shaped so that (total threads) %
// (vectors per pixel) == 0, hence every thread meets the same channels on every grid-stride step and keeps its per-channel
// partials in registers; one LDS pass folds the rows of a block, one f64 atomic per channel per block folds the blocks (f64:
// the cross-block order no longer shows after rounding to f32).
#include "launch.h"
#include "vec16.h"

namespace udaseg {

// the N coefficients of channel group q out of one LDS row of C floats
template <int N>
__device__ __forceinline__ void load_row(const float* row, int q, float (&out)[N]) {
#pragma unroll
  for (int e = 0; e < N; ++e) out[e] = row[q * N + e];
}

// channel c of the BN_REPLICAS replicated [2][C] f64 accumulator sets
__device__ __forceinline__ void replica_sums(const double* __restrict__ sums, int C, int c, double& s1, double& s2) {
  s1 = 0.0;
  s2 = 0.0;
#pragma unroll
  for (int r = 0; r < BN_REPLICAS; ++r) {
    s1 += sums[(size_t)r * 2 * C + c];
    s2 += sums[(size_t)r * 2 * C + C + c];
  }
}

// Replicated f64 sums of channel c -> mean, clamped variance, rstd and the scale = gamma * rstd, shift = beta - mean * scale
// that the forward applies with ONE fused multiply-add; `owner` (one thread per channel of the launch) also writes the saved and
// the running statistics.  The one statement of this arithmetic: bn_apply's prologue and bn_finalize give the same numbers.
__device__ __forceinline__ void bn_fold_channel(const double* __restrict__ sums, const float* __restrict__ gamma,
                                                const float* __restrict__ beta, int C, int c, int64_t pixels, float eps,
                                                float momentum, bool owner, float* running_mean, float* running_var,
                                                float* save_mean, float* save_rstd, float* scale, float* shift) {
  const double inv = 1.0 / (double)pixels;
  double s1, s2;
  replica_sums(sums, C, c, s1, s2);
  const double m = s1 * inv;
  double var = s2 * inv - m * m;
  var = var > 0.0 ? var : 0.0;
  const float rstd = (float)(1.0 / sqrt(var + (double)eps));
  const float sc = gamma[c] * rstd;
  scale[c] = sc;
  shift[c] = beta[c] - (float)m * sc;
  if (owner) {
    if (save_mean) save_mean[c] = (float)m;
    if (save_rstd) save_rstd[c] = rstd;
    if (running_mean) {
      // in f64 and rounded once: the fp32 form rounded six times and could land 2.3 ulp off (tests/test_gpu_norm_grade.py)
      const double unb = pixels > 1 ? var * ((double)pixels / (double)(pixels - 1)) : var, mo = (double)momentum;
      running_mean[c] = (float)((1.0 - mo) * (double)running_mean[c] + mo * m);
      running_var[c] = (float)((1.0 - mo) * (double)running_var[c] + mo * unb);
    }
  }
}

// Per-channel sum and sum of squares into the f64 replicas (what a convolution's fused statistics epilogue adds; the bf16 one
// stands behind the library GEMMs of csrc/gemm_lt.hip, which have no such epilogue).
template <bool BF>
__global__ void bn_stats_kernel(const f32x4* __restrict__ y, int64_t nq, int cq, double* __restrict__ sums) {
  // f64 accumulation: E[x^2] - mean^2 then loses nothing to the fp32 partials (the kernel is HBM-bound anyway)
  constexpr int N = Vec16<BF>::N;
  __shared__ double red[256 * N];
  const int64_t T = (int64_t)gridDim.x * blockDim.x;
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  double s[N] = {}, ss[N] = {};
  for (int64_t i = g; i < nq; i += T) {
    const Vec16<BF> v = Vec16<BF>::from(y[i]);
#pragma unroll
    for (int e = 0; e < N; ++e) {
      const double d = (double)v.v[e];
      s[e] += d;
      ss[e] += d * d;
    }
  }
  double* rep = sums + (size_t)(blockIdx.x % BN_REPLICAS) * 2 * cq * N;
  block_fold_atomic<N, double>(s, rep, cq, red);
  block_fold_atomic<N, double>(ss, rep + (size_t)cq * N, cq, red);
}

// Per-channel coefficients are computed ONCE per block (one CHANNEL per thread, strided: all threads share the replica sums,
// 32 independent loads each) into LDS; every thread then picks the group it streams.  (Summing the 16 replicas in every thread
// cost more than the streaming itself on small tensors.)
template <bool BF>
__global__ void bn_apply_kernel(const f32x4* __restrict__ y, const double* __restrict__ sums,
                                const float* __restrict__ gamma, const float* __restrict__ beta,
                                const f32x4* __restrict__ residual, f32x4* __restrict__ z, int64_t nq, int cq,
                                int64_t pixels, float eps, float momentum, float* running_mean, float* running_var,
                                float* save_mean, float* save_rstd, int act, float slope) {
  constexpr int N = Vec16<BF>::N;
  extern __shared__ __attribute__((aligned(16))) float coef[];  // [2][C]: scale, shift
  const int C = cq * N;
  for (int c = threadIdx.x; c < C; c += blockDim.x)
    bn_fold_channel(sums, gamma, beta, C, c, pixels, eps, momentum, blockIdx.x == 0, running_mean, running_var, save_mean,
                    save_rstd, coef, coef + C);
  __syncthreads();
  const int64_t T = (int64_t)gridDim.x * blockDim.x;
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int q = (int)(g % cq);
  if constexpr (!BF) {
    // fp32 keeps its loop written out on four-element vectors: the compiler packs their arithmetic (v_pk_fma_f32, v_pk_add_f32),
    // which it does not do for the element-wise body below, and that body cost the 67-134 MB layers 1-1.5 us of 32-59
    // (profiles/elem_storage_refactor.txt)
    const float4* coef4 = reinterpret_cast<const float4*>(coef);
    const float4 sc4 = coef4[q], sh4 = coef4[cq + q];
    const f32x4 scale = {sc4.x, sc4.y, sc4.z, sc4.w}, shift = {sh4.x, sh4.y, sh4.z, sh4.w};
    // four independent 16-byte streams per thread in flight (a single dependent load per iteration left HBM at ~3.9 TB/s)
    int64_t i = g;
    for (; i + 3 * T < nq; i += 4 * T) {
      f32x4 yy[4], rr[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) yy[u] = y[i + u * T];
      if (residual) {
#pragma unroll
        for (int u = 0; u < 4; ++u) rr[u] = residual[i + u * T];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = __builtin_fmaf(yy[u][e], scale[e], shift[e]);   // the backward re-evaluates exactly this
        if (residual) v += rr[u];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = act_apply(v[e], act, slope);
        z[i + u * T] = v;
      }
    }
    for (; i < nq; i += T) {
      const f32x4 yy = y[i];
      f32x4 v;
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = __builtin_fmaf(yy[e], scale[e], shift[e]);
      if (residual) v += residual[i];
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = act_apply(v[e], act, slope);
      z[i] = v;
    }
  } else {
    float sc[N], sh[N];
    load_row<N>(coef, q, sc);
    load_row<N>(coef + C, q, sh);
    auto body = [&](int64_t i, const f32x4 yv, const f32x4 rv) {
      Vec16<BF> v = Vec16<BF>::from(yv), r;
      if (residual) r = Vec16<BF>::from(rv);
  #pragma unroll
      for (int e = 0; e < N; ++e) {
        float t = __builtin_fmaf(v.v[e], sc[e], sh[e]);   // the backward re-evaluates exactly this
        if (residual) t += r.v[e];
        v.v[e] = act_apply(t, act, slope);
      }
      z[i] = v.raw();
    };
    // four independent 16-byte streams per array per thread in flight (a single dependent load per iteration left HBM at ~3.9 TB/s)
    const f32x4 zero = {0, 0, 0, 0};
    int64_t i = g;
    for (; i + 3 * T < nq; i += 4 * T) {
      f32x4 a[4], b[4];
  #pragma unroll
      for (int u = 0; u < 4; ++u) {
        a[u] = y[i + u * T];
        b[u] = zero;
      }
      if (residual) {
  #pragma unroll
        for (int u = 0; u < 4; ++u) b[u] = residual[i + u * T];
      }
  #pragma unroll
      for (int u = 0; u < 4; ++u) body(i + u * T, a[u], b[u]);
    }
    for (; i < nq; i += T) body(i, y[i], residual ? residual[i] : zero);
  }
}

__global__ void bn_apply_eval_kernel(const f32x4* __restrict__ y, const float* __restrict__ gamma,
                                     const float* __restrict__ beta, const float* __restrict__ rm,
                                     const float* __restrict__ rv, const f32x4* __restrict__ residual,
                                     f32x4* __restrict__ z, int64_t n4, int c4, float eps, int act, float slope) {
  const int64_t T = (int64_t)gridDim.x * blockDim.x;
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int q = (int)(g % c4);
  f32x4 scale, shift;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int c = q * 4 + e;
    const float rstd = 1.0f / sqrtf(rv[c] + eps);
    scale[e] = gamma[c] * rstd;
    shift[e] = beta[c] - rm[c] * scale[e];
  }
  for (int64_t i = g; i < n4; i += T) {
    f32x4 v = y[i] * scale + shift;
    if (residual) v += residual[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = act_apply(v[e], act, slope);
    z[i] = v;
  }
}

// Training-mode BatchNorm statistics -> everything the layer's consumers need, WITHOUT touching the activation: mean / rstd
// (saved for the backward), the running statistics, and the per-channel scale / shift that a consumer applies while it stages
// its input (udaseg_conv2d_fwd_frag_bf16 in_scale / in_shift): bn_apply's prologue on its own.
__global__ void bn_finalize_kernel(const double* __restrict__ sums, const float* __restrict__ gamma, const float* __restrict__ beta,
                                   int C, int64_t pixels, float eps, float momentum, float* running_mean, float* running_var,
                                   float* save_mean, float* save_rstd, float* scale, float* shift) {
  for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < C; c += gridDim.x * blockDim.x)
    bn_fold_channel(sums, gamma, beta, C, c, pixels, eps, momentum, true, running_mean, running_var, save_mean, save_rstd, scale,
                    shift);
}

// fp32 with z == nullptr and an activation: the layer had no residual input, so the activation's argument is bn(y) itself and is
// re-evaluated from y (same fused multiply-add, same coefficients as bn_apply_kernel) instead of reading z: one fewer pass over
// the activation in each of the two backward kernels.  (bf16 callers always pass z with an activation here: the sums of their
// unwritten activations come out of the consumer's data-gradient epilogue, not of this kernel.)
template <bool BF>
__global__ void bn_bwd_reduce_kernel(const f32x4* __restrict__ dz, const f32x4* __restrict__ z,
                                     const f32x4* __restrict__ y, const float* __restrict__ save_mean,
                                     const float* __restrict__ save_rstd, const float* __restrict__ gamma,
                                     const float* __restrict__ beta, int64_t nq, int cq,
                                     double* __restrict__ bsums, int act, float slope) {
  constexpr int N = Vec16<BF>::N;
  __shared__ double red[256 * N];
  const int64_t T = (int64_t)gridDim.x * blockDim.x;
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int q = (int)(g % cq);
  const bool recompute = !BF && !z && act != UDASEG_ACT_NONE;
  float mean[N], rstd[N], sc[N] = {}, sh[N] = {};
#pragma unroll
  for (int e = 0; e < N; ++e) {
    mean[e] = save_mean[q * N + e];
    rstd[e] = save_rstd[q * N + e];
    if (recompute) {
      sc[e] = gamma[q * N + e] * rstd[e];
      sh[e] = beta[q * N + e] - mean[e] * sc[e];
    }
  }
  double sg[N] = {}, sgx[N] = {};
  auto body = [&](const f32x4 gv, const f32x4 yv, const f32x4 zv) {
    Vec16<BF> gz = Vec16<BF>::from(gv);
    const Vec16<BF> yy = Vec16<BF>::from(yv);
    if (act != UDASEG_ACT_NONE) {
      Vec16<BF> zz = Vec16<BF>::from(zv);
      if (recompute) {
#pragma unroll
        for (int e = 0; e < N; ++e) zz.v[e] = __builtin_fmaf(yy.v[e], sc[e], sh[e]);
      }
#pragma unroll
      for (int e = 0; e < N; ++e) gz.v[e] *= act_grad(zz.v[e], act, slope);
    }
#pragma unroll
    for (int e = 0; e < N; ++e) {
      const float xh = (yy.v[e] - mean[e]) * rstd[e];
      sg[e] += (double)gz.v[e];
      sgx[e] += (double)gz.v[e] * (double)xh;
    }
  };
  // four independent iterations of loads in flight per thread (same summation order as the plain loop)
  const f32x4 zero = {0, 0, 0, 0};
  const bool need_z = z != nullptr && act != UDASEG_ACT_NONE;
  int64_t i = g;
  for (; i + 3 * T < nq; i += 4 * T) {
    f32x4 a[4], b[4], c[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      a[u] = dz[i + u * T];
      b[u] = y[i + u * T];
      c[u] = zero;
    }
    if (need_z) {
#pragma unroll
      for (int u = 0; u < 4; ++u) c[u] = z[i + u * T];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) body(a[u], b[u], c[u]);
  }
  for (; i < nq; i += T) body(dz[i], y[i], need_z ? z[i] : zero);
  double* rep = bsums + (size_t)(blockIdx.x % BN_REPLICAS) * 2 * cq * N;
  block_fold_atomic<N, double>(sg, rep, cq, red);
  block_fold_atomic<N, double>(sgx, rep + (size_t)cq * N, cq, red);
}

template <bool BF>
__global__ void bn_bwd_apply_kernel(const f32x4* __restrict__ dz, const f32x4* __restrict__ z,
                                    const f32x4* __restrict__ y, const float* __restrict__ save_mean,
                                    const float* __restrict__ save_rstd, const float* __restrict__ gamma,
                                    const float* __restrict__ beta, const double* __restrict__ bsums,
                                    f32x4* __restrict__ dy, f32x4* __restrict__ dres,
                                    float* dgamma, float* dbeta, int64_t nq, int cq, int64_t pixels, int act,
                                    float slope, int acc_dy, int acc_dres, int acc_param,
                                    const float* __restrict__ fwd_scale, const float* __restrict__ fwd_shift) {
  constexpr int N = Vec16<BF>::N;
  // rows of C floats: mean, rstd, scale, mean(g), mean(g*xhat), then the storage's recompute rows (below)
  extern __shared__ __attribute__((aligned(16))) float coef[];
  const int C = cq * N;
  const double inv = 1.0 / (double)pixels;
  // An activation that was never written is re-evaluated from y with the SAME fused multiply-add and coefficients as the forward,
  // so the mask is bit-identical to the forward's and z is not read.  The two storages learn of it, and get the coefficients,
  // differently:
  //   fp32: z == nullptr with an activation (the layer had no residual input).  The forward's scale is row 2 already; its shift
  //         = beta - mean * scale is derived here into a sixth row (always present: [6][C]).
  //   bf16: the caller hands over the fwd_scale / fwd_shift vectors that bn_finalize gave the consumer which applied BatchNorm +
  //         activation while staging (udaseg_conv2d_fwd_frag_bf16's in_scale / in_shift); they become rows 5 and 6 ([7][C],
  //         otherwise [5][C]).
  const bool recompute = BF ? fwd_scale != nullptr : !z && act != UDASEG_ACT_NONE;
  for (int c = threadIdx.x; c < C; c += blockDim.x) {     // one channel per thread, see bn_apply_kernel
    double s1, s2;
    replica_sums(bsums, C, c, s1, s2);
    const float rs = save_rstd[c], mu = save_mean[c], gs = gamma[c] * rs;
    coef[c] = mu;
    coef[C + c] = rs;
    coef[2 * C + c] = gs;
    coef[3 * C + c] = (float)(s1 * inv);
    coef[4 * C + c] = (float)(s2 * inv);
    if constexpr (BF) {
      if (recompute) {
        coef[5 * C + c] = fwd_scale[c];
        coef[6 * C + c] = fwd_shift[c];
      }
    } else {
      coef[5 * C + c] = recompute ? beta[c] - mu * gs : 0.f;
    }
    if (blockIdx.x == 0) {
      const float db = (float)s1, dg = (float)s2;
      if (dbeta) dbeta[c] = acc_param ? dbeta[c] + db : db;
      if (dgamma) dgamma[c] = acc_param ? dgamma[c] + dg : dg;
    }
  }
  __syncthreads();
  const int64_t T = (int64_t)gridDim.x * blockDim.x;
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int q = (int)(g % cq);
  float mean[N], rstd[N], scale[N], mg[N], mgx[N];
  load_row<N>(coef, q, mean);
  load_row<N>(coef + C, q, rstd);
  load_row<N>(coef + 2 * C, q, scale);
  load_row<N>(coef + 3 * C, q, mg);
  load_row<N>(coef + 4 * C, q, mgx);
  // the recompute coefficients: fp32 keeps its shift in registers beside the scale it has anyway; bf16 reads its two rows from
  // LDS in the loop (sixteen more registers there cost the occupancy the streams need)
  float shift[N] = {};
  if constexpr (!BF) load_row<N>(coef + 5 * C, q, shift);
  auto body = [&](int64_t i, const f32x4 gv, const f32x4 yv, const f32x4 zv, const f32x4 ov, const f32x4 rv) {
    Vec16<BF> gz = Vec16<BF>::from(gv), zz, out, old;
    const Vec16<BF> yy = Vec16<BF>::from(yv);
    if (act != UDASEG_ACT_NONE && !recompute) zz = Vec16<BF>::from(zv);
    if (acc_dy) old = Vec16<BF>::from(ov);
    if (recompute) {
#pragma unroll
      for (int e = 0; e < N; ++e) {
        if constexpr (BF) zz.v[e] = __builtin_fmaf(yy.v[e], coef[5 * C + q * N + e], coef[6 * C + q * N + e]);
        else zz.v[e] = __builtin_fmaf(yy.v[e], scale[e], shift[e]);
      }
    }
#pragma unroll
    for (int e = 0; e < N; ++e) {
      if (act != UDASEG_ACT_NONE) gz.v[e] *= act_grad(zz.v[e], act, slope);
      const float xh = (yy.v[e] - mean[e]) * rstd[e];
      out.v[e] = scale[e] * (gz.v[e] - mg[e] - xh * mgx[e]);
      if (acc_dy) out.v[e] += old.v[e];
    }
    dy[i] = out.raw();
    if (dres) {
      if (acc_dres) gz += Vec16<BF>::from(rv);
      dres[i] = gz.raw();
    }
  };
  // (a four-deep unroll like bn_apply's was measured here and LOST: 82.7 -> 123 us on the 134 MB fp32 layers -- five arrays of
  // four vectors cost the occupancy the streams need; the plain loop already has two or three loads in flight per thread)
  const f32x4 zero = {0, 0, 0, 0};
  const bool need_z = z != nullptr && act != UDASEG_ACT_NONE && !recompute, need_res = dres != nullptr && acc_dres;
  for (int64_t i = g; i < nq; i += T) body(i, dz[i], y[i], need_z ? z[i] : zero, acc_dy ? dy[i] : zero, need_res ? dres[i] : zero);
}

template <bool BF>
__global__ void act_bwd_kernel(const f32x4* __restrict__ dz, const f32x4* __restrict__ z, f32x4* __restrict__ dy,
                               int64_t nq, int act, float slope) {
  const int64_t T = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nq; i += T) {
    Vec16<BF> gz = Vec16<BF>::from(dz[i]);
    const Vec16<BF> zz = Vec16<BF>::from(z[i]);
#pragma unroll
    for (int e = 0; e < Vec16<BF>::N; ++e) gz.v[e] *= act_grad(zz.v[e], act, slope);
    dy[i] = gz.raw();
  }
}

template <bool BF>
__global__ void channel_sum_kernel(const f32x4* __restrict__ x, int64_t nq, int cq, float* __restrict__ out, int replicas) {
  constexpr int N = Vec16<BF>::N;
  out += (size_t)(blockIdx.x % replicas) * cq * N;
  __shared__ __attribute__((aligned(16))) float red[256 * N];
  const int64_t T = (int64_t)gridDim.x * blockDim.x;
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  Vec16<BF> s = Vec16<BF>::zero();
  for (int64_t i = g; i < nq; i += T) s += Vec16<BF>::from(x[i]);
  block_fold_atomic<N, float>(s.v, out, cq, red);
}

// Eval mode: fold BatchNorm into the preceding conv.  w'[co][j] = w[co][j] * gamma/sqrt(var+eps); b'[co] = beta +
// (bias - mean) * gamma/sqrt(var+eps).  Row-wise over the OHWI weight (j = taps*ci).
__global__ void bn_fold_kernel(const float* __restrict__ w, const float* __restrict__ bias, const float* __restrict__ gamma,
                               const float* __restrict__ beta, const float* __restrict__ rm, const float* __restrict__ rv,
                               float eps, int co, int J, float* __restrict__ wf, float* __restrict__ bf) {
  const int o = blockIdx.x;
  if (o >= co) return;
  const float s = gamma[o] / sqrtf(rv[o] + eps);
  for (int j = threadIdx.x; j < J; j += blockDim.x) wf[(size_t)o * J + j] = w[(size_t)o * J + j] * s;
  if (threadIdx.x == 0) bf[o] = beta[o] + ((bias ? bias[o] : 0.f) - rm[o]) * s;
}

// vec: channels per 16-byte vector of the storage (4 fp32, 8 bf16)
static int check_pc(int64_t pixels, int c, int vec, const char* who) {
  UDASEG_CHECK_ARG(pixels > 0 && c > 0 && c % vec == 0, "%s: need pixels > 0 and channels a positive multiple of %d (got %lld, %d)",
                   who, vec, (long long)pixels, c);
  UDASEG_CHECK_ARG(c <= UDASEG_BN_MAX_C, "%s: too many channels (%d, at most %d)", who, c, UDASEG_BN_MAX_C);
  return UDASEG_OK;
}

}  // namespace udaseg

using namespace udaseg;

extern "C" int udaseg_bn_replicas(void) { return BN_REPLICAS; }

extern "C" int udaseg_bn_stats(const float* y, int64_t pixels, int c, double* sums, void* stream) {
  int rc = check_pc(pixels, c, 4, "bn_stats");
  if (rc) return rc;
  UDASEG_CHECK_ARG(y && sums, "bn_stats: NULL pointer");
  const int64_t n4 = pixels * (c / 4);
  const StreamShape s = stream_shape(n4, c / 4, reduce_max_blocks());
  hipLaunchKernelGGL(bn_stats_kernel<false>, dim3(s.grid), dim3(s.bs), 0, as_stream(stream), (const f32x4*)y, n4, s.c4, sums);
  UDASEG_LAUNCH_CHECK("bn_stats launch");
  return UDASEG_OK;
}

extern "C" int udaseg_bn_stats_bf16(const void* y, int64_t pixels, int c, double* sums, void* stream) {
  int rc = check_pc(pixels, c, 8, "bn_stats_bf16");
  if (rc) return rc;
  UDASEG_CHECK_ARG(y && sums, "bn_stats_bf16: NULL pointer");
  const int64_t n8 = pixels * (c / 8);
  const StreamShape s = stream_shape(n8, c / 8, reduce_max_blocks());
  static KernelRec rec_bn_stats_bf16_kernel(nullptr, "bn_stats_bf16_kernel");
  KTimer kt_bn_stats_bf16_kernel(rec_bn_stats_bf16_kernel, as_stream(stream), (double)pixels * c * 2.0);
  hipLaunchKernelGGL(bn_stats_kernel<true>, dim3(s.grid), dim3(s.bs), 0, as_stream(stream), (const f32x4*)y, n8, s.c4, sums);
  UDASEG_LAUNCH_CHECK("bn_stats_bf16 launch");
  return UDASEG_OK;
}

extern "C" int udaseg_bn_apply(const float* y, const double* sums, const float* gamma, const float* beta,
                               const float* residual, float* z, int64_t pixels, int c, float eps, float momentum,
                               float* running_mean, float* running_var, float* save_mean, float* save_rstd, int act,
                               float slope, void* stream) {
  int rc = check_pc(pixels, c, 4, "bn_apply");
  if (rc) return rc;
  UDASEG_CHECK_ARG(y && sums && gamma && beta && z, "bn_apply: NULL pointer");
  UDASEG_CHECK_ARG((running_mean == nullptr) == (running_var == nullptr), "bn_apply: running_mean/var must come together");
  const int64_t n4 = pixels * (c / 4);
  const StreamShape s = stream_shape(n4, c / 4, 2048, apply_per_thread());
  static KernelRec rec_ba(nullptr, "bn_apply_kernel");
  KTimer kt_ba(rec_ba, as_stream(stream), (double)pixels * c * 4.0 * (residual ? 3.0 : 2.0));
  hipLaunchKernelGGL(bn_apply_kernel<false>, dim3(s.grid), dim3(s.bs), (size_t)2 * s.c4 * sizeof(float4), as_stream(stream), (const f32x4*)y, sums, gamma, beta,
                     (const f32x4*)residual, (f32x4*)z, n4, s.c4, pixels, eps, momentum, running_mean, running_var,
                     save_mean, save_rstd, act, slope);
  UDASEG_LAUNCH_CHECK("bn_apply launch");
  return UDASEG_OK;
}

extern "C" int udaseg_bn_apply_bf16(const void* y, const double* sums, const float* gamma, const float* beta,
                                    const void* residual, void* z, int64_t pixels, int c, float eps, float momentum,
                                    float* running_mean, float* running_var, float* save_mean, float* save_rstd, int act,
                                    float slope, void* stream) {
  int rc = check_pc(pixels, c, 8, "bn_apply_bf16");
  if (rc) return rc;
  UDASEG_CHECK_ARG(y && sums && gamma && beta && z, "bn_apply_bf16: NULL pointer");
  const int64_t n8 = pixels * (c / 8);
  const StreamShape s = stream_shape(n8, c / 8, 2048, apply_per_thread());
  static KernelRec rec_bn_apply_bf16_kernel(nullptr, "bn_apply_bf16_kernel");
  KTimer kt_bn_apply_bf16_kernel(rec_bn_apply_bf16_kernel, as_stream(stream), (double)pixels * c * 2.0 * (residual ? 3.0 : 2.0));
  hipLaunchKernelGGL(bn_apply_kernel<true>, dim3(s.grid), dim3(s.bs), (size_t)2 * c * sizeof(float), as_stream(stream),
                     (const f32x4*)y, sums, gamma, beta, (const f32x4*)residual, (f32x4*)z, n8, s.c4, pixels, eps, momentum,
                     running_mean, running_var, save_mean, save_rstd, act, slope);
  UDASEG_LAUNCH_CHECK("bn_apply_bf16 launch");
  return UDASEG_OK;
}

extern "C" int udaseg_bn_apply_eval(const float* y, const float* gamma, const float* beta, const float* running_mean,
                                    const float* running_var, const float* residual, float* z, int64_t pixels, int c,
                                    float eps, int act, float slope, void* stream) {
  int rc = check_pc(pixels, c, 4, "bn_apply_eval");
  if (rc) return rc;
  UDASEG_CHECK_ARG(y && gamma && beta && running_mean && running_var && z, "bn_apply_eval: NULL pointer");
  const int64_t n4 = pixels * (c / 4);
  const StreamShape s = stream_shape(n4, c / 4);
  hipLaunchKernelGGL(bn_apply_eval_kernel, dim3(s.grid), dim3(s.bs), 0, as_stream(stream), (const f32x4*)y, gamma, beta,
                     running_mean, running_var, (const f32x4*)residual, (f32x4*)z, n4, s.c4, eps, act, slope);
  UDASEG_LAUNCH_CHECK("bn_apply_eval launch");
  return UDASEG_OK;
}

extern "C" int udaseg_bn_finalize(const double* sums, const float* gamma, const float* beta, int64_t pixels, int c, float eps,
                                  float momentum, float* running_mean, float* running_var, float* save_mean, float* save_rstd,
                                  float* scale, float* shift, void* stream) {
  UDASEG_CHECK_ARG(sums && gamma && beta && scale && shift && pixels > 0 && c > 0, "bn_finalize: bad arguments");
  hipLaunchKernelGGL(bn_finalize_kernel, dim3(cdiv(c, 256)), dim3(256), 0, as_stream(stream), sums, gamma, beta, c, pixels, eps,
                     momentum, running_mean, running_var, save_mean, save_rstd, scale, shift);
  UDASEG_LAUNCH_CHECK("bn_finalize launch");
  return UDASEG_OK;
}

extern "C" int udaseg_bn_bwd_reduce(const float* dz, const float* z, const float* y, const float* save_mean,
                                    const float* save_rstd, const float* gamma, const float* beta, int64_t pixels, int c,
                                    double* bsums, int act, float slope, void* stream) {
  int rc = check_pc(pixels, c, 4, "bn_bwd_reduce");
  if (rc) return rc;
  UDASEG_CHECK_ARG(dz && y && save_mean && save_rstd && bsums, "bn_bwd_reduce: NULL pointer");
  UDASEG_CHECK_ARG(act == UDASEG_ACT_NONE || z || (gamma && beta),
                   "bn_bwd_reduce: an activation follows the norm: pass z, or gamma and beta to re-evaluate its argument");
  const int64_t n4 = pixels * (c / 4);
  const StreamShape s = stream_shape(n4, c / 4, reduce_max_blocks());
  static KernelRec rec_br(nullptr, "bn_bwd_reduce_kernel");
  KTimer kt_br(rec_br, as_stream(stream), (double)pixels * c * 4.0 * (z ? 3.0 : 2.0));
  hipLaunchKernelGGL(bn_bwd_reduce_kernel<false>, dim3(s.grid), dim3(s.bs), 0, as_stream(stream), (const f32x4*)dz, (const f32x4*)z,
                     (const f32x4*)y, save_mean, save_rstd, gamma, beta, n4, s.c4, bsums, act, slope);
  UDASEG_LAUNCH_CHECK("bn_bwd_reduce launch");
  return UDASEG_OK;
}

extern "C" int udaseg_bn_bwd_reduce_bf16(const void* dz, const void* z, const void* y, const float* save_mean,
                                         const float* save_rstd, int64_t pixels, int c, double* bsums, int act, float slope,
                                         void* stream) {
  int rc = check_pc(pixels, c, 8, "bn_bwd_reduce_bf16");
  if (rc) return rc;
  UDASEG_CHECK_ARG(dz && y && save_mean && save_rstd && bsums && (act == UDASEG_ACT_NONE || z), "bn_bwd_reduce_bf16: NULL pointer");
  const int64_t n8 = pixels * (c / 8);
  const StreamShape s = stream_shape(n8, c / 8, reduce_max_blocks());
  static KernelRec rec_bn_bwd_reduce_bf16_kernel(nullptr, "bn_bwd_reduce_bf16_kernel");
  KTimer kt_bn_bwd_reduce_bf16_kernel(rec_bn_bwd_reduce_bf16_kernel, as_stream(stream), (double)pixels * c * 2.0 * (act != UDASEG_ACT_NONE ? 3.0 : 2.0));
  hipLaunchKernelGGL(bn_bwd_reduce_kernel<true>, dim3(s.grid), dim3(s.bs), 0, as_stream(stream), (const f32x4*)dz,
                     (const f32x4*)z, (const f32x4*)y, save_mean, save_rstd, (const float*)nullptr, (const float*)nullptr, n8,
                     s.c4, bsums, act, slope);
  UDASEG_LAUNCH_CHECK("bn_bwd_reduce_bf16 launch");
  return UDASEG_OK;
}

extern "C" int udaseg_bn_bwd_apply(const float* dz, const float* z, const float* y, const float* save_mean,
                                   const float* save_rstd, const float* gamma, const float* beta, const double* bsums,
                                   float* dy, float* dres, float* dgamma, float* dbeta, int64_t pixels, int c, int act,
                                   float slope, int accumulate_dy, int accumulate_dres, int accumulate_param,
                                   void* stream) {
  int rc = check_pc(pixels, c, 4, "bn_bwd_apply");
  if (rc) return rc;
  UDASEG_CHECK_ARG(dz && y && save_mean && save_rstd && gamma && bsums && dy, "bn_bwd_apply: NULL pointer");
  UDASEG_CHECK_ARG(act == UDASEG_ACT_NONE || z || beta,
                   "bn_bwd_apply: an activation follows the norm: pass z, or beta to re-evaluate its argument");
  const int64_t n4 = pixels * (c / 4);
  const StreamShape s = stream_shape(n4, c / 4, 2048, apply_per_thread());
  static KernelRec rec_bw(nullptr, "bn_bwd_apply_kernel");
  KTimer kt_bw(rec_bw, as_stream(stream), (double)pixels * c * 4.0 * ((z ? 4.0 : 3.0) + (dres ? 1.0 : 0.0)));
  hipLaunchKernelGGL(bn_bwd_apply_kernel<false>, dim3(s.grid), dim3(s.bs), (size_t)6 * s.c4 * sizeof(float4), as_stream(stream), (const f32x4*)dz, (const f32x4*)z,
                     (const f32x4*)y, save_mean, save_rstd, gamma, beta, bsums, (f32x4*)dy, (f32x4*)dres, dgamma, dbeta, n4, s.c4,
                     pixels, act, slope, accumulate_dy, accumulate_dres, accumulate_param, (const float*)nullptr,
                     (const float*)nullptr);
  UDASEG_LAUNCH_CHECK("bn_bwd_apply launch");
  return UDASEG_OK;
}

extern "C" int udaseg_bn_bwd_apply_bf16(const void* dz, const void* z, const void* y, const float* save_mean,
                                        const float* save_rstd, const float* gamma, const double* bsums, void* dy, void* dres,
                                        float* dgamma, float* dbeta, int64_t pixels, int c, int act, float slope,
                                        int accumulate_dy, int accumulate_dres, int accumulate_param, void* stream) {
  int rc = check_pc(pixels, c, 8, "bn_bwd_apply_bf16");
  if (rc) return rc;
  UDASEG_CHECK_ARG(dz && y && save_mean && save_rstd && gamma && bsums && dy && (act == UDASEG_ACT_NONE || z),
                   "bn_bwd_apply_bf16: NULL pointer");
  static_assert((size_t)5 * UDASEG_BN_BWD_APPLY_BF16_MAX_C * sizeof(float) <= 65536 &&
                (size_t)5 * (UDASEG_BN_BWD_APPLY_BF16_MAX_C + 8) * sizeof(float) > 65536, "the documented maximum is the 64 KB of coefficients");
  UDASEG_CHECK_ARG(c <= UDASEG_BN_BWD_APPLY_BF16_MAX_C, "bn_bwd_apply_bf16: too many channels (%d, at most %d)", c,
                   UDASEG_BN_BWD_APPLY_BF16_MAX_C);
  const int64_t n8 = pixels * (c / 8);
  const StreamShape s = stream_shape(n8, c / 8, 2048, apply_per_thread());
  static KernelRec rec_bwa(nullptr, "bn_bwd_apply_bf16_kernel");
  KTimer kt_bwa(rec_bwa, as_stream(stream), (double)pixels * c * 2.0 * ((act != UDASEG_ACT_NONE ? 4.0 : 3.0) + (dres ? 1.0 : 0.0)));
  hipLaunchKernelGGL(bn_bwd_apply_kernel<true>, dim3(s.grid), dim3(s.bs), (size_t)5 * c * sizeof(float), as_stream(stream),
                     (const f32x4*)dz, (const f32x4*)z, (const f32x4*)y, save_mean, save_rstd, gamma, (const float*)nullptr, bsums,
                     (f32x4*)dy, (f32x4*)dres, dgamma, dbeta, n8, s.c4, pixels, act, slope, accumulate_dy, accumulate_dres,
                     accumulate_param, (const float*)nullptr, (const float*)nullptr);
  UDASEG_LAUNCH_CHECK("bn_bwd_apply_bf16 launch");
  return UDASEG_OK;
}

extern "C" int udaseg_bn_bwd_apply_recompute_bf16(const void* dz, const void* y, const float* fwd_scale, const float* fwd_shift,
                                                  const float* save_mean, const float* save_rstd, const float* gamma,
                                                  const double* bsums, void* dy, float* dgamma, float* dbeta, int64_t pixels, int c,
                                                  int act, float slope, void* stream) {
  int rc = check_pc(pixels, c, 8, "bn_bwd_apply_recompute_bf16");
  if (rc) return rc;
  UDASEG_CHECK_ARG(dz && y && fwd_scale && fwd_shift && save_mean && save_rstd && gamma && bsums && dy,
                   "bn_bwd_apply_recompute_bf16: NULL pointer");
  static_assert((size_t)7 * UDASEG_BN_BWD_RECOMPUTE_BF16_MAX_C * sizeof(float) <= 65536 &&
                (size_t)7 * (UDASEG_BN_BWD_RECOMPUTE_BF16_MAX_C + 8) * sizeof(float) > 65536, "the documented maximum is the 64 KB of coefficients");
  UDASEG_CHECK_ARG(c <= UDASEG_BN_BWD_RECOMPUTE_BF16_MAX_C, "bn_bwd_apply_recompute_bf16: too many channels (%d, at most %d)", c,
                   UDASEG_BN_BWD_RECOMPUTE_BF16_MAX_C);
  const int64_t n8 = pixels * (c / 8);
  const StreamShape s = stream_shape(n8, c / 8, 2048, apply_per_thread());
  static KernelRec rec_bwr(nullptr, "bn_bwd_apply_bf16_kernel");
  KTimer kt_bwr(rec_bwr, as_stream(stream), (double)pixels * c * 2.0 * 3.0);
  hipLaunchKernelGGL(bn_bwd_apply_kernel<true>, dim3(s.grid), dim3(s.bs), (size_t)7 * c * sizeof(float), as_stream(stream),
                     (const f32x4*)dz, (const f32x4*)nullptr, (const f32x4*)y, save_mean, save_rstd, gamma, (const float*)nullptr,
                     bsums, (f32x4*)dy, (f32x4*)nullptr, dgamma, dbeta, n8, s.c4, pixels, act, slope, 0, 0, 0, fwd_scale, fwd_shift);
  UDASEG_LAUNCH_CHECK("bn_bwd_apply_recompute_bf16 launch");
  return UDASEG_OK;
}

extern "C" int udaseg_bn_fold(const float* w, const float* bias, const float* gamma, const float* beta,
                              const float* running_mean, const float* running_var, float eps, int co, int row_len, float* w_folded,
                              float* bias_folded, void* stream) {
  UDASEG_CHECK_ARG(w && gamma && beta && running_mean && running_var && w_folded && bias_folded && co > 0 && row_len > 0,
                   "bn_fold: bad arguments");
  hipLaunchKernelGGL(bn_fold_kernel, dim3(co), dim3(256), 0, as_stream(stream), w, bias, gamma, beta, running_mean, running_var,
                     eps, co, row_len, w_folded, bias_folded);
  UDASEG_LAUNCH_CHECK("bn_fold launch");
  return UDASEG_OK;
}

extern "C" int udaseg_act_bwd(const float* dz, const float* z, float* dy, int64_t count, int act, float slope,
                              void* stream) {
  UDASEG_CHECK_ARG(dz && z && dy && count > 0 && count % 4 == 0, "act_bwd: bad arguments");
  const int64_t n4 = count / 4;
  int grid = (int)((n4 + 1023) / 1024 > 2048 ? 2048 : (n4 + 1023) / 1024);
  hipLaunchKernelGGL(act_bwd_kernel<false>, dim3(grid), dim3(256), 0, as_stream(stream), (const f32x4*)dz, (const f32x4*)z,
                     (f32x4*)dy, n4, act, slope);
  UDASEG_LAUNCH_CHECK("act_bwd launch");
  return UDASEG_OK;
}

extern "C" int udaseg_act_bwd_bf16(const void* dz, const void* z, void* dy, int64_t count, int act, float slope, void* stream) {
  UDASEG_CHECK_ARG(dz && z && dy && count > 0 && count % 8 == 0, "act_bwd_bf16: bad arguments");
  const int64_t n8 = count / 8;
  hipLaunchKernelGGL(act_bwd_kernel<true>, dim3(grid_for(n8)), dim3(256), 0, as_stream(stream), (const f32x4*)dz, (const f32x4*)z,
                     (f32x4*)dy, n8, act, slope);
  UDASEG_LAUNCH_CHECK("act_bwd_bf16 launch");
  return UDASEG_OK;
}

// who: "channel_sum" or "channel_sum_bf16", the name the messages carry
template <bool BF>
static int channel_sum_impl(const char* who, const void* x, int64_t pixels, int c, float* out, int accumulate, float* scratch,
                            size_t scratch_bytes, void* stream) {
  constexpr int N = Vec16<BF>::N;
  int rc = check_pc(pixels, c, N, who);
  if (rc) return rc;
  UDASEG_CHECK_ARG(x && out, "%s: NULL pointer", who);
  char what[64];     // "<call>(<who>)" / "<who> <step>" of a failed HIP call
  auto fail = [&](hipError_t e, const char* fmt) {
    snprintf(what, sizeof(what), fmt, who);
    return hip_fail(e, what);
  };
  hipStream_t st = as_stream(stream);
  const int64_t nq = pixels * (c / N);
  StreamShape s = stream_shape(nq, c / N, reduce_max_blocks());
  if (s.grid <= CHSUM_DIRECT_BLOCKS) {
    if (!accumulate) {
      hipError_t e = hipMemsetAsync(out, 0, (size_t)c * sizeof(float), st);
      if (e != hipSuccess) return fail(e, "hipMemsetAsync(%s)");
    }
    hipLaunchKernelGGL(channel_sum_kernel<BF>, dim3(s.grid), dim3(s.bs), 0, st, (const f32x4*)x, nq, s.c4, out, 1);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? UDASEG_OK : fail(e, "%s launch");
  }
  // replicas of the output in the caller's scratch (stream-ordered ownership is the caller's), or in a stream-ordered allocation
  const size_t rep_bytes = (size_t)CHSUM_REPLICAS * c * sizeof(float);
  float* rep = scratch;
  if (rep != nullptr) {
    UDASEG_CHECK_ARG(scratch_bytes >= rep_bytes, "%s: scratch of %zu bytes, need %zu", who, scratch_bytes, rep_bytes);
  } else {
    hipError_t e = hipMallocAsync(reinterpret_cast<void**>(&rep), rep_bytes, st);
    if (e != hipSuccess) return fail(e, "hipMallocAsync(%s)");
  }
  hipError_t e = hipMemsetAsync(rep, 0, rep_bytes, st);
  hipError_t e1 = hipSuccess, e2 = hipSuccess;
  if (e == hipSuccess) {
    hipLaunchKernelGGL(channel_sum_kernel<BF>, dim3(s.grid), dim3(s.bs), 0, st, (const f32x4*)x, nq, s.c4, rep, CHSUM_REPLICAS);
    e1 = hipGetLastError();
    hipLaunchKernelGGL(fold_replicas_kernel, dim3((c + 255) / 256), dim3(256), 0, st, rep, c, out, accumulate);
    e2 = hipGetLastError();
  }
  hipError_t e3 = scratch == nullptr ? hipFreeAsync(rep, st) : hipSuccess;
  if (e != hipSuccess) return fail(e, "hipMemsetAsync(%s)");
  if (e1 != hipSuccess) return fail(e1, "%s launch");
  if (e2 != hipSuccess) return fail(e2, "%s fold launch");
  if (e3 != hipSuccess) return fail(e3, "hipFreeAsync(%s)");
  return UDASEG_OK;
}

extern "C" size_t udaseg_channel_sum_scratch_bytes(int c) { return c > 0 ? (size_t)CHSUM_REPLICAS * c * sizeof(float) : 0; }

extern "C" int udaseg_channel_sum(const float* x, int64_t pixels, int c, float* out, int accumulate, void* stream) {
  return channel_sum_impl<false>("channel_sum", x, pixels, c, out, accumulate, nullptr, 0, stream);
}

extern "C" int udaseg_channel_sum_ws(const float* x, int64_t pixels, int c, float* out, int accumulate, float* scratch,
                                size_t scratch_bytes, void* stream) {
  UDASEG_CHECK_ARG(scratch != nullptr, "channel_sum_ws: NULL scratch");
  return channel_sum_impl<false>("channel_sum", x, pixels, c, out, accumulate, scratch, scratch_bytes, stream);
}

extern "C" int udaseg_channel_sum_bf16(const void* x, int64_t pixels, int c, float* out, int accumulate, void* stream) {
  return channel_sum_impl<true>("channel_sum_bf16", x, pixels, c, out, accumulate, nullptr, 0, stream);
}

extern "C" int udaseg_channel_sum_bf16_ws(const void* x, int64_t pixels, int c, float* out, int accumulate, float* scratch,
                                size_t scratch_bytes, void* stream) {
  UDASEG_CHECK_ARG(scratch != nullptr, "channel_sum_bf16_ws: NULL scratch");
  return channel_sum_impl<true>("channel_sum_bf16", x, pixels, c, out, accumulate, scratch, scratch_bytes, stream);
}
