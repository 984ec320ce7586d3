// Prototype-rectified pseudo-labels (ProDA, Zhang et al. 2021; an extension: the reference has no feature-space component).
// One prototype per class in the decoder's feature space; a pixel's class probabilities are re-weighted by how close its feature
// lies to each prototype, and pseudo.hip thresholds and labels the re-weighted probabilities.  With torch this is an index_add_
// per batch, a [pixels, C, D] broadcast for the distances, two softmaxes and a normalisation; here it is three entry points:
//   udaseg_proto_accumulate  ONE streaming pass: per-class float64 feature sums, squared norms and pixel counts
//   udaseg_proto_update      one small block: batch mean and spread, first sight or EMA, the temperature (numpy mirror: bit for bit)
//   udaseg_proto_rectify     ONE streaming pass, no atomics: the rectified probabilities as a padded NHWC score buffer
// features: padded NHWC fp32 [pixels][ldf], dim % 4 == 0, 4 <= dim <= 64, dim <= ldf, ldf % 4 == 0; only channels < dim count.
// scores:   [pixels][ldc] as scores_common.h describes, classes <= 32.
//
// Accumulate.  Memory-bound: dim floats and one label byte per pixel, nothing written back per pixel.  Every addition and every
// square is float64 (a feature is widened on load, its square is then exact; a pixel's squared norm is summed over ascending j,
// one number whatever route the pixel takes), so the order of the additions moves a cell by at most n 2^-53 sum|x| and no atomic
// order is visible at the graded tolerance.  Label maps are smooth: 64 consecutive pixels mostly carry one label, or two at a
// boundary, and same-address LDS atomics of a whole wave would serialise 64-fold.  So a wave takes 64 consecutive pixels at a time
// (grid-stride over such chunks: at any moment the waves read one contiguous window, as every other streaming kernel here) and
// handles the classes present one at a time, up to PA_ROUNDS of them: the lanes of that class contribute their features, the
// others zero, and a reduce-scatter over the lanes (half of the values change hands at every step: dim - 1 + log2(64 / dim) double
// shuffles instead of 6 dim) leaves channel j's sum on the lanes that own j, which add it ONCE to the block's [classes][dim]
// float64 table in LDS.  Pixels of further classes (noisy labels) fall back to per-lane LDS float64 atomics.
// Blocks are few and long (conf_hist_kernel's reasoning: a block flushes one global atomic per non-empty cell, so its pixel
// count must be large against classes * dim); a block is 16 waves at dim <= 16 and fewer above, where a lane holds its dim
// widened values in 2 * dim registers.
#include "scores_common.h"

namespace udaseg {

constexpr int PA_CU = 256;

template <int DV>
struct PaShape {
  static constexpr int threads = DV <= 4 ? 1024 : DV <= 8 ? 512 : 256;
  static constexpr int max_blocks = PA_CU * (1024 / threads);
};

constexpr int PA_ROUNDS = 4;

static constexpr int pow2_at_least(int n) { return n <= 4 ? 4 : n <= 8 ? 8 : n <= 16 ? 16 : n <= 32 ? 32 : 64; }

// Reduce-scatter of a[0 .. N) over the wave: at every step a lane keeps one half of its values, hands the other half to the lane
// O away and adds what it receives; with one value left the remaining steps are a butterfly.  Afterwards a[0] is the wave's sum of
// element ch, ch made of the lane's bits 32, 16, ... (N / 2, N / 4, ... each), the same on the 64 / N lanes that differ in the low bits.
template <int N, int O>
struct ReduceScatter {
  static __device__ __forceinline__ void run(double* a, int lane, int& ch) {
    if constexpr (N > 1) {
      constexpr int H = N / 2;
      const bool up = (lane & O) != 0;
#pragma unroll
      for (int i = 0; i < H; ++i) {
        const double send = up ? a[i] : a[i + H];
        const double keep = up ? a[i + H] : a[i];
        a[i] = keep + __shfl_xor(send, O, 64);
      }
      ch += up ? H : 0;
      if constexpr (O > 1) ReduceScatter<H, O / 2>::run(a, lane, ch);
    } else {
      a[0] += __shfl_xor(a[0], O, 64);
      if constexpr (O > 1) ReduceScatter<1, O / 2>::run(a, lane, ch);
    }
  }
};

// key of a pixel: its class, `classes` for a label beyond the classes, classes + 1 for a non-finite feature, -1 past the end
template <int DV>
__global__ __launch_bounds__(PaShape<DV>::threads) void proto_accumulate_kernel(const float* __restrict__ feat, int ldf,
                                                                                const uint8_t* __restrict__ labels, int64_t pixels,
                                                                                int classes, double* __restrict__ sums,
                                                                                double* __restrict__ sq,
                                                                                unsigned long long* __restrict__ counts) {
  constexpr int DIM = 4 * DV;
  constexpr int P2 = pow2_at_least(DIM);                   // the reduce-scatter halves: dims in between are padded with zeros
  constexpr int THREADS = PaShape<DV>::threads;
  constexpr int WAVES = THREADS / 64;
  __shared__ double tab[32 * DIM];
  __shared__ double tsq[32];
  __shared__ unsigned int cnt[34];
  for (int i = threadIdx.x; i < classes * DIM; i += THREADS) tab[i] = 0.0;
  if (threadIdx.x < 32) tsq[threadIdx.x] = 0.0;
  if (threadIdx.x < 34) cnt[threadIdx.x] = 0;
  __syncthreads();

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t chunks = (pixels + 63) >> 6;
  unsigned int nvoid = 0, nbad = 0;                        // wave-uniform
  for (int64_t ch = (int64_t)blockIdx.x * WAVES + wave; ch < chunks; ch += (int64_t)gridDim.x * WAVES) {
    const int64_t p = (ch << 6) + lane;
    int key = -1;
    f32x4 v[DV];
    if (p < pixels) {
      load_row<DV>(feat + p * ldf, v);
      bool fin = true;
#pragma unroll
      for (int q = 0; q < DV; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) fin &= __builtin_isfinite(v[q][e]);
      const int lab = labels[p];
      key = !fin ? classes + 1 : lab < classes ? lab : classes;
    } else {
#pragma unroll
      for (int q = 0; q < DV; ++q) v[q] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    nvoid += (unsigned int)__popcll(__ballot(key == classes));
    nbad += (unsigned int)__popcll(__ballot(key == classes + 1));
    unsigned long long todo = __ballot(key >= 0 && key < classes);
    for (int round = 0; todo && round < PA_ROUNDS; ++round) {          // wave-uniform: one class of the chunk per round
      const int k = __shfl(key, __ffsll((long long)todo) - 1, 64);
      const bool mine = key == k;
      double a[P2];
      double s2 = 0.0;                                     // the pixel's squared norm: ascending j
#pragma unroll
      for (int j = 0; j < P2; ++j) {
        const double d = (j < DIM && mine) ? (double)v[j >> 2][j & 3] : 0.0;
        a[j] = d;
        s2 += d * d;                                       // d * d is exact in float64: fusing it into the addition changes nothing
      }
      int chn = 0;
      ReduceScatter<P2, 32>::run(a, lane, chn);
      s2 = wave_sum_d(s2);
      const unsigned long long m = __ballot(mine);
      if ((lane & (64 / P2 - 1)) == 0 && chn < DIM) atomicAdd(&tab[k * DIM + chn], a[0]);
      if (lane == 0) {
        atomicAdd(&tsq[k], s2);
        atomicAdd(&cnt[k], (unsigned int)__popcll(m));
      }
      todo &= ~m;
    }
    if ((todo >> lane) & 1ull) {                           // more than PA_ROUNDS classes in 64 pixels: per-lane atomics
      double s2 = 0.0;
#pragma unroll
      for (int q = 0; q < DV; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const double d = (double)v[q][e];
          atomicAdd(&tab[key * DIM + 4 * q + e], d);
          s2 += d * d;
        }
      atomicAdd(&tsq[key], s2);
      atomicAdd(&cnt[key], 1u);
    }
  }
  // Written out, not BlockCounts (common.h): the two counts are wave sums already (ballots, in scalar registers), and carried through
  // BlockCounts::put the register allocation of DV = 7 and 9 moved from three waves a SIMD to two (profiles/block_counts_refactor.txt).
  if (lane == 0) {
    if (nvoid) atomicAdd(&cnt[32], nvoid);
    if (nbad) atomicAdd(&cnt[33], nbad);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < classes * DIM; i += THREADS)
    if (cnt[i / DIM]) {
      const double s = tab[i];
      if (s != 0.0) atomicAdd(&sums[i], s);
    }
  if (threadIdx.x < classes) {
    if (cnt[threadIdx.x]) {
      atomicAdd(&sq[threadIdx.x], tsq[threadIdx.x]);
      atomicAdd(&counts[threadIdx.x], (unsigned long long)cnt[threadIdx.x]);
    }
  } else if (threadIdx.x < classes + 2) {
    const unsigned int n = cnt[32 + threadIdx.x - classes];
    if (n) atomicAdd(&counts[threadIdx.x], (unsigned long long)n);
  }
}

// One block, thread c owns class c (threads classes, classes + 1 the two extra counters); thread 0 finishes with the temperature.
// Contraction is switched off for the body, so every product and every sum is rounded on its own (hipcc fuses a * b + c by
// default): proto.update_mirror is this function in numpy float64, bit for bit.
constexpr int PU_THREADS = 64;

__global__ __launch_bounds__(PU_THREADS) void proto_update_kernel(double* __restrict__ sums, double* __restrict__ sq,
                                                                  long long* __restrict__ counts, int classes, int dim,
                                                                  double momentum, long long min_pixels, double tau_scale, int clear,
                                                                  double* __restrict__ proto, double* __restrict__ spread,
                                                                  int* __restrict__ seen, long long* __restrict__ last_counts,
                                                                  float* __restrict__ inv_tau) {
#pragma clang fp contract(off)
  __shared__ double sp[32];
  __shared__ int sn[32];
  const int c = threadIdx.x;
  if (c < classes) {
    const long long n = counts[c];
    double* su = sums + (size_t)c * dim;
    double* pr = proto + (size_t)c * dim;
    int was = seen[c];
    double spr = spread[c];
    if (n >= min_pixels) {
      const double dn = (double)n;
      double msq = 0.0;
      for (int j = 0; j < dim; ++j) {
        const double m = su[j] / dn;
        const double mm = m * m;
        msq = msq + mm;
      }
      const double diff = sq[c] / dn - msq;
      const double s = diff > 0.0 ? diff : 0.0;
      if (!was) {
        for (int j = 0; j < dim; ++j) pr[j] = su[j] / dn;
        spr = s;
        was = 1;
        seen[c] = 1;
      } else {
        const double om = 1.0 - momentum;
        for (int j = 0; j < dim; ++j) {
          const double a = momentum * pr[j];
          const double b = om * (su[j] / dn);
          pr[j] = a + b;
        }
        const double a = momentum * spr;
        const double b = om * s;
        spr = a + b;
      }
      spread[c] = spr;
    }
    sp[c] = spr;
    sn[c] = was;
    if (clear) {
      for (int j = 0; j < dim; ++j) su[j] = 0.0;
      sq[c] = 0.0;
    }
  }
  if (c < classes + 2) {
    last_counts[c] = counts[c];
    if (clear) counts[c] = 0;
  }
  __syncthreads();
  if (c == 0 && tau_scale > 0.0) {
    double tot = 0.0;
    int ns = 0;
    for (int k = 0; k < classes; ++k)
      if (sn[k]) {
        tot = tot + sp[k];
        ++ns;
      }
    const double t = tau_scale * (tot / (double)ns);
    inv_tau[0] = (__builtin_isfinite(t) && t > 0.0) ? (float)(1.0 / t) : 0.f;
  }
}

// One lane per pixel.  The block stages the prototypes once as fp32 in LDS; every lane of a wave reads the same prototype words
// (a broadcast), its own feature row once and its own score row once.  d_c is summed in four chains, channel j in chain j % 4,
// folded as (s0 + s1) + (s2 + s3) -- pixel_conf's form, a fraction of one chain's rounding; S and R likewise over the classes.
constexpr int PR_THREADS = 256;
constexpr int PR_MAX_BLOCKS = 4096;

template <int NV>
__global__ __launch_bounds__(PR_THREADS) void proto_rectify_kernel(const float* __restrict__ feat, int ldf, int dim,
                                                                   const float* __restrict__ scores, int ldc, int classes, int probs,
                                                                   const double* __restrict__ proto, const int* __restrict__ seen,
                                                                   const float* __restrict__ inv_tau, int64_t pixels,
                                                                   float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float P[32 * 64];
  __shared__ unsigned int seen_mask;
  if (threadIdx.x == 0) {
    unsigned int m = 0;
    for (int c = 0; c < classes; ++c) m |= (seen[c] != 0 ? 1u : 0u) << c;
    seen_mask = m;
  }
  // the classes beyond `classes` of the last vector get zero prototypes: their distances are computed and never used, and
  // the loop over the channels has no branch
  for (int i = threadIdx.x; i < 4 * NV * dim; i += PR_THREADS) P[i] = i < classes * dim ? (float)proto[i] : 0.f;
  __syncthreads();
  const unsigned int sm = seen_mask;
  const unsigned int all = classes >= 32 ? 0xffffffffu : (1u << classes) - 1u;
  const unsigned int live = sm ? sm : all;                 // the classes that can get a probability
  const bool weigh = sm != 0u;
  const float it = inv_tau[0];
  const int dv = dim >> 2, lv = ldc >> 2;
  const float qnan = __builtin_nanf("");
  for (int64_t p = (int64_t)blockIdx.x * PR_THREADS + threadIdx.x; p < pixels; p += (int64_t)gridDim.x * PR_THREADS) {
    f32x4 d4[4 * NV];
#pragma unroll
    for (int c = 0; c < 4 * NV; ++c) d4[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    bool ok = true;
    const float* frow = feat + p * ldf;
#pragma unroll 1
    for (int q = 0; q < dv; ++q) {                         // rolled: 4 * NV accumulator vectors are live across it
      const f32x4 f = *reinterpret_cast<const f32x4*>(frow + 4 * q);
      ok &= __builtin_isfinite(f[0]) & __builtin_isfinite(f[1]) & __builtin_isfinite(f[2]) & __builtin_isfinite(f[3]);
      const float* pq = P + 4 * q;
#pragma unroll
      for (int c = 0; c < 4 * NV; ++c) {
        const f32x4 t = f - *reinterpret_cast<const f32x4*>(pq + c * dim);
#pragma unroll
        for (int e = 0; e < 4; ++e) d4[c][e] = fmaf(t[e], t[e], d4[c][e]);
      }
    }
    float d[4 * NV];
    float dmin = INFINITY;
#pragma unroll
    for (int c = 0; c < 4 * NV; ++c) {
      d[c] = (d4[c][0] + d4[c][1]) + (d4[c][2] + d4[c][3]);
      dmin = ((sm >> c) & 1u) ? fminf(dmin, d[c]) : dmin;
    }
    // p_c
    f32x4 v[NV];
    load_row<NV>(scores + p * ldc, v);
    float m;
    first_max<NV>(v, classes, m);
    f32x4 s4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < NV; ++q)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool in = ((all >> (4 * q + e)) & 1u) != 0u;
        const float x = v[q][e];
        ok &= !in || (probs ? (x >= 0.f && x <= 1.f) : __builtin_isfinite(x));
        const float pe = probs ? x : expf(x - m);
        v[q][e] = in ? pe : 0.f;
        s4[e] += v[q][e];
      }
    const float inv_s = probs ? 1.f : 1.f / ((s4[0] + s4[1]) + (s4[2] + s4[3]));
    // u_c, r_c
    f32x4 r4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < NV; ++q)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int c = 4 * q + e;
        const float pc = probs ? v[q][e] : v[q][e] * inv_s;
        const float u = weigh ? expf(-(d[c] - dmin) * it) : 1.f;
        const float r = ((live >> c) & 1u) ? pc * u : 0.f;
        v[q][e] = r;
        r4[e] += r;
      }
    const float R = (r4[0] + r4[1]) + (r4[2] + r4[3]);
    ok &= __builtin_isfinite(R) && R > 0.f;
    float* orow = out + p * ldc;
#pragma unroll
    for (int q = 0; q < NV; ++q) {
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = ((all >> (4 * q + e)) & 1u) ? (ok ? v[q][e] / R : qnan) : 0.f;
      *reinterpret_cast<f32x4*>(orow + 4 * q) = o;
    }
    for (int q = NV; q < lv; ++q) *reinterpret_cast<f32x4*>(orow + 4 * q) = f32x4{0.f, 0.f, 0.f, 0.f};
  }
}

}  // namespace udaseg

using namespace udaseg;

extern "C" int udaseg_proto_accumulate(const float* feat, int ldf, int dim, const uint8_t* labels, int64_t pixels, int classes,
                                       double* sums, double* sq, int64_t* counts, void* stream) {
  if (!proto_feat_ok("proto_accumulate", pixels, classes, dim, ldf)) return UDASEG_E_BADARG;
  UDASEG_CHECK_ARG(feat && labels && sums && sq && counts, "proto_accumulate: NULL pointer");
  UDASEG_CHECK_ARG((reinterpret_cast<uintptr_t>(feat) & 15) == 0, "proto_accumulate: feat must be 16-byte aligned");
  const int64_t chunks = cdiv64(pixels, 64);
  if (!dispatch_width<16>(dim / 4, [&](auto w) {
        constexpr int DV = decltype(w)::value;
        const int gx = capped_grid(chunks, PaShape<DV>::threads / 64, PaShape<DV>::max_blocks);
        hipLaunchKernelGGL(proto_accumulate_kernel<DV>, dim3(gx), dim3(PaShape<DV>::threads), 0, as_stream(stream), feat, ldf, labels,
                           pixels, classes, sums, sq, (unsigned long long*)counts);
      }))
    return unsupported_width("proto_accumulate", "dim", dim);
  UDASEG_LAUNCH_CHECK("proto_accumulate launch");
  return UDASEG_OK;
}

extern "C" int udaseg_proto_update(double* sums, double* sq, int64_t* counts, int classes, int dim, double momentum,
                                   int64_t min_pixels, double tau_scale, int clear, double* proto, double* spread, int32_t* seen,
                                   int64_t* last_counts, float* inv_tau, void* stream) {
  if (!proto_dims_ok("proto_update", classes, dim)) return UDASEG_E_BADARG;
  UDASEG_CHECK_ARG(momentum >= 0.0 && momentum <= 1.0, "proto_update: need 0 <= momentum <= 1 (momentum=%g)", momentum);
  UDASEG_CHECK_ARG(min_pixels >= 1, "proto_update: need min_pixels >= 1 (min_pixels=%lld)", (long long)min_pixels);
  UDASEG_CHECK_ARG(tau_scale == tau_scale && tau_scale < INFINITY, "proto_update: tau_scale must be a finite number or <= 0");
  UDASEG_CHECK_ARG(sums && sq && counts && proto && spread && seen && last_counts && inv_tau, "proto_update: NULL pointer");
  hipLaunchKernelGGL(proto_update_kernel, dim3(1), dim3(PU_THREADS), 0, as_stream(stream), sums, sq, (long long*)counts, classes, dim,
                     momentum, (long long)min_pixels, tau_scale, clear, proto, spread, seen, (long long*)last_counts, inv_tau);
  UDASEG_LAUNCH_CHECK("proto_update launch");
  return UDASEG_OK;
}

extern "C" int udaseg_proto_rectify(const float* feat, int ldf, int dim, const float* scores, int ldc, int classes, int probs,
                                    const double* proto, const int32_t* seen, const float* inv_tau, int64_t pixels, float* out,
                                    void* stream) {
  if (!proto_feat_ok("proto_rectify", pixels, classes, dim, ldf)) return UDASEG_E_BADARG;
  if (!scores_args_ok("proto_rectify", pixels, classes, ldc)) return UDASEG_E_BADARG;
  UDASEG_CHECK_ARG(probs == 0 || probs == 1, "proto_rectify: probs must be 0 (logits) or 1 (probabilities), got %d", probs);
  UDASEG_CHECK_ARG(feat && scores && proto && seen && inv_tau && out, "proto_rectify: NULL pointer");
  UDASEG_CHECK_ARG(((reinterpret_cast<uintptr_t>(feat) | reinterpret_cast<uintptr_t>(scores) | reinterpret_cast<uintptr_t>(out)) & 15) == 0,
                   "proto_rectify: feat, scores and out must be 16-byte aligned");
  const int gx = capped_grid(pixels, PR_THREADS, PR_MAX_BLOCKS);
  if (!dispatch_width<8>(cdiv(classes, 4), [&](auto w) {
        hipLaunchKernelGGL(proto_rectify_kernel<decltype(w)::value>, dim3(gx), dim3(PR_THREADS), 0, as_stream(stream), feat, ldf, dim,
                           scores, ldc, classes, probs, proto, seen, inv_tau, pixels, out);
      }))
    return unsupported_width("proto_rectify", "classes", classes);
  UDASEG_LAUNCH_CHECK("proto_rectify launch");
  return UDASEG_OK;
}
