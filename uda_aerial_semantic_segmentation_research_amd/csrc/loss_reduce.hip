// The finish kernels of the scalar-loss family, defined once (loss_reduce.h has the launchers' contracts and the whole order).
#include "loss_reduce.h"

namespace udaseg {

// single wave: the deterministic final sum, one divide.  D == 0 under a device denominator (all void, only zero-weight classes,
// every weight void): NaN, whatever the partials sum to -- torch's 0 / 0 in a weighted mean.
__global__ void loss_finish_kernel(const double* __restrict__ partials, int n, double divisor, const double* __restrict__ denom,
                                   float* __restrict__ out, int accumulate) {
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 64) s += partials[i];
  s = wave_sum_d(s);
  if (threadIdx.x == 0) {
    const float v = denom ? (*denom == 0.0 ? NAN : (float)(s / *denom)) : (float)(s / divisor);
    *out = accumulate ? *out + v : v;
  }
}

// one 256-thread block per column, fixed-order tree => deterministic
__global__ __launch_bounds__(256) void colsum_finish_kernel(const float* __restrict__ colpart, int nblocks, int ldc,
                                                            float* __restrict__ colsum, int accumulate) {
  __shared__ float red[4];
  const int c = blockIdx.x;
  float s = 0.f;
  for (int b = threadIdx.x; b < nblocks; b += 256) s += colpart[(size_t)b * ldc + c];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float t = (red[0] + red[1]) + (red[2] + red[3]);
    colsum[c] = accumulate ? colsum[c] + t : t;
  }
}

// single wave over partials[K][n]: row 0 is an f64 sum, rows 1 .. K-1 are whole numbers < 2^53 (exact in f64)
template <int K>
__global__ void rows_finish_kernel(const double* __restrict__ partials, int n, double* __restrict__ denom,
                                   int64_t* __restrict__ counts) {
  double s[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    double a = 0.0;
    for (int i = threadIdx.x; i < n; i += 64) a += partials[(size_t)k * n + i];
    s[k] = wave_sum_d(a);
  }
  if (threadIdx.x == 0) {
    *denom = s[0];
#pragma unroll
    for (int k = 1; k < K; ++k) counts[k - 1] = (int64_t)s[k];
  }
}

int launch_loss_finish(const double* partials, int n, double divisor, const double* denom, float* out, int accumulate, hipStream_t st,
                       const char* what) {
  hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(64), 0, st, partials, n, divisor, denom, out, accumulate);
  UDASEG_LAUNCH_CHECK(what);
  return UDASEG_OK;
}

int launch_colsum_finish(const float* colpart, int nblocks, int ldc, float* colsum, int accumulate, hipStream_t st, const char* what) {
  hipLaunchKernelGGL(colsum_finish_kernel, dim3(ldc), dim3(256), 0, st, colpart, nblocks, ldc, colsum, accumulate);
  UDASEG_LAUNCH_CHECK(what);
  return UDASEG_OK;
}

int launch_rows_finish(int rows, const double* partials, int n, double* denom, int64_t* counts, hipStream_t st, const char* what) {
  UDASEG_CHECK_ARG(rows == 3 || rows == 4, "%s: %d rows of partials", what, rows);
  hipLaunchKernelGGL((rows == 4 ? rows_finish_kernel<4> : rows_finish_kernel<3>), dim3(1), dim3(64), 0, st, partials, n, denom, counts);
  UDASEG_LAUNCH_CHECK(what);
  return UDASEG_OK;
}

}  // namespace udaseg
