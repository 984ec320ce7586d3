// What comes after the row arithmetic of a scalar loss (losses.hip, losses_seg.hip, advent.hip, distill.hip, proto_contrast.hip):
// the block's f64 partial, the 256-pixel LDS gradient tile with its column sums, and the single-wave finish kernels.  The loss
// kernels promise a fixed pixel-to-thread map and a fixed summation order -- two calls give the same bits, CrossEntropyLoss()
// equals the plain launches bit for bit -- and THE ORDER IS DEFINED HERE AND IN loss_reduce.hip (soft_ce_kernel alone restates the tile):
//   thread -> wave:    wave_sum_d, the xor butterfly with offsets 32 ... 1
//   wave -> block:     block_partial       red[0] + red[1] + red[2] + red[3]          (left to right)
//                      block_partial_rows  (red[k][0] + red[k][1]) + (red[k][2] + red[k][3])   (pairwise; other bits, kept apart)
//   block -> scalar:   loss_finish_kernel / rows_finish_kernel: lane l sums partials[l], partials[l + 64], ..., then wave_sum_d
//   columns:           GradTile: row group rg adds rows rg, rg + NG, ...; then the groups g2 = 0 .. NG - 1 in order;
//                      colsum_finish_kernel: thread t adds blocks t, t + 256, ..., wave_sum, (r0 + r1) + (r2 + r3)
// tests/test_gpu_loss_finish.py restates these trees on the host and compares bits.
// Every helper is for 256-thread blocks, and every barrier in it is reached by all threads of the block or by none: a caller
// keeps its own conditions around a call uniform.
#pragma once
#include "scores_common.h"

namespace udaseg {

// The row arithmetic the optioned cross entropy (losses.hip) and the hard-pixel-mining cross entropy (ohem.hip) share.
// valid(p): the target names a class and is not ignore_index.
__device__ __forceinline__ bool ce_valid(int64_t t, int classes, int has_ignore, int64_t ignore_index) {
  return (uint64_t)t < (uint64_t)classes && !(has_ignore && t == ignore_index);
}
// lse = mx + logf(sum_c expf(z_c - mx)) with the classes summed left to right; xt = z_t.
template <int LDC4>
__device__ __forceinline__ float ce_row_lse(const f32x4 (&v)[LDC4], int classes, int t, float& xt) {
  float mx = -INFINITY;
#pragma unroll
  for (int k = 0; k < LDC4; ++k)
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (k * 4 + e < classes) mx = fmaxf(mx, v[k][e]);
  float sum = 0.f;
  xt = 0.f;
#pragma unroll
  for (int k = 0; k < LDC4; ++k)
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (k * 4 + e < classes) {
        sum += expf(v[k][e] - mx);
        if (k * 4 + e == t) xt = v[k][e];
      }
  return mx + logf(sum);
}

// partials[blockIdx.x] = the block's sum of `local`.  red: 4 doubles of LDS.  One barrier.
__device__ __forceinline__ void block_partial(double local, double* red, double* partials) {
  local = wave_sum_d(local);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = local;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// partials[k][blockIdx.x] = the block's sum of v[k], k < K (the denominator and whole-number counters of a statistics pass).
template <int K>
__device__ __forceinline__ void block_partial_rows(double (&v)[K], double (&red)[K][4], double* partials) {
#pragma unroll
  for (int k = 0; k < K; ++k) {
    v[k] = wave_sum_d(v[k]);
    if ((threadIdx.x & 63) == 0) red[k][threadIdx.x >> 6] = v[k];
  }
  __syncthreads();
  if (threadIdx.x < K) {
    const int k = threadIdx.x;
    partials[(size_t)k * gridDim.x + blockIdx.x] = (red[k][0] + red[k][1]) + (red[k][2] + red[k][3]);
  }
}

// The gradient of a 256-pixel chunk on its way out (ldc <= 32): each thread puts its pixel's row (or a zero row) into the LDS
// tile, so the HBM stores are whole contiguous lines (per-thread 96-B-strided 16-B stores ran at 1.7 TB/s), and the same tile
// yields the per-class column sums = the segmentation head's bias gradient (saves a separate 200 MB pass).
// The kernel declares the two arrays, so that its LDS reads off its own source, and hands them to every call:
//   __shared__ __attribute__((aligned(16))) float tile[256 * Tile::LDC];   __shared__ float colred[Tile::NG * Tile::LDC];
// Thread tid holds pixel tid of the chunk; for the column sums it adds column cc = tid % LDC over the rows of group rg = tid / LDC.
// soft_ce_kernel (distill.hip) keeps this tile written out, for the reasons given there; the four cross-entropy kernels use it.
template <int LDC4>
struct GradTile {
  static constexpr int LDC = LDC4 * 4;
  static constexpr int NG = 256 / LDC;  // row groups for the column sums
  typedef float Rows[256 * LDC];
  typedef float Cols[NG * LDC];

  static __device__ __forceinline__ void put(Rows& tile, int k, f32x4 g) {
    const int tid = threadIdx.x;
    *reinterpret_cast<f32x4*>(tile + tid * LDC + k * 4) = g;
  }
  static __device__ __forceinline__ void put_zero(Rows& tile) {
#pragma unroll
    for (int k = 0; k < LDC4; ++k) put(tile, k, f32x4{0.f, 0.f, 0.f, 0.f});
  }
  // between the two barriers of a chunk: the tile as contiguous lines, and this thread's column over its row group
  static __device__ __forceinline__ void store_lines(const Rows& tile, int64_t chunk, int64_t pixels, f32x4* dlogits) {
    const int tid = threadIdx.x;
    const int64_t base4 = chunk * 256 * LDC4, lim4 = pixels * LDC4;
#pragma unroll
    for (int it = 0; it < LDC4; ++it) {
      const int idx = it * 256 + tid;
      if (base4 + idx < lim4) dlogits[base4 + idx] = reinterpret_cast<const f32x4*>(tile)[idx];
    }
  }
  static __device__ __forceinline__ void add_columns(const Rows& tile, float& colacc) {
    const int tid = threadIdx.x, cc = tid % LDC, rg = tid / LDC;
    if (rg < NG)
      for (int r = rg; r < 256; r += NG) colacc += tile[r * LDC + cc];
  }
  // barrier, line stores, column accumulation, barrier
  static __device__ __forceinline__ void flush(const Rows& tile, int64_t chunk, int64_t pixels, f32x4* dlogits, bool colpart_wanted,
                                               float& colacc) {
    __syncthreads();
    store_lines(tile, chunk, pixels, dlogits);
    if (colpart_wanted) add_columns(tile, colacc);
    __syncthreads();
  }
  // after the chunk loop: the row groups' sums into colred, a barrier of the CALLER's (its own, or the loss epilogue's), then
  // colpart[blockIdx.x][.] in the fixed order g2 = 0 .. NG - 1
  static __device__ __forceinline__ void put_columns(Cols& colred, float colacc) {
    const int tid = threadIdx.x, cc = tid % LDC, rg = tid / LDC;
    if (rg < NG) colred[rg * LDC + cc] = colacc;
  }
  static __device__ __forceinline__ void write_columns(const Cols& colred, float* colpart) {
    const int tid = threadIdx.x;
    if (tid < LDC) {
      float s = 0.f;
      for (int g2 = 0; g2 < NG; ++g2) s += colred[g2 * LDC + tid];
      colpart[(size_t)blockIdx.x * LDC + tid] = s;
    }
  }
  static __device__ __forceinline__ void finish(Cols& colred, float* colpart, float colacc) {
    put_columns(colred, colacc);
    __syncthreads();
    write_columns(colred, colpart);
  }
};

// ---- the finish kernels (loss_reduce.hip), each a launch plus its check; `what` names the caller in udaseg_last_error ----------
// *out (+)= denom ? (*denom == 0 ? NaN : sum / *denom) : sum / divisor, as fp32;  sum = the n partials in the fixed order
int launch_loss_finish(const double* partials, int n, double divisor, const double* denom, float* out, int accumulate, hipStream_t st,
                       const char* what);
// colsum[c] (+)= sum over the nblocks blocks of colpart[b][c], c < ldc
int launch_colsum_finish(const float* colpart, int nblocks, int ldc, float* colsum, int accumulate, hipStream_t st,
                         const char* what = "colsum_finish launch");
// partials[rows][n] (rows 3 or 4): *denom = sum of row 0, counts[k - 1] = (int64) sum of row k
int launch_rows_finish(int rows, const double* partials, int n, double* denom, int64_t* counts, hipStream_t st, const char* what);

}  // namespace udaseg
