// Device-side frame ingest: the step between a decoded frame of any size and the uint8 batch at the model's size that the
// augmentation kernels take (the reference does it per sample on the host: cv2.resize(INTER_AREA) in
// src/data/target_dataset.py:46-48, Resize(Config.IMAGE_SIZE) in src/models/predict.py:91-98, the mask statistics of
// src/data/dataset.py:48-111).  Four entry points, definitions in include/udaseg.h:
//   udaseg_resize_area_u8     exact integer box filter, uint8 -> uint8
//   udaseg_resize_aa_u8       antialiased bilinear from host-built tap tables, fused with A.Normalize -> padded NHWC fp32 / bf16
//   udaseg_resize_nearest_u8  label masks
//   udaseg_mask_hist_u8       per-mask histogram of the 256 byte values
//
// The two filters are separable and share one kernel, VERTICAL PASS FIRST.  A block owns one destination row and `jb`
// destination pixels of it; the source columns under them are walked in pieces of RS_CHUNK bytes (341 pixels):
//   1. vertical: lane l of every wave owns 16 source bytes of the piece and adds them up over the source rows under the
//      destination row, weighted by the row weights; the four waves take every fourth row (so a destination of few pixels
//      still has four rows in flight per block) and their partial columns are summed through LDS.  Each source byte is read
//      from memory exactly once per destination row that it lies under, as part of a 16-byte load.
//   2. horizontal: the summed column (u32 / fp32 per source byte, in LDS) is shared by the destination pixels that straddle
//      it; four lanes per destination pixel take every fourth source pixel and fold with two shuffles.
// Source rows are 3 W bytes: neither 16-byte aligned nor a multiple of 16.  A lane's 16 bytes are read as the five dwords that
// hold them (dword-aligned dwordx4 + dword) and shifted into place; the shift is the same for a whole row.  Only the lanes whose
// five dwords would reach past the end of the tensor (the tail of its last row) read byte by byte.
//
// Area mode is integer arithmetic throughout.  With row weights summing to H (each <= h) a column sum is <= 255 H, a u32
// (H <= 16843009 is checked); rows
// of full weight h -- all but the first and last under a destination row -- are added as two 16-bit fields per dword and
// multiplied by h once per 256 rows.  The horizontal sum reaches 255 H W (4000 x 6000: 6.1e9 > 2^32) and is u64, as is the
// final rounding division.
#include <type_traits>

#include "common.h"

namespace udaseg {

constexpr int RS_THREADS = 256;
constexpr int RS_WAVES = 4;
constexpr int RS_CHUNK = 1024;               // source bytes of one piece: 64 lanes x 16 bytes
constexpr int RS_CHUNK_PX = RS_CHUNK / 3;    // 341 whole pixels
constexpr int RS_MAX_JB = RS_CHUNK_PX;       // destination pixels of one block (their totals live in LDS)
constexpr int RS_PACK_ROWS = 256;            // 256 x 255 < 2^16

enum { RS_AREA = 0, RS_AA_F32 = 1, RS_AA_BF16 = 2 };

// the 16 bytes at a (any alignment) as four little-endian dwords; nothing at or past `end` is touched by the byte path, and
// the dword path is taken only when its five dwords end before `end`
__device__ __forceinline__ void load_window(const uint8_t* __restrict__ a, const uint8_t* __restrict__ end, uint32_t (&d)[4]) {
  if (a + 20 <= end) {
    const unsigned p = (unsigned)((uintptr_t)a & 3);
    const uint32_t* q = reinterpret_cast<const uint32_t*>(a - p);
    const uint32_t r0 = q[0], r1 = q[1], r2 = q[2], r3 = q[3], r4 = q[4];
    const unsigned sh = 8 * p;
    d[0] = (uint32_t)((((uint64_t)r1 << 32) | r0) >> sh);
    d[1] = (uint32_t)((((uint64_t)r2 << 32) | r1) >> sh);
    d[2] = (uint32_t)((((uint64_t)r3 << 32) | r2) >> sh);
    d[3] = (uint32_t)((((uint64_t)r4 << 32) | r3) >> sh);
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      uint32_t v = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (a + 4 * q + k < end) v |= (uint32_t)a[4 * q + k] << (8 * k);
      d[q] = v;
    }
  }
}

__device__ __forceinline__ void add_weighted(uint32_t (&acc)[16], const uint32_t (&d)[4], uint32_t wy) {
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[4 * q + k] += wy * ((d[q] >> (8 * k)) & 255u);
}
__device__ __forceinline__ void add_weighted(float (&acc)[16], const uint32_t (&d)[4], float wy) {
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[4 * q + k] += wy * (float)((d[q] >> (8 * k)) & 255u);
}
// bytes 0 / 2 of every dword into the two 16-bit fields of pk[2q], bytes 1 / 3 into those of pk[2q + 1]
__device__ __forceinline__ void add_packed(uint32_t (&pk)[8], const uint32_t (&d)[4]) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    pk[2 * q] += d[q] & 0x00FF00FFu;
    pk[2 * q + 1] += (d[q] >> 8) & 0x00FF00FFu;
  }
}
__device__ __forceinline__ void flush_packed(uint32_t (&acc)[16], uint32_t (&pk)[8], uint32_t wy) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    acc[4 * q + 0] += wy * (pk[2 * q] & 0xFFFFu);
    acc[4 * q + 2] += wy * (pk[2 * q] >> 16);
    acc[4 * q + 1] += wy * (pk[2 * q + 1] & 0xFFFFu);
    acc[4 * q + 3] += wy * (pk[2 * q + 1] >> 16);
    pk[2 * q] = pk[2 * q + 1] = 0;
  }
}

// overlap of destination cell j, [j L, (j + 1) L), with source cell s, [s l, (s + 1) l), in units of 1 / (L l) of the axis
// (L source cells, l destination cells; L l < 2^31)
__device__ __forceinline__ uint32_t box_weight(int j, int s, int L, int l) {
  const uint32_t a = max((uint32_t)j * L, (uint32_t)s * l), b = min((uint32_t)(j + 1) * L, (uint32_t)(s + 1) * l);
  return b - a;
}

template <int MODE>
__global__ __launch_bounds__(RS_THREADS) void resize_sep_kernel(const uint8_t* __restrict__ src, const uint8_t* __restrict__ end,
                                                                int H, int W, int h, int w, int jb,
                                                                const int32_t* __restrict__ y_start, const float* __restrict__ y_w,
                                                                int y_taps, const int32_t* __restrict__ x_start,
                                                                const float* __restrict__ x_w, int x_taps, Normalize3 nm,
                                                                void* __restrict__ out, int cpad) {
  constexpr bool AA = MODE != RS_AREA;
  using TA = typename std::conditional<AA, float, uint32_t>::type;       // one column of the vertical pass
  using TT = typename std::conditional<AA, float, uint64_t>::type;       // one destination channel
  __shared__ TA part[RS_WAVES][RS_CHUNK];
  __shared__ TT tot[RS_MAX_JB * 3];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int i = blockIdx.y, ni = blockIdx.z;
  const int j0 = blockIdx.x * jb, nj = min(w, j0 + jb) - j0;
  const uint8_t* img = src + (size_t)ni * H * W * 3;
  // source rows [s0, s1) under destination row i, source pixels [t0, t1) under the block's destination pixels
  int s0, s1, t0, t1;
  if (AA) {
    s0 = y_start[i];
    s1 = min(s0 + y_taps, H);
    t0 = max(x_start[j0], 0);
    t1 = min(x_start[j0 + nj - 1] + x_taps, W);
  } else {
    s0 = (int)(((int64_t)i * H) / h);
    s1 = (int)(((int64_t)(i + 1) * H + h - 1) / h);
    t0 = (int)(((int64_t)j0 * W) / w);
    t1 = (int)(((int64_t)(j0 + nj) * W + w - 1) / w);
  }
  for (int o = tid; o < nj * 3; o += RS_THREADS) tot[o] = 0;
  __syncthreads();

  for (int ta = t0; ta < t1; ta += RS_CHUNK_PX) {
    const int tb = min(t1, ta + RS_CHUNK_PX);
    const int nb = 3 * (tb - ta);
    // ---- vertical pass: this wave's rows, this lane's 16 bytes
    TA acc[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0;
    if (16 * lane < nb) {
      const uint8_t* col = img + (size_t)ta * 3 + 16 * lane;
      uint32_t d[4];
      if constexpr (AA) {
        for (int a = wv; a < y_taps; a += RS_WAVES) {
          const int s = s0 + a;
          if (s < 0 || s >= s1) continue;
          load_window(col + (size_t)s * W * 3, end, d);
          add_weighted(acc, d, y_w[(size_t)i * y_taps + a]);
        }
      } else {
        uint32_t pk[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        int held = 0;
        auto add_row = [&](const uint32_t (&v)[4], int s) {
          const uint32_t wy = box_weight(i, s, H, h);
          if (wy == (uint32_t)h) {                           // the same for the whole wave
            add_packed(pk, v);
            if (++held == RS_PACK_ROWS) {
              flush_packed(acc, pk, (uint32_t)h);
              held = 0;
            }
          } else {
            add_weighted(acc, v, wy);
          }
        };
        uint32_t d2[4];
        for (int s = s0 + wv; s < s1; s += 2 * RS_WAVES) {   // two rows in flight per wave
          const bool two = s + RS_WAVES < s1;
          load_window(col + (size_t)s * W * 3, end, d);
          if (two) load_window(col + (size_t)(s + RS_WAVES) * W * 3, end, d2);
          add_row(d, s);
          if (two) add_row(d2, s + RS_WAVES);
        }
        flush_packed(acc, pk, (uint32_t)h);
      }
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) part[wv][16 * lane + e] = acc[e];
    __syncthreads();
#pragma unroll
    for (int e = 0; e < RS_CHUNK / RS_THREADS; ++e) {
      const int c = tid + e * RS_THREADS;
      part[0][c] = ((part[0][c] + part[1][c]) + part[2][c]) + part[3][c];
    }
    __syncthreads();
    // ---- horizontal pass: four lanes per destination pixel, 64 destination pixels per round
    for (int jr = 0; jr < nj; jr += RS_THREADS / 4) {
      const int jj = jr + (tid >> 2), k = tid & 3;
      TT sum[3] = {0, 0, 0};
      if (jj < nj) {
        const int j = j0 + jj;
        int lo, hi, xs = 0;
        if (AA) {
          xs = x_start[j];
          lo = xs;
          hi = xs + x_taps;
        } else {
          lo = (int)(((int64_t)j * W) / w);
          hi = (int)(((int64_t)(j + 1) * W + w - 1) / w);
        }
        lo = max(lo, ta);
        hi = min(hi, tb);
        for (int t = lo + k; t < hi; t += 4) {
          const TA* c = &part[0][3 * (t - ta)];
          if constexpr (AA) {
            const float wx = x_w[(size_t)j * x_taps + (t - xs)];
            sum[0] += wx * c[0];
            sum[1] += wx * c[1];
            sum[2] += wx * c[2];
          } else {
            const uint64_t wx = box_weight(j, t, W, w);
            sum[0] += wx * c[0];
            sum[1] += wx * c[1];
            sum[2] += wx * c[2];
          }
        }
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        sum[c] += __shfl_xor(sum[c], 1, 64);
        sum[c] += __shfl_xor(sum[c], 2, 64);
      }
      if (jj < nj && k == 0) {
        tot[3 * jj + 0] += sum[0];
        tot[3 * jj + 1] += sum[1];
        tot[3 * jj + 2] += sum[2];
      }
    }
    __syncthreads();
  }

  for (int jj = tid; jj < nj; jj += RS_THREADS) {
    const size_t px = ((size_t)ni * h + i) * w + j0 + jj;
    if constexpr (AA) {
      store_normalized<MODE == RS_AA_BF16>(out, px * cpad, cpad, nm, tot[3 * jj], tot[3 * jj + 1], tot[3 * jj + 2]);
    } else {
      const uint64_t hw = (uint64_t)H * W;
      uint8_t* dst = reinterpret_cast<uint8_t*>(out) + px * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) dst[c] = (uint8_t)((2 * tot[3 * jj + c] + hw) / (2 * hw));
    }
  }
}

// dst[i][j] = src[(i H) / h][(j W) / w]: four destination pixels per thread, one dword store where the address allows it
__global__ __launch_bounds__(256) void resize_nearest_kernel(const uint8_t* __restrict__ src, int H, int W, int h, int w,
                                                             uint8_t* __restrict__ dst) {
  const int ni = blockIdx.z;
  const int w4 = (w + 3) >> 2;
  const uint8_t* img = src + (size_t)ni * H * W;
  uint8_t* o = dst + (size_t)ni * h * w;
  const int64_t total = (int64_t)h * w4;
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (int64_t)gridDim.x * 256) {
    const int i = (int)(g / w4), j = (int)(g - (int64_t)i * w4) * 4;
    const uint8_t* row = img + (size_t)(((int64_t)i * H) / h) * W;
    uint8_t* p = o + (size_t)i * w + j;
    uint32_t v = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (j + k < w) v |= (uint32_t)row[((int64_t)(j + k) * W) / w] << (8 * k);
    if (j + 4 <= w && ((uintptr_t)p & 3) == 0) {
      *reinterpret_cast<uint32_t*>(p) = v;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (j + k < w) p[k] = (uint8_t)(v >> (8 * k));
    }
  }
}

// hist[k][v] += pixels of mask k equal to v.  One LDS table per wave; a lane reads 16 pixels and adds each RUN of equal pixels
// with one LDS atomic, so a mask of large uniform regions costs one atomic per 16 pixels, and a constant mask one same-address
// wave instruction per 1024 pixels, not per 64.  The block's tables are flushed with one 64-bit global atomic per non-empty
// value; the grid is small (MH_MAX_BLOCKS per call) because on a constant mask all of those land on one address.
constexpr int MH_THREADS = 256;
constexpr int MH_MAX_BLOCKS = 256;

__device__ __forceinline__ void count_runs(unsigned int* __restrict__ hist, const uint32_t (&d)[4]) {
  uint32_t cur = d[0] & 255u, cnt = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t b = (d[q] >> (8 * k)) & 255u;
      if (b != cur) {
        atomicAdd(&hist[cur], cnt);
        cur = b;
        cnt = 0;
      }
      ++cnt;
    }
  atomicAdd(&hist[cur], cnt);
}

__global__ __launch_bounds__(MH_THREADS) void mask_hist_kernel(const uint8_t* __restrict__ masks, int64_t pixels,
                                                               unsigned long long* __restrict__ hist) {
  __shared__ unsigned int lh[MH_THREADS / 64][256];
  const int tid = threadIdx.x, wv = tid >> 6, k = blockIdx.y;
  for (int v = tid; v < (MH_THREADS / 64) * 256; v += MH_THREADS) (&lh[0][0])[v] = 0;
  __syncthreads();
  const uint8_t* m = masks + (size_t)k * pixels;
  // [0, head): bytes before the first 16-byte boundary; then nvec aligned vectors; then the tail
  int64_t head = (int64_t)((16 - ((uintptr_t)m & 15)) & 15);
  if (head > pixels) head = pixels;
  const int64_t nvec = (pixels - head) >> 4;
  const uint4* vec = reinterpret_cast<const uint4*>(m + head);
  for (int64_t g = (int64_t)blockIdx.x * MH_THREADS + tid; g < nvec; g += (int64_t)gridDim.x * MH_THREADS) {
    const uint4 v = vec[g];
    const uint32_t d[4] = {v.x, v.y, v.z, v.w};
    count_runs(lh[wv], d);
  }
  if (blockIdx.x == 0) {
    const int64_t tail0 = head + (nvec << 4);
    for (int64_t p = tid; p < head; p += MH_THREADS) atomicAdd(&lh[wv][m[p]], 1u);
    for (int64_t p = tail0 + tid; p < pixels; p += MH_THREADS) atomicAdd(&lh[wv][m[p]], 1u);
  }
  __syncthreads();
  for (int v = tid; v < 256; v += MH_THREADS) {
    const unsigned int c = lh[0][v] + lh[1][v] + lh[2][v] + lh[3][v];
    if (c) atomicAdd(&hist[(size_t)k * 256 + v], (unsigned long long)c);
  }
}

static int resize_jb(int L, int l, int taps) {   // destination pixels per block: their source span fits one piece where it can
  const int64_t room = RS_CHUNK_PX - 1 - taps;
  int64_t jb = room > 0 ? room * l / L : 1;
  if (jb < 1) jb = 1;
  if (jb > RS_MAX_JB) jb = RS_MAX_JB;
  return (int)jb;
}

static bool resize_extents_ok(int n, int H, int W, int h, int w) {
  return n > 0 && H > 0 && W > 0 && h > 0 && w > 0 && n <= 65535 && h <= 65535 && (int64_t)H * h < (1LL << 31) &&
         (int64_t)W * w < (1LL << 31) && (int64_t)H * W < (1LL << 40);
}

}  // namespace udaseg

using namespace udaseg;

extern "C" int udaseg_resize_area_u8(const uint8_t* src, int n, int H, int W, int h, int w, uint8_t* dst, void* stream) {
  UDASEG_CHECK_ARG(src && dst, "resize_area_u8: NULL pointer");
  UDASEG_CHECK_ARG(resize_extents_ok(n, H, W, h, w),
                   "resize_area_u8: need n, h in 1..65535, H*h and W*w below 2^31 (n=%d H=%d W=%d h=%d w=%d)", n, H, W, h, w);
  UDASEG_CHECK_ARG(H <= 16843009, "resize_area_u8: H must be at most 16843009 (column sums reach 255*H and are 32-bit), got %d", H);
  UDASEG_CHECK_ARG(H >= h && W >= w, "resize_area_u8: %dx%d -> %dx%d enlarges an axis; the area filter only shrinks -- use the "
                   "bilinear mode (udaseg_resize_aa_u8)", H, W, h, w);
  const int jb = resize_jb(W, w, 0);
  hipLaunchKernelGGL(resize_sep_kernel<RS_AREA>, dim3(cdiv(w, jb), h, n), dim3(RS_THREADS), 0, as_stream(stream), src,
                     src + (size_t)n * H * W * 3, H, W, h, w, jb, (const int32_t*)nullptr, (const float*)nullptr, 0,
                     (const int32_t*)nullptr, (const float*)nullptr, 0, Normalize3{}, (void*)dst, 0);
  UDASEG_LAUNCH_CHECK("resize_area launch");
  return UDASEG_OK;
}

extern "C" int udaseg_resize_aa_u8(const uint8_t* src, int n, int H, int W, int h, int w, const int32_t* y_start, const float* y_w,
                                   int y_taps, const int32_t* x_start, const float* x_w, int x_taps, const float* mean255,
                                   const float* inv_std255, void* out, int cpad, int out_bf16, void* stream) {
  UDASEG_CHECK_ARG(src && out && y_start && y_w && x_start && x_w && mean255 && inv_std255, "resize_aa_u8: NULL pointer");
  UDASEG_CHECK_ARG(resize_extents_ok(n, H, W, h, w),
                   "resize_aa_u8: need n, h in 1..65535, H*h and W*w below 2^31 (n=%d H=%d W=%d h=%d w=%d)", n, H, W, h, w);
  UDASEG_CHECK_ARG(y_taps >= 1 && x_taps >= 1 && y_taps <= H + 1 && x_taps <= W + 1,
                   "resize_aa_u8: taps must lie in 1..side+1 (y_taps=%d x_taps=%d)", y_taps, x_taps);
  UDASEG_CHECK_ARG(cpad >= 4 && cpad % (out_bf16 ? 8 : 4) == 0, "resize_aa_u8: cpad must be a multiple of %d", out_bf16 ? 8 : 4);
  const int jb = resize_jb(W, w, x_taps);
  const Normalize3 nm = normalize3(mean255, inv_std255);
  const dim3 grid(cdiv(w, jb), h, n);
  const uint8_t* end = src + (size_t)n * H * W * 3;
  if (out_bf16)
    hipLaunchKernelGGL(resize_sep_kernel<RS_AA_BF16>, grid, dim3(RS_THREADS), 0, as_stream(stream), src, end, H, W, h, w, jb, y_start,
                       y_w, y_taps, x_start, x_w, x_taps, nm, out, cpad);
  else
    hipLaunchKernelGGL(resize_sep_kernel<RS_AA_F32>, grid, dim3(RS_THREADS), 0, as_stream(stream), src, end, H, W, h, w, jb, y_start,
                       y_w, y_taps, x_start, x_w, x_taps, nm, out, cpad);
  UDASEG_LAUNCH_CHECK("resize_aa launch");
  return UDASEG_OK;
}

extern "C" int udaseg_resize_nearest_u8(const uint8_t* src, int n, int H, int W, int h, int w, uint8_t* dst, void* stream) {
  UDASEG_CHECK_ARG(src && dst, "resize_nearest_u8: NULL pointer");
  UDASEG_CHECK_ARG(resize_extents_ok(n, H, W, h, w),
                   "resize_nearest_u8: need n, h in 1..65535, H*h and W*w below 2^31 (n=%d H=%d W=%d h=%d w=%d)", n, H, W, h, w);
  const int64_t groups = (int64_t)h * ((w + 3) / 4);
  const int gx = (int)(cdiv64(groups, 256) > 1024 ? 1024 : cdiv64(groups, 256));
  hipLaunchKernelGGL(resize_nearest_kernel, dim3(gx, 1, n), dim3(256), 0, as_stream(stream), src, H, W, h, w, dst);
  UDASEG_LAUNCH_CHECK("resize_nearest launch");
  return UDASEG_OK;
}

extern "C" int udaseg_mask_hist_u8(const uint8_t* masks, int n, int64_t pixels, int64_t* hist, void* stream) {
  UDASEG_CHECK_ARG(masks && hist, "mask_hist_u8: NULL pointer");
  UDASEG_CHECK_ARG(n > 0 && n <= 65535 && pixels > 0 && pixels < (1LL << 32),
                   "mask_hist_u8: need n in 1..65535 and 0 < pixels < 2^32 (n=%d pixels=%lld)", n, (long long)pixels);
  int64_t gx = cdiv64(pixels, (int64_t)MH_THREADS * 16 * 4);
  const int64_t cap = MH_MAX_BLOCKS / n > 1 ? MH_MAX_BLOCKS / n : 1;
  if (gx > cap) gx = cap;
  if (gx < 1) gx = 1;
  hipLaunchKernelGGL(mask_hist_kernel, dim3((int)gx, n), dim3(MH_THREADS), 0, as_stream(stream), masks, pixels,
                     (unsigned long long*)hist);
  UDASEG_LAUNCH_CHECK("mask_hist launch");
  return UDASEG_OK;
}
