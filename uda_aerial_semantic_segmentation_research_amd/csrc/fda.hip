// Fourier-domain style transfer of source frames to a target's style on the device (FDA, Yang & Soatto 2020; the amplitude mix of
// Xu et al. 2021; an extension: the reference has no counterpart).  The low-frequency amplitude of a source frame's spectrum is
// replaced by (mixed with) a target frame's, the phase stays the source's.  Only the (2b+1) x (2b+1) lowest frequencies change, so
// no FFT is needed (and none is linked):
//     out = src + Re(IDFT(D)),   D[u][v] = lam (|F_t[u][v]| - |F_s[u][v]|) F_s[u][v] / |F_s[u][v]|   for |u|, |v| <= b, 0 elsewhere
// and F_s, F_t are needed on that block alone: a separable partial DFT W_r (K x H) . X (H x W) . W_c^T (W x K), K = 2 bmax + 1.
// fda.py's module docstring has the contract.  Twiddles come from tables tw[k] = (cos, sin)(2 pi k / L), k in [0, L), built on the
// host in float64 (the synthesis takes their float32 roundings) and indexed by (u * y) mod L in integers: no device sincos.
//
//   udaseg_fda_spectrum_u8   ANALYSIS in float64 from the exact integer pixels, two stages through a caller's workspace:
//       row stage     rows[i][c][y][kv] = sum_x X[i][y][x][c] e^{-2 pi i v x / W}.  A wave takes a 256-pixel segment of a row
//                     (one, two or four waves per row by its width),
//                     lanes across x, four pixels per lane with the three interleaved channels apart in registers: every frame
//                     byte is loaded once.  Eight kv at a time (48 float64 accumulators per lane) are reduced over the wave by a
//                     reduce-scatter (xor 32, 16, 8 halve the kv a lane holds, xor 4, 2, 1 finish its own), then over the row's
//                     waves through LDS in a fixed order; a row wider than 1024 pixels takes more passes, which the same thread
//                     adds into the workspace.  No atomics: the same frames give the same bits.
//       column stage  coeffs[i][c][ku][kv] = sum_y rows[i][c][y][kv] e^{-2 pi i u y / H}: a 16 x 16 tile of coefficients per block, the rows
//                     and twiddles of 64 y at a time in LDS, a thread per coefficient adding y in order.
//   udaseg_fda_amplitude     |F| of a coefficient table (the companion of the delta kernel: the target side).
//   udaseg_fda_delta         D / (H W) in float32, the per-sample band mask inside the bmax block and the degenerate rule applied.
//   udaseg_fda_apply_u8      SYNTHESIS in float32: a small pre-kernel forms the column part T[i][c][ku][x] = sum_v D[ku][v]
//                     e^{+2 pi i v x / W} once (a block of the streaming pass that formed it for its own x range would repeat
//                     K * K multiply-adds per column for every 32 rows, 2 K / 32 times the pass's own work: 5.8 times at K = 93);
//                     the streaming pass then takes 32 x 64 pixel tiles, a lane per column and eight rows per lane, K complex
//                     multiply-adds per value with conj(w_r[u][y]) staged in LDS 32 u at a time.  The frame tile goes through
//                     LDS both ways: 16-byte loads and stores when w % 16 == 0 and the pointers are 16-byte aligned (wide form),
//                     bytes otherwise (scalar form); the arithmetic is the same code, so the two forms give the same bytes.
//
// b[i] and pick[i] are device tables: the kernels clamp them (b to [-1, bmax], pick to [0, m)), so a bad table cannot index out of
// bounds.  A sample with b[i] = -1 adds nothing: its output is the copy of its source.
#include "common.h"

namespace udaseg {

typedef unsigned int fda_u32x4 __attribute__((ext_vector_type(4)));

constexpr int FS_THREADS = 256, FS_WAVES = 4;       // row stage: threads, waves per block
constexpr int FS_PX = 4;                            // pixels per lane and pass: a wave's segment is 64 * FS_PX = 256 pixels
constexpr int FS_SEG = 64 * FS_PX;
constexpr int FS_KB = 8;                            // kv per reduction batch
constexpr int FC_THREADS = 128;                     // delta, amplitude
constexpr int FT_THREADS = 256, FT_TILE = 16, FT_Y = 64;   // column stage: a 16 x 16 tile of (ku, kv) per block, y per staged chunk
constexpr int FA_THREADS = 256;                     // streaming pass
static_assert(FA_THREADS == 64 * 4, "BlockCounts<K>: four waves a block");
constexpr int FA_ROWS = 32, FA_COLS = 64, FA_RPL = 8;   // tile; rows per lane (FA_ROWS = 4 waves * FA_RPL)
constexpr int FA_UC = 32;                           // u per staged twiddle chunk
constexpr int FA_PITCH = FA_COLS * 3;               // 192 bytes: a multiple of 16

__device__ __forceinline__ int fda_band(const int32_t* __restrict__ b, int i, int bmax) {
  const int v = b[i];
  return v < -1 ? -1 : (v > bmax ? bmax : v);
}

// (f * k) mod L for a frequency f in [-bmax, bmax] and 0 <= k < L, bmax < L
__device__ __forceinline__ int fda_index(int f, int k, int L) {
  const int fm = f < 0 ? f + L : f;
  return (int)(((long long)fm * k) % L);
}

__device__ __forceinline__ double fda_shfl_xor_d(double v, int mask) { return __shfl_xor(v, mask, 64); }

// ---------------------------------------------------------------------------------------------------------------- analysis
__global__ __launch_bounds__(FS_THREADS) void fda_rows_kernel(const uint8_t* __restrict__ frames, const double* __restrict__ tw_w, int n,
                                                              int h, int w, int bmax, int wpr, double* __restrict__ rows) {
  __shared__ double red[FS_WAVES][FS_KB][6];
  const int K = 2 * bmax + 1;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int rpb = FS_WAVES / wpr;                                           // rows per block: 4 (w <= 256), 2 (w <= 512) or 1
  const long long row = (long long)blockIdx.x * rpb + wave / wpr;           // i * h + y
  const bool live = row < (long long)n * h;
  const int seg = wave % wpr;
  const uint8_t* src = frames + (size_t)(live ? row : 0) * w * 3;
  const bool up32 = lane & 32, up16 = lane & 16, up8 = lane & 8;
  for (int x0 = 0, pass = 0; x0 < w; x0 += FS_SEG * wpr, ++pass) {
    double px[FS_PX][3];
    int xs[FS_PX];
#pragma unroll
    for (int p = 0; p < FS_PX; ++p) {
      const int x = x0 + seg * FS_SEG + p * 64 + lane;
      const bool in = live && x < w;
      xs[p] = in ? x : 0;                                                   // x = 0 with zero pixels adds exact zeros
#pragma unroll
      for (int c = 0; c < 3; ++c) px[p][c] = in ? (double)src[(size_t)x * 3 + c] : 0.0;
    }
    for (int kv0 = 0; kv0 < K; kv0 += FS_KB) {
      double v[FS_KB][6];
#pragma unroll
      for (int j = 0; j < FS_KB; ++j)
#pragma unroll
        for (int q = 0; q < 6; ++q) v[j][q] = 0.0;
#pragma unroll
      for (int p = 0; p < FS_PX; ++p) {
        int idx = fda_index(kv0 - bmax, xs[p], w);
#pragma unroll
        for (int j = 0; j < FS_KB; ++j) {                                   // kv past K - 1: computed, never written
          const double cs = tw_w[2 * idx], sn = tw_w[2 * idx + 1];
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            v[j][2 * c] = fma(px[p][c], cs, v[j][2 * c]);
            v[j][2 * c + 1] = fma(-px[p][c], sn, v[j][2 * c + 1]);
          }
          idx += xs[p];
          if (idx >= w) idx -= w;
        }
      }
      // reduce-scatter over the wave: after the three steps a lane holds the six sums of kv0 + ((lane >> 3) & 7) over 8 lanes
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int q = 0; q < 6; ++q) {
          const double keep = up32 ? v[j + 4][q] : v[j][q], send = up32 ? v[j][q] : v[j + 4][q];
          v[j][q] = keep + fda_shfl_xor_d(send, 32);
        }
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int q = 0; q < 6; ++q) {
          const double keep = up16 ? v[j + 2][q] : v[j][q], send = up16 ? v[j][q] : v[j + 2][q];
          v[j][q] = keep + fda_shfl_xor_d(send, 16);
        }
#pragma unroll
      for (int q = 0; q < 6; ++q) {
        const double keep = up8 ? v[1][q] : v[0][q], send = up8 ? v[0][q] : v[1][q];
        v[0][q] = keep + fda_shfl_xor_d(send, 8);
      }
#pragma unroll
      for (int q = 0; q < 6; ++q) {
        double s = v[0][q];
        s += fda_shfl_xor_d(s, 4);
        s += fda_shfl_xor_d(s, 2);
        s += fda_shfl_xor_d(s, 1);
        v[0][q] = s;
      }
      if ((lane & 7) == 0) {
#pragma unroll
        for (int q = 0; q < 6; ++q) red[wave][lane >> 3][q] = v[0][q];
      }
      __syncthreads();
      if ((int)threadIdx.x < rpb * FS_KB * 6) {                             // the row's waves in a fixed order, then the workspace
        const int r = threadIdx.x / (FS_KB * 6), e = threadIdx.x - r * (FS_KB * 6);
        const int j = e / 6, q = e - j * 6;
        const long long orow = (long long)blockIdx.x * rpb + r;
        const int kv = kv0 + j;
        if (orow < (long long)n * h && kv < K) {
          double s = red[r * wpr][j][q];
          for (int sw = 1; sw < wpr; ++sw) s += red[r * wpr + sw][j][q];
          const int oi = (int)(orow / h), oy = (int)(orow - (long long)oi * h);
          double* dst = rows + ((((size_t)oi * 3 + (q >> 1)) * h + oy) * K + kv) * 2 + (q & 1);
          if (pass) s += *dst;                                              // written by this thread in the pass before
          *dst = s;
        }
      }
      __syncthreads();
    }
  }
}

// A (K x H) . (H x K) complex product per sample and channel: a block takes a 16 x 16 tile of (ku, kv) and walks y in chunks of 64,
// the chunk's rows and twiddles staged in LDS, so that a row of the workspace is read once per tile row and not once per ku (at
// K = 93 the thread-per-coefficient form read 1.7 GB through L2, 0.4 ms).  A thread owns one coefficient and adds y in order.
__global__ __launch_bounds__(FT_THREADS) void fda_cols_kernel(const double* __restrict__ rows, const double* __restrict__ tw_h, int h,
                                                              int bmax, int tiles, double* __restrict__ coeffs) {
  __shared__ double a[FT_Y][FT_TILE][2];
  __shared__ double t[FT_TILE][FT_Y + 1][2];                                 // + 1: the four ku of a wave on different banks
  const int K = 2 * bmax + 1;
  const int tkv = blockIdx.x % tiles;
  const int rest = blockIdx.x / tiles;
  const int tku = rest % tiles, ic = rest / tiles;
  const int lu = threadIdx.x / FT_TILE, lv = threadIdx.x % FT_TILE;
  const int ku = tku * FT_TILE + lu, kv = tkv * FT_TILE + lv;
  double re = 0.0, im = 0.0;
  for (int y0 = 0; y0 < h; y0 += FT_Y) {
    __syncthreads();
    for (int e = threadIdx.x; e < FT_Y * FT_TILE; e += FT_THREADS) {
      const int yy = e / FT_TILE, v = e % FT_TILE;                          // the chunk's rows: zeros past the frame and the block
      const int y = y0 + yy, gv = tkv * FT_TILE + v;
      const bool in = y < h && gv < K;
      const double* src = rows + (((size_t)ic * h + (in ? y : 0)) * K + (in ? gv : 0)) * 2;
      a[yy][v][0] = in ? src[0] : 0.0;
      a[yy][v][1] = in ? src[1] : 0.0;
      const int uu = e / FT_Y, ty = e % FT_Y;                               // the chunk's twiddles
      const int gu = tku * FT_TILE + uu;
      const int idx = fda_index(gu < K ? gu - bmax : 0, y0 + ty < h ? y0 + ty : 0, h);
      t[uu][ty][0] = tw_h[2 * idx];
      t[uu][ty][1] = tw_h[2 * idx + 1];
    }
    __syncthreads();
#pragma unroll 8
    for (int yy = 0; yy < FT_Y; ++yy) {
      const double ar = a[yy][lv][0], ai = a[yy][lv][1], cs = t[lu][yy][0], sn = t[lu][yy][1];
      re = fma(ar, cs, fma(ai, sn, re));                                    // (ar + i ai)(cs - i sn)
      im = fma(ai, cs, fma(-ar, sn, im));
    }
  }
  if (ku < K && kv < K) {
    double* dst = coeffs + (((size_t)ic * K + ku) * K + kv) * 2;
    dst[0] = re;
    dst[1] = im;
  }
}

__global__ __launch_bounds__(FC_THREADS) void fda_amplitude_kernel(const double* __restrict__ coeffs, long long count,
                                                                   double* __restrict__ amps) {
  const long long t = (long long)blockIdx.x * FC_THREADS + threadIdx.x;
  if (t >= count) return;
  const double re = coeffs[2 * t], im = coeffs[2 * t + 1];
  amps[t] = sqrt(fma(re, re, im * im));
}

// ------------------------------------------------------------------------------------------------------------------- delta
__global__ __launch_bounds__(FC_THREADS) void fda_delta_kernel(const double* __restrict__ coeffs, const double* __restrict__ amps,
                                                               const int32_t* __restrict__ pick, const int32_t* __restrict__ b,
                                                               const float* __restrict__ lam, int m, int bmax, double degenerate,
                                                               double inv_hw, long long total, float* __restrict__ delta) {
  const int K = 2 * bmax + 1;
  const long long t = (long long)blockIdx.x * FC_THREADS + threadIdx.x;     // ((i * 3 + c) * K + ku) * K + kv
  if (t >= total) return;
  const int kv = (int)(t % K);
  const long long r = t / K;
  const int ku = (int)(r % K);
  const long long ic = r / K;
  const int i = (int)(ic / 3), c = (int)(ic - (long long)i * 3);
  const int band = fda_band(b, i, bmax);
  const int u = ku - bmax, v = kv - bmax;
  float dr = 0.f, di = 0.f;
  if (u >= -band && u <= band && v >= -band && v <= band) {
    int p = pick[i];
    p = p < 0 ? 0 : (p >= m ? m - 1 : p);
    const double re = coeffs[2 * t], im = coeffs[2 * t + 1];
    const double as = sqrt(fma(re, re, im * im));
    const double at = amps[(((size_t)p * 3 + c) * K + ku) * K + kv];
    double pr = 1.0, pi = 0.0;                                              // the degenerate coefficient: phase 0
    if (as > degenerate) { pr = re / as; pi = im / as; }
    const double g = (double)lam[i] * (at - as) * inv_hw;
    dr = (float)(g * pr);
    di = (float)(g * pi);
  }
  delta[2 * t] = dr;
  delta[2 * t + 1] = di;
}

// --------------------------------------------------------------------------------------------------------------- synthesis
// T[i][c][ku][x] = sum_{|v| <= band} D[i][c][ku][v] e^{+2 pi i v x / W} for |u| <= band; the rest of T is neither written nor read
__global__ __launch_bounds__(FA_THREADS) void fda_colpart_kernel(const float* __restrict__ delta, const int32_t* __restrict__ b,
                                                                 const float* __restrict__ tw_w, int w, int bmax, int xblocks,
                                                                 float* __restrict__ colws) {
  const int K = 2 * bmax + 1;
  const long long blk = blockIdx.x;
  const int xb = (int)(blk % xblocks);
  const long long r = blk / xblocks;                                        // (i * 3 + c) * K + ku
  const int ku = (int)(r % K);
  const int i = (int)(r / K / 3);
  const int band = fda_band(b, i, bmax);
  const int u = ku - bmax;
  if (u < -band || u > band) return;
  const int x = xb * FA_THREADS + threadIdx.x;
  if (x >= w) return;
  const float* d = delta + ((size_t)r * K + (bmax - band)) * 2;
  int idx = fda_index(-band, x, w);
  float re = 0.f, im = 0.f;
  for (int v = -band; v <= band; ++v, d += 2) {
    const float cs = tw_w[2 * idx], sn = tw_w[2 * idx + 1];
    const float dr = d[0], di = d[1];
    re = fmaf(dr, cs, fmaf(-di, sn, re));                                   // (dr + i di)(cs + i sn)
    im = fmaf(dr, sn, fmaf(di, cs, im));
    idx += x;
    if (idx >= w) idx -= w;
  }
  float* o = colws + ((size_t)r * w + x) * 2;
  o[0] = re;
  o[1] = im;
}

template <bool WIDE>
__global__ __launch_bounds__(FA_THREADS) void fda_apply_kernel(const uint8_t* __restrict__ src, const float* __restrict__ colws,
                                                               const int32_t* __restrict__ b, const float* __restrict__ tw_h, int h,
                                                               int w, int bmax, int tiles_x, int tiles_y, uint8_t* __restrict__ out,
                                                               float* __restrict__ field, unsigned long long* __restrict__ counts) {
  __shared__ float tw[FA_UC][FA_ROWS][2];
  __shared__ __attribute__((aligned(16))) uint8_t tile[FA_ROWS * FA_PITCH];
  __shared__ BlockCounts<2>::Slots cnt;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tx = blockIdx.x % tiles_x;
  const int rest = blockIdx.x / tiles_x;
  const int ty = rest % tiles_y, i = rest / tiles_y;
  const int y0 = ty * FA_ROWS, x0 = tx * FA_COLS;
  const int rows = h - y0 < FA_ROWS ? h - y0 : FA_ROWS, cols = w - x0 < FA_COLS ? w - x0 : FA_COLS;
  const int rb = cols * 3;                                                  // bytes per tile row; a multiple of 16 in the wide form
  const size_t base = (((size_t)i * h + y0) * w + x0) * 3;                  // + r * w * 3: row r of the tile
  const int band = fda_band(b, i, bmax);
  if (WIDE) {
    const int cpr = rb >> 4;
    for (int e = tid; e < rows * cpr; e += FA_THREADS) {
      const int r = e / cpr, k = e - r * cpr;
      *reinterpret_cast<fda_u32x4*>(tile + r * FA_PITCH + 16 * k) =
          *reinterpret_cast<const fda_u32x4*>(src + base + (size_t)r * w * 3 + 16 * k);
    }
  } else {
    for (int e = tid; e < rows * rb; e += FA_THREADS) {
      const int r = e / rb, k = e - r * rb;
      tile[r * FA_PITCH + k] = src[base + (size_t)r * w * 3 + k];
    }
  }
  const int x = x0 + lane;
  const bool valid = lane < cols;
  float acc[FA_RPL][3];
#pragma unroll
  for (int r = 0; r < FA_RPL; ++r) acc[r][0] = acc[r][1] = acc[r][2] = 0.f;
  const int K = 2 * bmax + 1;
  for (int u0 = -band; u0 <= band; u0 += FA_UC) {                           // band = -1: no trip, the tile is copied
    const int nu = band - u0 + 1 < FA_UC ? band - u0 + 1 : FA_UC;
    __syncthreads();
    for (int e = tid; e < nu * FA_ROWS; e += FA_THREADS) {
      const int uu = e / FA_ROWS, r = e - uu * FA_ROWS;
      const int y = y0 + r < h ? y0 + r : h - 1;
      const int k = fda_index(u0 + uu, y, h);
      tw[uu][r][0] = tw_h[2 * k];
      tw[uu][r][1] = tw_h[2 * k + 1];
    }
    __syncthreads();
    if (valid) {
      for (int uu = 0; uu < nu; ++uu) {
        const int ku = u0 + uu + bmax;
        float tr[3], ti[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float* t = colws + ((((size_t)i * 3 + c) * K + ku) * w + x) * 2;
          tr[c] = t[0];
          ti[c] = t[1];
        }
#pragma unroll
        for (int r = 0; r < FA_RPL; ++r) {
          const float cs = tw[uu][wave * FA_RPL + r][0], sn = tw[uu][wave * FA_RPL + r][1];
#pragma unroll
          for (int c = 0; c < 3; ++c) acc[r][c] = fmaf(tr[c], cs, fmaf(-ti[c], sn, acc[r][c]));   // Re((tr + i ti)(cs + i sn))
        }
      }
    }
  }
  __syncthreads();                                                          // the tile is staged
  unsigned int ev[2] = {0, 0};                                              // below 0, above 255
#pragma unroll
  for (int r = 0; r < FA_RPL; ++r) {
    const int row = wave * FA_RPL + r;
    if (valid && row < rows) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float v = (float)tile[row * FA_PITCH + lane * 3 + c] + acc[r][c];
        ev[0] += v < 0.f ? 1u : 0u;
        ev[1] += v > 255.f ? 1u : 0u;
        if (field) field[base + ((size_t)row * w + lane) * 3 + c] = v;
        tile[row * FA_PITCH + lane * 3 + c] = (uint8_t)fminf(fmaxf(rintf(v), 0.f), 255.f);   // round half to even, then clamp
      }
    }
  }
  if (counts) BlockCounts<2>::put(cnt, ev);
  __syncthreads();                                                          // the tile holds the output bytes; closes the slots
  if (counts) BlockCounts<2>::flush(cnt, counts + (size_t)i * 2);
  if (!out) return;
  if (WIDE) {
    const int cpr = rb >> 4;
    for (int e = tid; e < rows * cpr; e += FA_THREADS) {
      const int r = e / cpr, k = e - r * cpr;
      *reinterpret_cast<fda_u32x4*>(out + base + (size_t)r * w * 3 + 16 * k) =
          *reinterpret_cast<const fda_u32x4*>(tile + r * FA_PITCH + 16 * k);
    }
  } else {
    for (int e = tid; e < rows * rb; e += FA_THREADS) {
      const int r = e / rb, k = e - r * rb;
      out[base + (size_t)r * w * 3 + k] = tile[r * FA_PITCH + k];
    }
  }
}

static bool fda_overlap(const void* a, size_t na, const void* b, size_t nb) {
  if (!a || !b) return false;
  const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
  return pa < pb + nb && pb < pa + na;
}

// outs against ins and against one another
static bool fda_any_overlap(const void* const* outs, const size_t* out_bytes, int no, const void* const* ins, const size_t* in_bytes,
                            int ni, int* which_out, int* which_other) {
  for (int o = 0; o < no; ++o) {
    for (int i = 0; i < ni; ++i)
      if (fda_overlap(outs[o], out_bytes[o], ins[i], in_bytes[i])) { *which_out = o; *which_other = i; return true; }
    for (int p = 0; p < o; ++p)
      if (fda_overlap(outs[o], out_bytes[o], outs[p], out_bytes[p])) { *which_out = o; *which_other = -1 - p; return true; }
  }
  return false;
}

static bool fda_extents_ok(int n, int h, int w) { return n > 0 && h > 0 && w > 0 && (int64_t)n * h * w < ((int64_t)1 << 31); }
static bool fda_bmax_ok(int bmax, int h, int w) { return bmax >= 0 && bmax <= ((h < w ? h : w) - 1) / 2; }

}  // namespace udaseg

using namespace udaseg;

extern "C" int udaseg_fda_spectrum_u8(const uint8_t* frames, const double* tw_h, const double* tw_w, int n, int h, int w, int bmax,
                                      double* rows_ws, double* coeffs, void* stream) {
  UDASEG_CHECK_ARG(frames && tw_h && tw_w && rows_ws && coeffs, "fda_spectrum_u8: NULL pointer");
  UDASEG_CHECK_ARG(fda_extents_ok(n, h, w), "fda_spectrum_u8: need n, h, w > 0 and n*h*w < 2^31 (n=%d h=%d w=%d)", n, h, w);
  UDASEG_CHECK_ARG(fda_bmax_ok(bmax, h, w), "fda_spectrum_u8: need 0 <= bmax <= (min(h, w) - 1) / 2 (bmax=%d h=%d w=%d)", bmax, h, w);
  const size_t K = 2 * (size_t)bmax + 1;
  const void* ins[3] = {frames, tw_h, tw_w};
  const size_t in_bytes[3] = {(size_t)n * h * w * 3, (size_t)h * 16, (size_t)w * 16};
  const void* outs[2] = {rows_ws, coeffs};
  const size_t out_bytes[2] = {(size_t)n * 3 * h * K * 16, (size_t)n * 3 * K * K * 16};
  int a = 0, o = 0;
  UDASEG_CHECK_ARG(!fda_any_overlap(outs, out_bytes, 2, ins, in_bytes, 3, &a, &o),
                   "fda_spectrum_u8: output %d overlaps operand %d (negative: output -1 - value)", a, o);
  const int wpr = w <= FS_SEG ? 1 : (w <= 2 * FS_SEG ? 2 : FS_WAVES);        // waves per row: none without pixels in the first pass
  const int64_t rows = (int64_t)n * h;
  hipLaunchKernelGGL(fda_rows_kernel, dim3((unsigned int)cdiv64(rows, FS_WAVES / wpr)), dim3(FS_THREADS), 0, as_stream(stream), frames,
                     tw_w, n, h, w, bmax, wpr, rows_ws);
  UDASEG_LAUNCH_CHECK("fda_spectrum_u8 row stage launch");
  const int tiles = cdiv((int)K, FT_TILE);
  const int64_t cblocks = (int64_t)n * 3 * tiles * tiles;                   // <= 3 n (K / 16 + 1)^2, K <= min(h, w)
  UDASEG_CHECK_ARG(cblocks < ((int64_t)1 << 31), "fda_spectrum_u8: 3 n ceil((2 bmax + 1) / 16)^2 must stay below 2^31");
  hipLaunchKernelGGL(fda_cols_kernel, dim3((unsigned int)cblocks), dim3(FT_THREADS), 0, as_stream(stream), (const double*)rows_ws, tw_h,
                     h, bmax, tiles, coeffs);
  UDASEG_LAUNCH_CHECK("fda_spectrum_u8 column stage launch");
  return UDASEG_OK;
}

extern "C" int udaseg_fda_amplitude(const double* coeffs, int64_t count, double* amps, void* stream) {
  UDASEG_CHECK_ARG(coeffs && amps, "fda_amplitude: NULL pointer");
  UDASEG_CHECK_ARG(count > 0 && count < ((int64_t)1 << 34), "fda_amplitude: need 0 < count < 2^34 (count=%lld)", (long long)count);
  UDASEG_CHECK_ARG(!fda_overlap(amps, (size_t)count * 8, coeffs, (size_t)count * 16), "fda_amplitude: amps overlaps coeffs");
  hipLaunchKernelGGL(fda_amplitude_kernel, dim3((unsigned int)cdiv64(count, FC_THREADS)), dim3(FC_THREADS), 0, as_stream(stream), coeffs,
                     (long long)count, amps);
  UDASEG_LAUNCH_CHECK("fda_amplitude launch");
  return UDASEG_OK;
}

extern "C" int udaseg_fda_delta(const double* coeffs, const double* amps, const int32_t* pick, const int32_t* b, const float* lam, int n,
                                int m, int h, int w, int bmax, float* delta, void* stream) {
  UDASEG_CHECK_ARG(coeffs && amps && pick && b && lam && delta, "fda_delta: NULL pointer");
  UDASEG_CHECK_ARG(fda_extents_ok(n, h, w), "fda_delta: need n, h, w > 0 and n*h*w < 2^31 (n=%d h=%d w=%d)", n, h, w);
  UDASEG_CHECK_ARG(m > 0, "fda_delta: need m > 0 target rows (m=%d)", m);
  UDASEG_CHECK_ARG(fda_bmax_ok(bmax, h, w), "fda_delta: need 0 <= bmax <= (min(h, w) - 1) / 2 (bmax=%d h=%d w=%d)", bmax, h, w);
  const size_t K = 2 * (size_t)bmax + 1;
  const void* ins[5] = {coeffs, amps, pick, b, lam};
  const size_t in_bytes[5] = {(size_t)n * 3 * K * K * 16, (size_t)m * 3 * K * K * 8, (size_t)n * 4, (size_t)n * 4, (size_t)n * 4};
  const void* outs[1] = {delta};
  const size_t out_bytes[1] = {(size_t)n * 3 * K * K * 8};
  int a = 0, o = 0;
  UDASEG_CHECK_ARG(!fda_any_overlap(outs, out_bytes, 1, ins, in_bytes, 5, &a, &o), "fda_delta: delta overlaps input %d", o);
  const long long total = (long long)n * 3 * (long long)(K * K);
  const double hw = (double)h * (double)w;
  hipLaunchKernelGGL(fda_delta_kernel, dim3((unsigned int)cdiv64(total, FC_THREADS)), dim3(FC_THREADS), 0, as_stream(stream), coeffs, amps,
                     pick, b, lam, m, bmax, 1e-9 * 255.0 * hw, 1.0 / hw, total, delta);
  UDASEG_LAUNCH_CHECK("fda_delta launch");
  return UDASEG_OK;
}

extern "C" int udaseg_fda_apply_u8(const uint8_t* src, const float* delta, const int32_t* b, const float* tw_h, const float* tw_w, int n,
                                   int h, int w, int bmax, float* cols_ws, uint8_t* out, float* field, int64_t* counts, void* stream) {
  UDASEG_CHECK_ARG(src && delta && b && tw_h && tw_w && cols_ws, "fda_apply_u8: NULL pointer");
  UDASEG_CHECK_ARG(out || field, "fda_apply_u8: need out, field or both");
  UDASEG_CHECK_ARG(fda_extents_ok(n, h, w), "fda_apply_u8: need n, h, w > 0 and n*h*w < 2^31 (n=%d h=%d w=%d)", n, h, w);
  UDASEG_CHECK_ARG(fda_bmax_ok(bmax, h, w), "fda_apply_u8: need 0 <= bmax <= (min(h, w) - 1) / 2 (bmax=%d h=%d w=%d)", bmax, h, w);
  const size_t K = 2 * (size_t)bmax + 1;
  const size_t px = (size_t)n * h * w;
  const void* ins[5] = {src, delta, b, tw_h, tw_w};
  const size_t in_bytes[5] = {px * 3, (size_t)n * 3 * K * K * 8, (size_t)n * 4, (size_t)h * 8, (size_t)w * 8};
  const void* outs[4] = {cols_ws, out, field, counts};
  const size_t out_bytes[4] = {(size_t)n * 3 * K * w * 8, px * 3, px * 12, (size_t)n * 16};
  int a = 0, o = 0;
  UDASEG_CHECK_ARG(!fda_any_overlap(outs, out_bytes, 4, ins, in_bytes, 5, &a, &o),
                   "fda_apply_u8: output %d overlaps operand %d (negative: output -1 - value)", a, o);
  const int xblocks = cdiv(w, FA_THREADS);
  const int64_t cblocks = (int64_t)n * 3 * (int64_t)K * xblocks;            // K <= w: <= 3 n w (w / 256 + 1)
  UDASEG_CHECK_ARG(cblocks < ((int64_t)1 << 31), "fda_apply_u8: n * 3 * (2 bmax + 1) * ceil(w / 256) must stay below 2^31");
  hipLaunchKernelGGL(fda_colpart_kernel, dim3((unsigned int)cblocks), dim3(FA_THREADS), 0, as_stream(stream), delta, b, tw_w, w, bmax,
                     xblocks, cols_ws);
  UDASEG_LAUNCH_CHECK("fda_apply_u8 column part launch");
  const int tiles_x = cdiv(w, FA_COLS), tiles_y = cdiv(h, FA_ROWS);
  const dim3 grid((unsigned int)((int64_t)n * tiles_y * tiles_x));          // <= n*h*w < 2^31
  const uintptr_t align = reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(out);   // NULL adds nothing
  const bool wide = w % 16 == 0 && (align & 15) == 0;
  if (wide)
    hipLaunchKernelGGL(fda_apply_kernel<true>, grid, dim3(FA_THREADS), 0, as_stream(stream), src, (const float*)cols_ws, b, tw_h, h, w,
                       bmax, tiles_x, tiles_y, out, field, (unsigned long long*)counts);
  else
    hipLaunchKernelGGL(fda_apply_kernel<false>, grid, dim3(FA_THREADS), 0, as_stream(stream), src, (const float*)cols_ws, b, tw_h, h, w,
                       bmax, tiles_x, tiles_y, out, field, (unsigned long long*)counts);
  UDASEG_LAUNCH_CHECK("fda_apply_u8 launch");
  return UDASEG_OK;
}
