// CLAHE of the two device augmentation pipelines (stage-5 kind 3; the definition: INTEGRATION.md, "CLAHE"): the table pass.
// The stage needs a histogram of the Lab lightness of the stage-4 image over each of the 8 x 8 tiles before any output pixel
// can be written, so it gets a pass of its own between the source pass and the output pass:
//   one block per (tile, sample, view); samples not on CLAHE return at once (block-uniform)
//   stage 4 (/ 4b) is evaluated per pixel through aug_stage4 after the output pass's own per-block set-up (aug_block), as the
//   3 x 3 stage does: no full-frame intermediate
//   integer histograms in LDS, one private 256-bin histogram per wave (aerial tiles are dominated by a few bins: the four
//   waves do not queue on one another's atomics), summed afterwards, one bin per thread
//   clip, redistribution, prefix sum (a wave scan + the four wave totals) and the rounding stay in integers inside the block
//   output: uint8 lut[slot][8][8][256], slot = view * n + sample
// Integer LDS atomics are order-independent: two calls give equal bits.  The output pass's CLAHE branch (cl_apply,
// aug_common.h) lives in the two pipelines' output kernel (augment.hip).
#include "aug_common.h"

namespace udaseg {

constexpr int CL_WAVES = 4;             // 256 threads

__device__ __forceinline__ unsigned cl_wave_sum(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

template <bool TRAIN>
__global__ __launch_bounds__(256) void clahe_lut_kernel(const uint8_t* __restrict__ images, const int32_t* __restrict__ table,
                                                        const f32x4* __restrict__ mid, const ta_f2* __restrict__ field, int n, int h,
                                                        int w, uint8_t* __restrict__ lut) {
  constexpr int WORDS = TRAIN ? TA_WORDS : SA_WORDS;
  __shared__ unsigned hist[CL_WAVES][CL_BINS];
  __shared__ unsigned part[2][CL_WAVES];
  __shared__ float grid_tab[24];
  const int tile = blockIdx.x, ni = blockIdx.y, view = blockIdx.z;
  const size_t slot = (size_t)view * n + ni;
  const int32_t* t = table + slot * WORDS;
  if (!((t[SA_W_FLAGS] & SA_STAGE5) && t[SA_W_S5_KIND] == SA_CLAHE)) return;         // block-uniform
  const AugBlock blk = aug_block<TRAIN>(t, images, mid, field, ni, slot, h, w, grid_tab);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
#pragma unroll
  for (int i = 0; i < CL_WAVES; ++i) hist[i][tid] = 0u;
  __syncthreads();
  const int th = h / CL_GRID, tw = w / CL_GRID, area = th * tw;   // the entry points refuse sides that are no multiples of 8
  const int ty0 = (tile / CL_GRID) * th, tx0 = (tile % CL_GRID) * tw;
  for (int i = tid; i < area; i += 256) {
    const int ly = i / tw, lx = i - ly * tw;
    float v[3], l8, a, b;
    aug_stage4<TRAIN>(blk, ty0 + ly, tx0 + lx, v);
    cl_rgb_to_lab(v, l8, a, b);
    atomicAdd(&hist[wave][cl_bin(l8)], 1u);
  }
  __syncthreads();
  // bin `tid` from here on
  unsigned cnt = hist[0][tid] + hist[1][tid] + hist[2][tid] + hist[3][tid];
  const double lim = (double)blk.rec.s.p5a * (double)area / 256.0;    // exact: a 24-bit factor times an integer below 2^24
  const unsigned limit = lim >= (double)area ? (unsigned)area : (lim >= 1.0 ? (unsigned)lim : 1u);   // max(1, int(lim)); above the area it clips nothing
  const unsigned over = cnt > limit ? cnt - limit : 0u;
  cnt -= over;
  const unsigned wsum = cl_wave_sum(over);
  if (lane == 0) part[0][wave] = wsum;
  __syncthreads();
  const unsigned excess = part[0][0] + part[0][1] + part[0][2] + part[0][3];
  cnt += excess / CL_BINS;
  const unsigned rest = excess % CL_BINS;                         // one each to bins 0, s, 2s, ... until `rest` are placed
  if (rest) {
    const unsigned step = CL_BINS / rest;                         // >= 1 as rest <= 255
    if (tid % step == 0 && tid / step < rest) cnt += 1u;
  }
  unsigned run = cnt;                                             // inclusive prefix sum: a scan per wave, then the waves before it
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned up = __shfl_up(run, o);
    if (lane >= o) run += up;
  }
  if (lane == 63) part[1][wave] = run;
  __syncthreads();
  for (int i = 0; i < wave; ++i) run += part[1][i];
  const unsigned num = run * 255u, a32 = (unsigned)area;          // run <= area < 2^24
  unsigned q = num / a32;
  const unsigned rem = num - q * a32;
  if (2u * rem > a32 || (2u * rem == a32 && (q & 1u))) q += 1u;   // round half to even
  lut[(slot * CL_TILES + tile) * CL_BINS + tid] = (uint8_t)(q > 255u ? 255u : q);
}

void clahe_launch_lut(const uint8_t* images, const int32_t* table, int words, int views, int n, int h, int w, const float* mid,
                      const float* field, uint8_t* lut, hipStream_t st) {
  if (words == TA_WORDS)
    hipLaunchKernelGGL(clahe_lut_kernel<true>, dim3(CL_TILES, n, views), dim3(256), 0, st, images, table, (const f32x4*)mid,
                       (const ta_f2*)field, n, h, w, lut);
  else
    hipLaunchKernelGGL(clahe_lut_kernel<false>, dim3(CL_TILES, n, views), dim3(256), 0, st, images, table, (const f32x4*)mid,
                       (const ta_f2*)field, n, h, w, lut);
}

}  // namespace udaseg

using namespace udaseg;

extern "C" int udaseg_clahe_lut_u8(const uint8_t* images, const int32_t* table, int words, int views, int n, int h, int w,
                                   const float* mid, const float* field, uint8_t* lut, void* stream) {
  UDASEG_CHECK_ARG(images && table && lut && n > 0 && h > 0 && w > 0, "clahe_lut_u8: bad arguments");
  UDASEG_CHECK_ARG(words == SA_WORDS || words == TA_WORDS, "clahe_lut_u8: records have %d or %d words", SA_WORDS, TA_WORDS);
  UDASEG_CHECK_ARG(views == 1 || (views == 2 && words == SA_WORDS), "clahe_lut_u8: views must be 1, or 2 for the 32-word records");
  UDASEG_CHECK_ARG(h % CL_GRID == 0 && w % CL_GRID == 0, "clahe_lut_u8: the frame sides must be multiples of %d", CL_GRID);
  UDASEG_CHECK_ARG((int64_t)h * w < (1LL << 30) && n <= 65535, "clahe_lut_u8: batch too large");
  UDASEG_CHECK_ARG(((uintptr_t)mid & 15) == 0 && ((uintptr_t)field & 7) == 0, "clahe_lut_u8: mid must be 16-byte, field 8-byte aligned");
  clahe_launch_lut(images, table, words, views, n, h, w, mid, field, lut, as_stream(stream));
  UDASEG_LAUNCH_CHECK("clahe_lut launch");
  return UDASEG_OK;
}
