// Cross-domain class mixing of a source and a target batch on the device (DACS, Tranheden et al. 2021; ClassMix, Olsson et al.
// 2021; an extension: the reference has no counterpart).  Between "pseudo-label the target batch" and "augment and train" a
// self-training loop pastes the pixels, frame and label, of half of the classes of a source mask onto a target frame and its
// pseudo-label mask.  With torch that is unique -> a host round trip -> randperm -> isin -> three where; here the existing mask
// histogram (udaseg_mask_hist_u8), one tiny selection kernel (udaseg_classmix_select) and one streaming pass (udaseg_classmix_u8).
// Integers only: every output is exact, and mix.py's selection_from_hist is the host mirror bit for bit.
//
// The mixing pass moves 12 bytes per pixel (reads 3 + 1 + 3 + 1, writes 3 + 1) and has two forms with identical bytes:
//   wide    16 pixels per lane: three 16-byte loads per frame operand, one per mask operand, the matching 16-byte stores.  Taken
//           when h * w % 16 == 0 (no chunk straddles two samples, whose selections differ) and every operand is 16-byte aligned.
//   scalar  one pixel per lane, byte accesses: everything else.
// The host chooses per launch.  A block belongs to ONE sample (blockIdx.x / bx), so the selection word and the box are
// block-uniform, and it strides over the sample's chunks with its bx - 1 siblings; n * bx stays near MIX_MAX_BLOCKS.  Counts:
// per lane in registers, summed over the wave, one LDS atomic per wave and one 64-bit global atomic per non-zero counter per block.
#include "aug_common.h"

namespace udaseg {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int MIX_THREADS = 256;
static_assert(MIX_THREADS == 64 * 4, "BlockCounts<K>: four waves a block");
constexpr int MIX_MAX_BLOCKS = 2048;
constexpr int SEL_THREADS = 64;

// one sample per thread; the present list of thread t is column t of LDS (a byte per class)
__global__ __launch_bounds__(SEL_THREADS) void classmix_select_kernel(const unsigned long long* __restrict__ hist, int n, int classes,
                                                                      unsigned long long min_pixels, const int32_t* __restrict__ keys,
                                                                      int32_t* __restrict__ sel) {
  __shared__ uint8_t present[32][SEL_THREADS];
  const int i = blockIdx.x * SEL_THREADS + threadIdx.x;
  if (i >= n) return;
  const unsigned long long* row = hist + (size_t)i * 256;
  int P = 0;
  for (int c = 0; c < classes; ++c)
    if (row[c] >= min_pixels) present[P++][threadIdx.x] = (uint8_t)c;
  const int k = (P + 1) >> 1;
  const uint32_t k0 = (uint32_t)keys[2 * i], k1 = (uint32_t)keys[2 * i + 1];
  uint32_t bits = 0;
  for (int j = 0; j < k; ++j) {
    uint32_t r[4];
    philox4x32_10((uint32_t)j, 0u, 0u, 0u, k0, k1, r);
    const int t = j + (int)__umulhi(r[0], (uint32_t)(P - j));             // j <= t < P
    const uint8_t a = present[j][threadIdx.x], b = present[t][threadIdx.x];
    present[j][threadIdx.x] = b;
    present[t][threadIdx.x] = a;
    bits |= 1u << b;
  }
  sel[i] = (int32_t)bits;
}

struct MixBox { int y0, x0, y1, x1; };

// what a block forms once: its sample, the selection among the classes, the box (empty without boxes)
struct MixBlock {
  int i, b;
  uint32_t sel;
  MixBox box;
};

__device__ __forceinline__ MixBlock mix_block(const int32_t* __restrict__ sel, const int32_t* __restrict__ boxes, int bx, int classes) {
  MixBlock k;
  k.i = blockIdx.x / bx;
  k.b = blockIdx.x - k.i * bx;
  k.sel = (uint32_t)sel[k.i] & (classes == 32 ? 0xffffffffu : (1u << classes) - 1u);
  k.box = MixBox{0, 0, 0, 0};
  if (boxes) k.box = MixBox{boxes[4 * k.i], boxes[4 * k.i + 1], boxes[4 * k.i + 2], boxes[4 * k.i + 3]};
  return k;
}

__device__ __forceinline__ bool mix_pasted(const MixBlock& k, uint32_t s, int y, int x) {
  const bool cls = s < 32u && ((k.sel >> (s & 31u)) & 1u);                // k.sel holds no bit at or above classes
  return cls || (y >= k.box.y0 && y < k.box.y1 && x >= k.box.x0 && x < k.box.x1);
}

__global__ __launch_bounds__(MIX_THREADS) void classmix_wide_kernel(const uint8_t* __restrict__ src, const uint8_t* __restrict__ src_masks,
                                                                    const uint8_t* __restrict__ tgt, const uint8_t* __restrict__ tgt_masks,
                                                                    const int32_t* __restrict__ sel, const int32_t* __restrict__ boxes,
                                                                    int hw, int w, int bx, int classes, int void_label,
                                                                    uint8_t* __restrict__ out, uint8_t* __restrict__ out_masks,
                                                                    unsigned long long* __restrict__ counts) {
  __shared__ BlockCounts<3>::Slots cnt;
  const MixBlock k = mix_block(sel, boxes, bx, classes);
  const size_t base = (size_t)k.i * hw;                                   // hw % 16 == 0: every chunk below is 16-byte aligned
  const u32x4* ps = reinterpret_cast<const u32x4*>(src + base * 3);
  const u32x4* pt = reinterpret_cast<const u32x4*>(tgt + base * 3);
  const u32x4* pms = reinterpret_cast<const u32x4*>(src_masks + base);
  const u32x4* pmt = tgt_masks ? reinterpret_cast<const u32x4*>(tgt_masks + base) : nullptr;
  u32x4* po = reinterpret_cast<u32x4*>(out + base * 3);
  u32x4* pmo = reinterpret_cast<u32x4*>(out_masks + base);
  const unsigned int vw = (unsigned int)void_label * 0x01010101u;
  const int chunks = hw >> 4;
  unsigned int c0 = 0, c1 = 0;
  int done = 0;
  for (int ch = k.b * MIX_THREADS + threadIdx.x; ch < chunks; ch += bx * MIX_THREADS) {
    unsigned int fs[12], ft[12], ms[4], mt[4];
#pragma unroll
    for (int v = 0; v < 3; ++v) {
      const u32x4 a = ps[3 * ch + v], b = pt[3 * ch + v];
#pragma unroll
      for (int e = 0; e < 4; ++e) { fs[4 * v + e] = a[e]; ft[4 * v + e] = b[e]; }
    }
    {
      const u32x4 a = pms[ch];
      u32x4 b = {vw, vw, vw, vw};
      if (pmt) b = pmt[ch];
#pragma unroll
      for (int e = 0; e < 4; ++e) { ms[e] = a[e]; mt[e] = b[e]; }
    }
    const int q = ch << 4;
    int y = 0, x = 0;
    if (boxes) { y = q / w; x = q - y * w; }
    unsigned int pasted = 0, valid = 0;                                   // bit j: pixel q + j
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const uint32_t s = (ms[j >> 2] >> (8 * (j & 3))) & 0xffu;
      const uint32_t t = (mt[j >> 2] >> (8 * (j & 3))) & 0xffu;
      pasted |= (mix_pasted(k, s, y, x) ? 1u : 0u) << j;
      valid |= ((int)t < classes ? 1u : 0u) << j;
      if (boxes && ++x == w) { x = 0; ++y; }
    }
    u32x4 o[3], om;
#pragma unroll
    for (int v = 0; v < 12; ++v) {                                        // byte e of word v belongs to pixel (4 v + e) / 3
      unsigned int bm = 0;
#pragma unroll
      for (int e = 0; e < 4; ++e) bm |= (0u - ((pasted >> ((4 * v + e) / 3)) & 1u)) & (0xffu << (8 * e));
      o[v >> 2][v & 3] = (fs[v] & bm) | (ft[v] & ~bm);
    }
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      unsigned int bm = 0;
#pragma unroll
      for (int e = 0; e < 4; ++e) bm |= (0u - ((pasted >> (4 * v + e)) & 1u)) & (0xffu << (8 * e));
      om[v] = (ms[v] & bm) | (mt[v] & ~bm);
    }
#pragma unroll
    for (int v = 0; v < 3; ++v) po[3 * ch + v] = o[v];
    pmo[ch] = om;
    c0 += __popc(pasted);
    c1 += __popc(~pasted & valid);
    done += 16;
  }
  const unsigned int ev[3] = {c0, c1, (unsigned int)done - c0 - c1};
  if (counts) BlockCounts<3>::add(cnt, ev, counts + (size_t)k.i * 3);     // uniform over the block
}

__global__ __launch_bounds__(MIX_THREADS) void classmix_scalar_kernel(const uint8_t* __restrict__ src, const uint8_t* __restrict__ src_masks,
                                                                      const uint8_t* __restrict__ tgt, const uint8_t* __restrict__ tgt_masks,
                                                                      const int32_t* __restrict__ sel, const int32_t* __restrict__ boxes,
                                                                      int hw, int w, int bx, int classes, int void_label,
                                                                      uint8_t* __restrict__ out, uint8_t* __restrict__ out_masks,
                                                                      unsigned long long* __restrict__ counts) {
  __shared__ BlockCounts<3>::Slots cnt;
  const MixBlock k = mix_block(sel, boxes, bx, classes);
  const size_t base = (size_t)k.i * hw;
  unsigned int c0 = 0, c1 = 0, c2 = 0;
  for (unsigned int q = k.b * MIX_THREADS + threadIdx.x; q < (unsigned int)hw; q += bx * MIX_THREADS) {   // hw < 2^31: no wrap
    const size_t p = base + q;
    const uint32_t s = src_masks[p];
    const uint32_t t = tgt_masks ? (uint32_t)tgt_masks[p] : (uint32_t)void_label;
    const int y = (int)(q / (unsigned int)w), x = (int)(q - (unsigned int)y * (unsigned int)w);
    const bool m = mix_pasted(k, s, y, x);
    const uint8_t* f = (m ? src : tgt) + p * 3;
    out[p * 3 + 0] = f[0];
    out[p * 3 + 1] = f[1];
    out[p * 3 + 2] = f[2];
    out_masks[p] = (uint8_t)(m ? s : t);
    if (m) ++c0;
    else if ((int)t < classes) ++c1;
    else ++c2;
  }
  const unsigned int ev[3] = {c0, c1, c2};
  if (counts) BlockCounts<3>::add(cnt, ev, counts + (size_t)k.i * 3);     // uniform over the block
}

static bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
  if (!a || !b) return false;
  const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
  return pa < pb + nb && pb < pa + na;
}

}  // namespace udaseg

using namespace udaseg;

extern "C" int udaseg_classmix_select(const int64_t* hist, int n, int classes, int64_t min_pixels, const int32_t* keys, int32_t* sel,
                                      void* stream) {
  UDASEG_CHECK_ARG(hist && keys && sel, "classmix_select: NULL pointer");
  UDASEG_CHECK_ARG(n > 0, "classmix_select: need n > 0 (n=%d)", n);
  UDASEG_CHECK_ARG(classes >= 1 && classes <= 32, "classmix_select: need 1 <= classes <= 32 (classes=%d)", classes);
  UDASEG_CHECK_ARG(min_pixels >= 1, "classmix_select: need min_pixels >= 1 (min_pixels=%lld)", (long long)min_pixels);
  const size_t sel_bytes = (size_t)n * 4;
  UDASEG_CHECK_ARG(!ranges_overlap(sel, sel_bytes, hist, (size_t)n * 256 * 8) && !ranges_overlap(sel, sel_bytes, keys, (size_t)n * 8),
                   "classmix_select: sel overlaps an input");
  hipLaunchKernelGGL(classmix_select_kernel, dim3(cdiv(n, SEL_THREADS)), dim3(SEL_THREADS), 0, as_stream(stream),
                     (const unsigned long long*)hist, n, classes, (unsigned long long)min_pixels, keys, sel);
  UDASEG_LAUNCH_CHECK("classmix_select launch");
  return UDASEG_OK;
}

extern "C" int udaseg_classmix_u8(const uint8_t* src, const uint8_t* src_masks, const uint8_t* tgt, const uint8_t* tgt_masks,
                                  const int32_t* sel, const int32_t* boxes, int n, int h, int w, int classes, int void_label,
                                  uint8_t* out, uint8_t* out_masks, int64_t* counts, void* stream) {
  UDASEG_CHECK_ARG(src && src_masks && tgt && sel && out && out_masks, "classmix_u8: NULL pointer");
  UDASEG_CHECK_ARG(n > 0 && h > 0 && w > 0 && (int64_t)n * h * w < ((int64_t)1 << 31),
                   "classmix_u8: need n, h, w > 0 and n*h*w < 2^31 (n=%d h=%d w=%d)", n, h, w);
  UDASEG_CHECK_ARG(classes >= 1 && classes <= 32, "classmix_u8: need 1 <= classes <= 32 (classes=%d)", classes);
  UDASEG_CHECK_ARG(void_label >= classes && void_label <= 255, "classmix_u8: need classes <= void_label <= 255 (void_label=%d classes=%d)",
                   void_label, classes);
  const int hw = h * w;
  const size_t px = (size_t)n * hw;
  const void* ins[6] = {src, src_masks, tgt, tgt_masks, sel, boxes};
  const size_t in_bytes[6] = {px * 3, px, px * 3, px, (size_t)n * 4, (size_t)n * 16};
  const void* outs[3] = {out, out_masks, counts};
  const size_t out_bytes[3] = {px * 3, px, (size_t)n * 24};
  for (int o = 0; o < 3; ++o) {
    for (int i = 0; i < 6; ++i)
      UDASEG_CHECK_ARG(!ranges_overlap(outs[o], out_bytes[o], ins[i], in_bytes[i]), "classmix_u8: output %d overlaps input %d", o, i);
    for (int p = 0; p < o; ++p)
      UDASEG_CHECK_ARG(!ranges_overlap(outs[o], out_bytes[o], outs[p], out_bytes[p]), "classmix_u8: outputs %d and %d overlap", p, o);
  }
  uintptr_t align = reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(out_masks);
  for (int i = 0; i < 4; ++i) align |= reinterpret_cast<uintptr_t>(ins[i]);   // NULL adds nothing
  const bool wide = hw % 16 == 0 && (align & 15) == 0;
  const int cap = n >= MIX_MAX_BLOCKS ? 1 : MIX_MAX_BLOCKS / n;             // blocks per sample
  int bx = cdiv(wide ? hw / 16 : hw, MIX_THREADS);
  if (bx > cap) bx = cap;
  const dim3 grid((unsigned int)((int64_t)n * bx));                         // <= n*h*w < 2^31
  if (wide)
    hipLaunchKernelGGL(classmix_wide_kernel, grid, dim3(MIX_THREADS), 0, as_stream(stream), src, src_masks, tgt, tgt_masks, sel, boxes,
                       hw, w, bx, classes, void_label, out, out_masks, (unsigned long long*)counts);
  else
    hipLaunchKernelGGL(classmix_scalar_kernel, grid, dim3(MIX_THREADS), 0, as_stream(stream), src, src_masks, tgt, tgt_masks, sel, boxes,
                       hw, w, bx, classes, void_label, out, out_masks, (unsigned long long*)counts);
  UDASEG_LAUNCH_CHECK("classmix_u8 launch");
  return UDASEG_OK;
}
