// The two device augmentation pipelines: the strong views of the phase-3 (unsupervised fine-tuning) step and the labelled
// training batches -- what the reference does per image on the host with albumentations (src/models/unsupervised_trainer.py:
// 100-114, src/models/augmentation.py:8-88), as a deterministic function of (uint8 frame, uint8 mask, parameter record).  The
// pipelines are defined in INTEGRATION.md ("Phase 3", "Training augmentation"); in order:
//   1 D4   2 Gaussian noise (Philox4x32-10)   3 blur (box / median / motion, k in {3,5})   4 shift-scale-rotate (bilinear)
//   4b (training records) one of optical / grid / elastic distortion
//   5 one of sharpen / emboss / brightness-contrast / CLAHE   6 HSV shift   7 A.Normalize + channel-padded NHWC store
// All stages compute in fp32 on the 0..255 scale, nothing is rounded to uint8 in between, every neighbourhood or out-of-frame
// read takes reflect-101 borders.  Stages 4 and 4b are composed into ONE gather: output pixel p -> q(p) (the distortion, on
// stage 4's grid) -> r = M (q, 1) (the inverse affine map); the image is sampled bilinearly once at r, the mask nearest at r by
// the same thread.  The passes of a call, ONE kernel each for both pipelines:
//   field pass   (training; only for samples on elastic): the smoothed displacement field (elastic_field.hip)
//   source pass  (only for samples with noise or blur): D4 gather + noise into an LDS tile with a 2-pixel halo, blur from the
//                tile, fp32 intermediate [views][n][h][w][4]
//   table pass   (only the *_clahe_u8 calls, for samples on CLAHE): the 8 x 8 lightness tables (clahe.hip)
//   output pass  the composed gather (4 bilinear taps, x 9 for the 3x3 stage) from that intermediate -- or straight from the
//                uint8 frame through the D4 code when the sample has neither noise nor blur -- then the point-wise stages, the
//                image store and (training) the mask store.
// A record with every stage off therefore costs one pass and computes exactly udaseg_prepare_batch_u8's arithmetic, image and
// mask.  Stage selection is per sample (blockIdx.y) and per view (blockIdx.z; the training call has one): every branch on the
// record is uniform over the block.  TRAIN selects the 64-word record, stage 4b and the mask; the strong instantiations carry
// none of the geometry.
#include "aug_common.h"

namespace udaseg {

__global__ __launch_bounds__(256) void aug_source_kernel(const uint8_t* __restrict__ images, const int32_t* __restrict__ table,
                                                         int words, int n, int h, int w, f32x4* __restrict__ mid) {
  const int ni = blockIdx.y;
  const size_t slot = (size_t)blockIdx.z * n + ni;
  const SaRec rec = sa_load(table + slot * words);
  if (!(rec.flags & (SA_NOISE | SA_BLUR))) return;            // block-uniform: the output pass reads the frame itself
  sa_source_pass(images, rec, ni, slot, h, w, mid);
}

// the output pass.  CLAHE = false is the kernel of udaseg_strong_aug_u8 / udaseg_train_aug_u8 (lut is not read); CLAHE = true
// adds stage-5 kind 3 (the slot's table from the table pass, clahe.hip) and leaves every other branch as it is written here.
// The mask never sees stage 5.  slot = view * n + ni indexes everything but the frame.
template <bool TRAIN, bool BF16, bool CLAHE>
__global__ __launch_bounds__(256) void aug_output_kernel(const uint8_t* __restrict__ images, const uint8_t* __restrict__ masks,
                                                         const int32_t* __restrict__ table, const f32x4* __restrict__ mid,
                                                         const ta_f2* __restrict__ field, int n, int h, int w, Normalize3 nm,
                                                         void* __restrict__ out, int cpad, int64_t* __restrict__ out_masks,
                                                         const uint8_t* __restrict__ lut) {
  __shared__ float grid_tab[TRAIN ? 24 : 1];
  const int ni = blockIdx.y;
  const size_t slot = (size_t)blockIdx.z * n + ni;
  const int hw = h * w;
  const AugBlock b = aug_block<TRAIN>(table + slot * (TRAIN ? TA_WORDS : SA_WORDS), images, mid, field, ni, slot, h, w, grid_tab);
  const SaRec& rec = b.rec.s;
  const uint8_t* msk = (TRAIN && masks) ? masks + slot * hw : nullptr;
  const bool conv3 = (rec.flags & SA_STAGE5) && rec.s5_kind < 2;
  float k3[9];
  if (conv3) sa_kernel3(rec, k3);
  for (int pix = blockIdx.x * 256 + threadIdx.x; pix < hw; pix += gridDim.x * 256) {
    const int y = pix / w, x = pix - y * w;
    float v[3];
    if (conv3) {
      float acc[3] = {0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const int yy = reflect101(y + i - 1, h);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          float t[3];
          aug_stage4<TRAIN>(b, yy, reflect101(x + j - 1, w), t);
#pragma unroll
          for (int c = 0; c < 3; ++c) acc[c] += k3[i * 3 + j] * t[c];
        }
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c] = clamp255(acc[c]);
    } else if (CLAHE && (rec.flags & SA_STAGE5) && rec.s5_kind == SA_CLAHE) {
      aug_stage4<TRAIN>(b, y, x, v);
      cl_apply(v, lut + slot * (CL_TILES * CL_BINS), y, x, h / CL_GRID, w / CL_GRID);
    } else {
      aug_stage4<TRAIN>(b, y, x, v);
      if (rec.flags & SA_STAGE5) {                               // brightness-contrast: v (1 + c) + 255 b
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = clamp255(v[c] * (1.f + rec.p5b) + 255.f * rec.p5a);
      }
    }
    if (rec.flags & SA_HSV) sa_hsv_shift(v, rec.dh, rec.ds, rec.dv);
    store_normalized<BF16>(out, (slot * hw + pix) * cpad, cpad, nm, v[0], v[1], v[2]);
    if (TRAIN && msk) {                                          // the label nearest to the same r, through the D4 code
      int my = y, mx = x;
      if (b.geo.affine | b.geo.kind) {
        float sx, sy;
        ta_position(b.geo, b.rec, y, x, h, w, sx, sy);
        mx = reflect101((int)floorf(sx + 0.5f), w);
        my = reflect101((int)floorf(sy + 0.5f), h);
      }
      out_masks[slot * hw + pix] = (int64_t)msk[d4_source(b.src.d4, my, mx, h, w)];
    }
  }
}

__global__ void philox_debug_kernel(const int32_t* __restrict__ counters, const int32_t* __restrict__ keys, int32_t* __restrict__ out,
                                    int count) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  uint32_t r[4];
  philox4x32_10((uint32_t)counters[4 * i], (uint32_t)counters[4 * i + 1], (uint32_t)counters[4 * i + 2], (uint32_t)counters[4 * i + 3],
                (uint32_t)keys[2 * i], (uint32_t)keys[2 * i + 1], r);
#pragma unroll
  for (int k = 0; k < 4; ++k) out[4 * i + k] = (int32_t)r[k];
}

}  // namespace udaseg

using namespace udaseg;

// every pass of a call of either pipeline: field -> source -> table (clahe) -> output.  The strong entry points pass no masks,
// no field and field_pass = 0; the training entry points pass views = 1.
static int aug_run(const char* who, bool train, bool clahe, const uint8_t* images, const uint8_t* masks, const int32_t* table, int views,
                   int n, int h, int w, float* mid, float* field, const float* gauss_weights, int radius, const float* mean255,
                   const float* inv_std255, void* out_images, int cpad, int out_bf16, int64_t* out_masks, int source_pass,
                   int field_pass, uint8_t* lut, void* stream) {
  UDASEG_CHECK_ARG(images && table && out_images && mean255 && inv_std255 && n > 0 && h > 0 && w > 0, "%s: bad arguments", who);
  UDASEG_CHECK_ARG(train || views == 1 || views == 2, "%s: views must be 1 or 2", who);
  UDASEG_CHECK_ARG(cpad >= 4 && cpad % (out_bf16 ? 8 : 4) == 0, "%s: cpad must be a multiple of %d", who, out_bf16 ? 8 : 4);
  UDASEG_CHECK_ARG((int64_t)h * w < (1LL << 30) && n <= 65535, "%s: batch too large", who);
  UDASEG_CHECK_ARG((masks == nullptr) == (out_masks == nullptr), "%s: masks and out_masks go together", who);
  UDASEG_CHECK_ARG(!source_pass || mid, "%s: the source pass needs the intermediate buffer", who);
  UDASEG_CHECK_ARG(!field_pass || (field && gauss_weights), "%s: the field pass needs the field buffer and the weights", who);
  UDASEG_CHECK_ARG(!field_pass || (radius >= 0 && radius <= TA_MAX_RADIUS), "%s: radius must be 0..%d", who, TA_MAX_RADIUS);
  UDASEG_CHECK_ARG(((uintptr_t)mid & 15) == 0 && ((uintptr_t)out_images & 15) == 0, "%s: buffers must be 16-byte aligned", who);
  UDASEG_CHECK_ARG(((uintptr_t)field & 7) == 0 && ((uintptr_t)out_masks & 7) == 0, "%s: field and out_masks must be 8-byte aligned", who);
  UDASEG_CHECK_ARG(!clahe || lut, "%s: the table pass needs the table buffer", who);
  UDASEG_CHECK_ARG(!clahe || (h % CL_GRID == 0 && w % CL_GRID == 0), "%s: the frame sides must be multiples of %d", who, CL_GRID);
  hipStream_t st = as_stream(stream);
  const int words = train ? TA_WORDS : SA_WORDS;
  if (field_pass) {
    elastic_launch_field(table, n, h, w, gauss_weights, radius, field, st);
    UDASEG_LAUNCH_CHECK("train_aug field pass launch");
  }
  if (source_pass) {
    const int tiles = cdiv(h, SA_TILE) * cdiv(w, SA_TILE);
    hipLaunchKernelGGL(aug_source_kernel, dim3(tiles, n, views), dim3(256), 0, st, images, table, words, n, h, w, (f32x4*)mid);
    UDASEG_LAUNCH_CHECK(train ? "train_aug source pass launch" : "strong_aug source pass launch");
  }
  if (clahe) {
    clahe_launch_lut(images, table, words, views, n, h, w, source_pass ? mid : nullptr, field, lut, st);
    UDASEG_LAUNCH_CHECK(train ? "train_aug table pass launch" : "strong_aug table pass launch");
  }
  const int gx = (h * w + 255) / 256 > 1024 ? 1024 : (h * w + 255) / 256;
  const Normalize3 nm = normalize3(mean255, inv_std255);
#define UDASEG_AUG_OUTPUT(TRAIN, BF16, CLAHE)                                                                                        \
  case (TRAIN ? 4 : 0) | (BF16 ? 2 : 0) | (CLAHE ? 1 : 0):                                                                          \
    hipLaunchKernelGGL((aug_output_kernel<TRAIN, BF16, CLAHE>), dim3(gx, n, views), dim3(256), 0, st, images, masks, table,         \
                       (const f32x4*)mid, (const ta_f2*)field, n, h, w, nm, out_images, cpad, out_masks, (const uint8_t*)lut);      \
    break
  switch ((train ? 4 : 0) | (out_bf16 ? 2 : 0) | (clahe ? 1 : 0)) {
    UDASEG_AUG_OUTPUT(false, false, false);
    UDASEG_AUG_OUTPUT(false, false, true);
    UDASEG_AUG_OUTPUT(false, true, false);
    UDASEG_AUG_OUTPUT(false, true, true);
    UDASEG_AUG_OUTPUT(true, false, false);
    UDASEG_AUG_OUTPUT(true, false, true);
    UDASEG_AUG_OUTPUT(true, true, false);
    UDASEG_AUG_OUTPUT(true, true, true);
  }
#undef UDASEG_AUG_OUTPUT
  UDASEG_LAUNCH_CHECK(train ? "train_aug output pass launch" : "strong_aug output pass launch");
  return UDASEG_OK;
}

extern "C" int udaseg_strong_aug_u8(const uint8_t* images, const int32_t* table, int views, int n, int h, int w, float* mid,
                                    const float* mean255, const float* inv_std255, void* out_images, int cpad, int out_bf16,
                                    int source_pass, void* stream) {
  return aug_run("strong_aug_u8", false, false, images, nullptr, table, views, n, h, w, mid, nullptr, nullptr, 0, mean255, inv_std255,
                 out_images, cpad, out_bf16, nullptr, source_pass, 0, nullptr, stream);
}

extern "C" int udaseg_strong_aug_clahe_u8(const uint8_t* images, const int32_t* table, int views, int n, int h, int w, float* mid,
                                          const float* mean255, const float* inv_std255, void* out_images, int cpad, int out_bf16,
                                          int source_pass, uint8_t* lut, void* stream) {
  return aug_run("strong_aug_clahe_u8", false, true, images, nullptr, table, views, n, h, w, mid, nullptr, nullptr, 0, mean255,
                 inv_std255, out_images, cpad, out_bf16, nullptr, source_pass, 0, lut, stream);
}

extern "C" int udaseg_train_aug_u8(const uint8_t* images, const uint8_t* masks, const int32_t* table, int n, int h, int w, float* mid,
                                   float* field, const float* gauss_weights, int radius, const float* mean255,
                                   const float* inv_std255, void* out_images, int cpad, int out_bf16, int64_t* out_masks,
                                   int source_pass, int field_pass, void* stream) {
  return aug_run("train_aug_u8", true, false, images, masks, table, 1, n, h, w, mid, field, gauss_weights, radius, mean255, inv_std255,
                 out_images, cpad, out_bf16, out_masks, source_pass, field_pass, nullptr, stream);
}

extern "C" int udaseg_train_aug_clahe_u8(const uint8_t* images, const uint8_t* masks, const int32_t* table, int n, int h, int w,
                                         float* mid, float* field, const float* gauss_weights, int radius, const float* mean255,
                                         const float* inv_std255, void* out_images, int cpad, int out_bf16, int64_t* out_masks,
                                         int source_pass, int field_pass, uint8_t* lut, void* stream) {
  return aug_run("train_aug_clahe_u8", true, true, images, masks, table, 1, n, h, w, mid, field, gauss_weights, radius, mean255,
                 inv_std255, out_images, cpad, out_bf16, out_masks, source_pass, field_pass, lut, stream);
}

extern "C" int udaseg_philox4x32_debug(const int32_t* counters, const int32_t* keys, int32_t* out, int count, void* stream) {
  UDASEG_CHECK_ARG(counters && keys && out && count > 0, "philox4x32_debug: bad arguments");
  hipLaunchKernelGGL(philox_debug_kernel, dim3(cdiv(count, 64)), dim3(64), 0, as_stream(stream), counters, keys, out, count);
  UDASEG_LAUNCH_CHECK("philox4x32_debug launch");
  return UDASEG_OK;
}
