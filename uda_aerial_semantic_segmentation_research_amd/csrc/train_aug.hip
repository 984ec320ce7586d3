// Labelled training augmentation on the device: the reference's get_training_augmentation() (src/models/augmentation.py:8-38)
// as a deterministic function of (uint8 frame, uint8 mask, parameter record).  The pipeline is defined in INTEGRATION.md
// ("Training augmentation"); in order:
//   1 D4   2 Gaussian noise   3 blur   4 shift-scale-rotate   4b one of optical / grid / elastic distortion
//   5 one of sharpen / emboss / brightness-contrast   6 HSV shift   7 A.Normalize + channel-padded NHWC store
// Stages 1-3 and 5-7 are the strong pipeline's (aug_common.h, strong_aug.hip) and touch the image only.  Stages 4 and 4b are
// composed into ONE gather: output pixel p -> q(p) (the distortion, on stage 4's grid) -> r = M (q, 1) (the inverse affine map);
// the image is sampled bilinearly once at r, the mask nearest at r by the same thread.  Up to three kernels per call:
//   field pass   (only for samples on elastic): the smoothed displacement field G, float2 [n][h][w]
//   source pass  (only for samples with noise or blur): stages 1-3 into the fp32 intermediate, as strong_aug.hip
//   output pass  the composed gather (x 9 for the 3x3 stage), the point-wise stages, the image store and the mask store
// A record with every stage off computes exactly udaseg_prepare_batch_u8's arithmetic, image and mask.
// Stage selection is per sample (blockIdx.y): every branch on the record is uniform over the block.
// udaseg_train_aug_clahe_u8 is the same call for batches with a record on CLAHE (stage-5 kind 3): the table pass (clahe.hip)
// runs in front of the output pass, which is the variant with that one more stage-5 branch; the record, the geometry and the
// composed gather (TaRec, TaGeo, ta_stage4) live in aug_common.h, where the table pass finds them too.
#include "aug_common.h"

namespace udaseg {

// ------------------------------------------------------------------------------------------------------ the elastic field
// G = separable Gaussian (radius R, reflect-101 at any distance) of the raw field (2 u0 - 1, 2 u1 - 1), u = the first two
// uniforms of Philox4x32-10 at counter (y w + x, 1, 0, 0) under the record's elastic key.  One kernel, no global intermediate:
// a block owns a 32 x 32 tile; the raw values of the tile and its R-wide halo go into one LDS plane ((32 + 2R)^2 float2), the
// horizontal pass writes a second plane ((32 + 2R) x 32 float2), the vertical pass goes to global.  At R = 18 the planes take
// 36 992 + 17 408 bytes, next to each other below the 64 KiB a block may have.  The halo is recomputed, not exchanged: a block
// evaluates (32 + 2R)^2 / 32^2 generator calls per output pixel, 4.5 at R = 18 (a Philox call is ~70 integer operations; the two
// filter passes cost 2 x (3.1 + 1) x (2R + 1) = 230 multiply-adds per pixel there and dominate).  A wider tile would recompute
// less but the two planes no longer fit side by side (64 x 32: 68 KiB).  Only samples on elastic pay for any of it.
__global__ __launch_bounds__(256) void elastic_field_kernel(const int32_t* __restrict__ table, int h, int w, TaWeights gw, int radius,
                                                            ta_f2* __restrict__ field) {
  __shared__ ta_f2 raw[TA_FS * TA_FS];
  __shared__ ta_f2 hp[TA_FS * TA_FT];
  __shared__ float wt[2 * TA_MAX_RADIUS + 1];
  const int ni = blockIdx.y;
  const int32_t* t = table + (size_t)ni * TA_WORDS;
  if (!((t[0] & TA_DISTORT) && t[32] == TA_ELASTIC)) return;      // block-uniform
  const uint32_t k0 = (uint32_t)t[50], k1 = (uint32_t)t[51];
  const int taps = 2 * radius + 1, side = TA_FT + 2 * radius;
  if ((int)threadIdx.x < taps) wt[threadIdx.x] = gw.w[threadIdx.x];
  const int tiles_x = (w + TA_FT - 1) / TA_FT;
  const int ty0 = (blockIdx.x / tiles_x) * TA_FT, tx0 = (blockIdx.x % tiles_x) * TA_FT;
  for (int i = threadIdx.x; i < side * side; i += 256) {
    const int ly = i / side, lx = i - ly * side;
    const int y = reflect101(ty0 - radius + ly, h), x = reflect101(tx0 - radius + lx, w);
    uint32_t r[4];
    philox4x32_10((uint32_t)(y * w + x), 1u, 0u, 0u, k0, k1, r);
    raw[i] = ta_f2{2.f * sa_uniform(r[0]) - 1.f, 2.f * sa_uniform(r[1]) - 1.f};
  }
  __syncthreads();
  for (int i = threadIdx.x; i < side * TA_FT; i += 256) {        // horizontal: every row of the plane, the tile's 32 columns
    const int ly = i / TA_FT, lx = i - ly * TA_FT;
    const ta_f2* src = raw + ly * side + lx;
    ta_f2 acc = {0.f, 0.f};
    for (int k = 0; k < taps; ++k) acc += wt[k] * src[k];
    hp[i] = acc;
  }
  __syncthreads();
  const int lx = threadIdx.x & (TA_FT - 1);
  const int x = tx0 + lx;
  for (int ly = threadIdx.x / TA_FT; ly < TA_FT; ly += 256 / TA_FT) {   // vertical
    const int y = ty0 + ly;
    if (y >= h || x >= w) continue;
    const ta_f2* src = hp + ly * TA_FT + lx;
    ta_f2 acc = {0.f, 0.f};
    for (int k = 0; k < taps; ++k) acc += wt[k] * src[k * TA_FT];
    field[((size_t)ni * h + y) * w + x] = acc;
  }
}

// ------------------------------------------------------------------------------------------------------------ source pass
__global__ __launch_bounds__(256) void train_source_kernel(const uint8_t* __restrict__ images, const int32_t* __restrict__ table,
                                                           int h, int w, f32x4* __restrict__ mid) {
  const int ni = blockIdx.y;
  const SaRec rec = sa_load(table + (size_t)ni * TA_WORDS);
  if (!(rec.flags & (SA_NOISE | SA_BLUR))) return;              // block-uniform: the output pass reads the frame itself
  sa_source_pass(images, rec, ni, (size_t)ni, h, w, mid);
}

// ------------------------------------------------------------------------------------------------------------ output pass
// the output pass.  CLAHE = false is the kernel of udaseg_train_aug_u8 (lut is not read); CLAHE = true adds stage-5 kind 3 (the
// sample's table from the table pass, clahe.hip) and leaves every other branch as it is written here.  The mask never sees it.
template <bool BF16, bool CLAHE>
__global__ __launch_bounds__(256) void train_output_kernel(const uint8_t* __restrict__ images, const uint8_t* __restrict__ masks,
                                                           const int32_t* __restrict__ table, const f32x4* __restrict__ mid,
                                                           const ta_f2* __restrict__ field, int h, int w, float m0, float m1, float m2,
                                                           float r0, float r1, float r2, void* __restrict__ out, int cpad,
                                                           int64_t* __restrict__ out_masks, const uint8_t* __restrict__ lut) {
  __shared__ float grid_tab[24];
  const int ni = blockIdx.y;
  const TaRec rec = ta_load(table + (size_t)ni * TA_WORDS);
  const int hw = h * w;
  SaSrc src;
  src.img = images + (size_t)ni * hw * 3;
  src.mid = (rec.s.flags & (SA_NOISE | SA_BLUR)) ? mid + (size_t)ni * hw : nullptr;
  src.d4 = sa_code(rec.s.d4, h, w); src.h = h; src.w = w;
  const TaGeo geo = ta_geometry(rec, field ? field + (size_t)ni * hw : nullptr, grid_tab, h, w);
  if (geo.kind == TA_GRID) ta_grid_table(table + (size_t)ni * TA_WORDS, geo.cw, geo.ch, grid_tab);     // block-uniform
  const uint8_t* msk = masks ? masks + (size_t)ni * hw : nullptr;
  const bool conv3 = (rec.s.flags & SA_STAGE5) && rec.s.s5_kind < 2;
  float k3[9];                                                   // the 3x3 stage's kernel (correlation, row-major)
  if (conv3) {
    const float a = rec.s.p5a, p = rec.s.p5b;
    if (rec.s.s5_kind == 0) {                                    // sharpen: (1-a) I + a [[-1,-1,-1],[-1,8+l,-1],[-1,-1,-1]]
#pragma unroll
      for (int i = 0; i < 9; ++i) k3[i] = -a;
      k3[4] = (1.f - a) + a * (8.f + p);
    } else {                                                     // emboss: (1-a) I + a [[-1-s,-s,0],[-s,1,s],[0,s,1+s]]
      k3[0] = a * (-1.f - p); k3[1] = a * -p; k3[2] = 0.f;
      k3[3] = a * -p; k3[4] = (1.f - a) + a; k3[5] = a * p;
      k3[6] = 0.f; k3[7] = a * p; k3[8] = a * (1.f + p);
    }
  }
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
          ta_stage4(src, geo, rec, yy, reflect101(x + j - 1, w), t);
#pragma unroll
          for (int c = 0; c < 3; ++c) acc[c] += k3[i * 3 + j] * t[c];
        }
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c] = clamp255(acc[c]);
    } else if (CLAHE && (rec.s.flags & SA_STAGE5) && rec.s.s5_kind == SA_CLAHE) {
      ta_stage4(src, geo, rec, y, x, v);
      cl_apply(v, lut + (size_t)ni * (CL_TILES * CL_BINS), y, x, h / CL_GRID, w / CL_GRID);
    } else {
      ta_stage4(src, geo, rec, y, x, v);
      if (rec.s.flags & SA_STAGE5) {                             // brightness-contrast: v (1 + c) + 255 b
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = clamp255(v[c] * (1.f + rec.s.p5b) + 255.f * rec.s.p5a);
      }
    }
    if (rec.s.flags & SA_HSV) sa_hsv_shift(v, rec.s.dh, rec.s.ds, rec.s.dv);
    const float v0 = (v[0] - m0) * r0, v1 = (v[1] - m1) * r1, v2 = (v[2] - m2) * r2;
    const size_t o = ((size_t)ni * hw + pix) * cpad;
    if (BF16) {
      __bf16* dst = reinterpret_cast<__bf16*>(out) + o;
      dst[0] = (__bf16)v0;
      dst[1] = (__bf16)v1;
      dst[2] = (__bf16)v2;
      for (int k = 3; k < cpad; ++k) dst[k] = (__bf16)0.f;
    } else {
      float* dst = reinterpret_cast<float*>(out) + o;
      *reinterpret_cast<f32x4*>(dst) = f32x4{v0, v1, v2, 0.f};
      for (int k = 4; k < cpad; ++k) dst[k] = 0.f;
    }
    if (msk) {                                                   // the label nearest to the same r, through the D4 code
      int my = y, mx = x;
      if (geo.affine | geo.kind) {
        float sx, sy;
        ta_position(geo, rec, y, x, h, w, sx, sy);
        mx = reflect101((int)floorf(sx + 0.5f), w);
        my = reflect101((int)floorf(sy + 0.5f), h);
      }
      out_masks[(size_t)ni * hw + pix] = (int64_t)msk[d4_source(src.d4, my, mx, h, w)];
    }
  }
}

static bool ta_weights(const float* gauss_weights, int radius, TaWeights& gw) {
  if (!gauss_weights || radius < 0 || radius > TA_MAX_RADIUS) return false;
  for (int i = 0; i < 2 * TA_MAX_RADIUS + 1; ++i) gw.w[i] = i < 2 * radius + 1 ? gauss_weights[i] : 0.f;
  return true;
}

static void ta_launch_field(const int32_t* table, int n, int h, int w, const TaWeights& gw, int radius, float* field, hipStream_t st) {
  const int tiles = cdiv(h, TA_FT) * cdiv(w, TA_FT);
  hipLaunchKernelGGL(elastic_field_kernel, dim3(tiles, n), dim3(256), 0, st, table, h, w, gw, radius, (ta_f2*)field);
}

}  // namespace udaseg

using namespace udaseg;

extern "C" int udaseg_elastic_field_f32(const int32_t* table, int n, int h, int w, const float* gauss_weights, int radius,
                                        float* field, void* stream) {
  UDASEG_CHECK_ARG(table && field && gauss_weights && n > 0 && h > 0 && w > 0, "elastic_field_f32: bad arguments");
  UDASEG_CHECK_ARG(radius >= 0 && radius <= TA_MAX_RADIUS, "elastic_field_f32: radius must be 0..%d", TA_MAX_RADIUS);
  UDASEG_CHECK_ARG((int64_t)h * w < (1LL << 30) && n <= 65535, "elastic_field_f32: batch too large");
  UDASEG_CHECK_ARG(((uintptr_t)field & 7) == 0, "elastic_field_f32: the field must be 8-byte aligned");
  TaWeights gw;
  ta_weights(gauss_weights, radius, gw);
  ta_launch_field(table, n, h, w, gw, radius, field, as_stream(stream));
  UDASEG_LAUNCH_CHECK("elastic_field launch");
  return UDASEG_OK;
}

// every pass of a call; clahe == false: today's launches, else the table pass goes in front of the output pass
static int train_aug_run(const char* who, const uint8_t* images, const uint8_t* masks, const int32_t* table, int n, int h, int w,
                         float* mid, float* field, const float* gauss_weights, int radius, const float* mean255,
                         const float* inv_std255, void* out_images, int cpad, int out_bf16, int64_t* out_masks, int source_pass,
                         int field_pass, uint8_t* lut, bool clahe, void* stream) {
  UDASEG_CHECK_ARG(images && table && out_images && mean255 && inv_std255 && n > 0 && h > 0 && w > 0, "%s: bad arguments", who);
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
  if (field_pass) {
    TaWeights gw;
    ta_weights(gauss_weights, radius, gw);
    ta_launch_field(table, n, h, w, gw, radius, field, st);
    UDASEG_LAUNCH_CHECK("train_aug field pass launch");
  }
  if (source_pass) {
    const int tiles = cdiv(h, SA_TILE) * cdiv(w, SA_TILE);
    hipLaunchKernelGGL(train_source_kernel, dim3(tiles, n), dim3(256), 0, st, images, table, h, w, (f32x4*)mid);
    UDASEG_LAUNCH_CHECK("train_aug source pass launch");
  }
  if (clahe) {
    clahe_launch_lut(images, table, TA_WORDS, 1, n, h, w, source_pass ? mid : nullptr, field, lut, st);
    UDASEG_LAUNCH_CHECK("train_aug table pass launch");
  }
  const int gx = (h * w + 255) / 256 > 1024 ? 1024 : (h * w + 255) / 256;
  const float m0 = mean255[0], m1 = mean255[1], m2 = mean255[2], r0 = inv_std255[0], r1 = inv_std255[1], r2 = inv_std255[2];
  const uint8_t* tab = lut;
#define UDASEG_TA_OUTPUT(BF16, CLAHE)                                                                                               \
  hipLaunchKernelGGL((train_output_kernel<BF16, CLAHE>), dim3(gx, n), dim3(256), 0, st, images, masks, table, (const f32x4*)mid,    \
                     (const ta_f2*)field, h, w, m0, m1, m2, r0, r1, r2, out_images, cpad, out_masks, tab)
  if (clahe) {
    if (out_bf16) UDASEG_TA_OUTPUT(true, true);
    else UDASEG_TA_OUTPUT(false, true);
  } else {
    if (out_bf16) UDASEG_TA_OUTPUT(true, false);
    else UDASEG_TA_OUTPUT(false, false);
  }
#undef UDASEG_TA_OUTPUT
  UDASEG_LAUNCH_CHECK("train_aug output pass launch");
  return UDASEG_OK;
}

extern "C" int udaseg_train_aug_u8(const uint8_t* images, const uint8_t* masks, const int32_t* table, int n, int h, int w, float* mid,
                                   float* field, const float* gauss_weights, int radius, const float* mean255,
                                   const float* inv_std255, void* out_images, int cpad, int out_bf16, int64_t* out_masks,
                                   int source_pass, int field_pass, void* stream) {
  return train_aug_run("train_aug_u8", images, masks, table, n, h, w, mid, field, gauss_weights, radius, mean255, inv_std255, out_images,
                       cpad, out_bf16, out_masks, source_pass, field_pass, nullptr, false, stream);
}

extern "C" int udaseg_train_aug_clahe_u8(const uint8_t* images, const uint8_t* masks, const int32_t* table, int n, int h, int w,
                                         float* mid, float* field, const float* gauss_weights, int radius, const float* mean255,
                                         const float* inv_std255, void* out_images, int cpad, int out_bf16, int64_t* out_masks,
                                         int source_pass, int field_pass, uint8_t* lut, void* stream) {
  return train_aug_run("train_aug_clahe_u8", images, masks, table, n, h, w, mid, field, gauss_weights, radius, mean255, inv_std255,
                       out_images, cpad, out_bf16, out_masks, source_pass, field_pass, lut, true, stream);
}
