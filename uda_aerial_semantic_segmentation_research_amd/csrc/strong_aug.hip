// Strong augmentation of the phase-3 (unsupervised fine-tuning) step on the device: what the reference does per image on the
// host with albumentations (src/models/unsupervised_trainer.py:100-114, src/models/augmentation.py:40-88), as a deterministic
// function of (uint8 frame, parameter record).  The pipeline is defined in INTEGRATION.md ("Phase 3"); in order:
//   1 D4   2 Gaussian noise (Philox4x32-10)   3 blur (box / median / motion, k in {3,5})   4 shift-scale-rotate (bilinear)
//   5 one of sharpen / emboss / brightness-contrast   6 HSV shift   7 A.Normalize + channel-padded NHWC store
// All stages compute in fp32 on the 0..255 scale, nothing is rounded to uint8 in between, every neighbourhood or out-of-frame
// read takes reflect-101 borders.  Two kernels for both views of a call:
//   source pass  (only for samples with noise or blur): D4 gather + noise into an LDS tile with a 2-pixel halo, blur from the
//                tile, fp32 intermediate [views][n][h][w][4]
//   output pass  affine gather (4 bilinear taps, x 9 for the 3x3 stage) from that intermediate -- or straight from the uint8
//                frame through the D4 code when the sample has neither noise nor blur -- then the point-wise stages and the store.
// A record with every stage off therefore costs one pass and computes exactly udaseg_prepare_batch_u8's arithmetic.
// Stage selection is per sample (blockIdx.y) and per view (blockIdx.z): every branch on the record is uniform over the block.
// udaseg_strong_aug_clahe_u8 is the same call for batches with a record on CLAHE (stage-5 kind 3): the table pass (clahe.hip)
// runs between the two, and the output pass is the variant with that one more stage-5 branch.
#include "aug_common.h"

namespace udaseg {

__global__ __launch_bounds__(256) void strong_source_kernel(const uint8_t* __restrict__ images, const int32_t* __restrict__ table,
                                                            int n, int h, int w, f32x4* __restrict__ mid) {
  const int ni = blockIdx.y, view = blockIdx.z;
  const SaRec rec = sa_load(table + ((size_t)view * n + ni) * SA_WORDS);
  if (!(rec.flags & (SA_NOISE | SA_BLUR))) return;            // block-uniform: the output pass reads the frame itself
  sa_source_pass(images, rec, ni, (size_t)view * n + ni, h, w, mid);
}

// the output pass.  CLAHE = false is the kernel of udaseg_strong_aug_u8 (lut is not read); CLAHE = true adds stage-5 kind 3 (the
// slot's table from the table pass, clahe.hip) and leaves every other branch as it is written here.
template <bool BF16, bool CLAHE>
__global__ __launch_bounds__(256) void strong_output_kernel(const uint8_t* __restrict__ images, const int32_t* __restrict__ table,
                                                            const f32x4* __restrict__ mid, int n, int h, int w, float m0, float m1,
                                                            float m2, float r0, float r1, float r2, void* __restrict__ out, int cpad,
                                                            const uint8_t* __restrict__ lut) {
  const int ni = blockIdx.y, view = blockIdx.z;
  const SaRec rec = sa_load(table + ((size_t)view * n + ni) * SA_WORDS);
  const int hw = h * w;
  SaSrc src;
  src.img = images + (size_t)ni * hw * 3;
  src.mid = (rec.flags & (SA_NOISE | SA_BLUR)) ? mid + ((size_t)view * n + ni) * hw : nullptr;
  src.d4 = sa_code(rec.d4, h, w); src.h = h; src.w = w;
  float k3[9];                                                   // the 3x3 stage's kernel (correlation, row-major)
  if ((rec.flags & SA_STAGE5) && rec.s5_kind < 2) {
    const float a = rec.p5a, p = rec.p5b;
    if (rec.s5_kind == 0) {                                      // sharpen: (1-a) I + a [[-1,-1,-1],[-1,8+l,-1],[-1,-1,-1]]
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
    if ((rec.flags & SA_STAGE5) && rec.s5_kind < 2) {
      float acc[3] = {0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const int yy = reflect101(y + i - 1, h);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          float t[3];
          sa_stage4(src, rec, yy, reflect101(x + j - 1, w), t);
#pragma unroll
          for (int c = 0; c < 3; ++c) acc[c] += k3[i * 3 + j] * t[c];
        }
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c] = clamp255(acc[c]);
    } else if (CLAHE && (rec.flags & SA_STAGE5) && rec.s5_kind == SA_CLAHE) {
      sa_stage4(src, rec, y, x, v);
      cl_apply(v, lut + ((size_t)view * n + ni) * (CL_TILES * CL_BINS), y, x, h / CL_GRID, w / CL_GRID);
    } else {
      sa_stage4(src, rec, y, x, v);
      if (rec.flags & SA_STAGE5) {                               // brightness-contrast: v (1 + c) + 255 b
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = clamp255(v[c] * (1.f + rec.p5b) + 255.f * rec.p5a);
      }
    }
    if (rec.flags & SA_HSV) sa_hsv_shift(v, rec.dh, rec.ds, rec.dv);
    const float v0 = (v[0] - m0) * r0, v1 = (v[1] - m1) * r1, v2 = (v[2] - m2) * r2;
    const size_t o = (((size_t)view * n + ni) * hw + pix) * cpad;
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

// every pass of a call; lut == nullptr: today's launches, else the table pass goes between the source and the output pass
static int strong_aug_run(const char* who, const uint8_t* images, const int32_t* table, int views, int n, int h, int w, float* mid,
                          const float* mean255, const float* inv_std255, void* out_images, int cpad, int out_bf16, int source_pass,
                          uint8_t* lut, bool clahe, void* stream) {
  UDASEG_CHECK_ARG(images && table && out_images && mean255 && inv_std255 && n > 0 && h > 0 && w > 0, "%s: bad arguments", who);
  UDASEG_CHECK_ARG(views == 1 || views == 2, "%s: views must be 1 or 2", who);
  UDASEG_CHECK_ARG(cpad >= 4 && cpad % (out_bf16 ? 8 : 4) == 0, "%s: cpad must be a multiple of %d", who, out_bf16 ? 8 : 4);
  UDASEG_CHECK_ARG((int64_t)h * w < (1LL << 30) && n <= 65535, "%s: batch too large", who);
  UDASEG_CHECK_ARG(!source_pass || mid, "%s: the source pass needs the intermediate buffer", who);
  UDASEG_CHECK_ARG(((uintptr_t)mid & 15) == 0 && ((uintptr_t)out_images & 15) == 0, "%s: buffers must be 16-byte aligned", who);
  UDASEG_CHECK_ARG(!clahe || lut, "%s: the table pass needs the table buffer", who);
  UDASEG_CHECK_ARG(!clahe || (h % CL_GRID == 0 && w % CL_GRID == 0), "%s: the frame sides must be multiples of %d", who, CL_GRID);
  hipStream_t st = as_stream(stream);
  if (source_pass) {
    const int tiles = cdiv(h, SA_TILE) * cdiv(w, SA_TILE);
    hipLaunchKernelGGL(strong_source_kernel, dim3(tiles, n, views), dim3(256), 0, st, images, table, n, h, w, (f32x4*)mid);
    UDASEG_LAUNCH_CHECK("strong_aug source pass launch");
  }
  if (clahe) {
    clahe_launch_lut(images, table, SA_WORDS, views, n, h, w, source_pass ? mid : nullptr, nullptr, lut, st);
    UDASEG_LAUNCH_CHECK("strong_aug table pass launch");
  }
  const int gx = (h * w + 255) / 256 > 1024 ? 1024 : (h * w + 255) / 256;
  const float m0 = mean255[0], m1 = mean255[1], m2 = mean255[2], r0 = inv_std255[0], r1 = inv_std255[1], r2 = inv_std255[2];
  const uint8_t* tab = lut;
#define UDASEG_SA_OUTPUT(BF16, CLAHE)                                                                                                \
  hipLaunchKernelGGL((strong_output_kernel<BF16, CLAHE>), dim3(gx, n, views), dim3(256), 0, st, images, table, (const f32x4*)mid, n, \
                     h, w, m0, m1, m2, r0, r1, r2, out_images, cpad, tab)
  if (clahe) {
    if (out_bf16) UDASEG_SA_OUTPUT(true, true);
    else UDASEG_SA_OUTPUT(false, true);
  } else {
    if (out_bf16) UDASEG_SA_OUTPUT(true, false);
    else UDASEG_SA_OUTPUT(false, false);
  }
#undef UDASEG_SA_OUTPUT
  UDASEG_LAUNCH_CHECK("strong_aug output pass launch");
  return UDASEG_OK;
}

extern "C" int udaseg_strong_aug_u8(const uint8_t* images, const int32_t* table, int views, int n, int h, int w, float* mid,
                                    const float* mean255, const float* inv_std255, void* out_images, int cpad, int out_bf16,
                                    int source_pass, void* stream) {
  return strong_aug_run("strong_aug_u8", images, table, views, n, h, w, mid, mean255, inv_std255, out_images, cpad, out_bf16,
                        source_pass, nullptr, false, stream);
}

extern "C" int udaseg_strong_aug_clahe_u8(const uint8_t* images, const int32_t* table, int views, int n, int h, int w, float* mid,
                                          const float* mean255, const float* inv_std255, void* out_images, int cpad, int out_bf16,
                                          int source_pass, uint8_t* lut, void* stream) {
  return strong_aug_run("strong_aug_clahe_u8", images, table, views, n, h, w, mid, mean255, inv_std255, out_images, cpad, out_bf16,
                        source_pass, lut, true, stream);
}

extern "C" int udaseg_philox4x32_debug(const int32_t* counters, const int32_t* keys, int32_t* out, int count, void* stream) {
  UDASEG_CHECK_ARG(counters && keys && out && count > 0, "philox4x32_debug: bad arguments");
  hipLaunchKernelGGL(philox_debug_kernel, dim3(cdiv(count, 64)), dim3(64), 0, as_stream(stream), counters, keys, out, count);
  UDASEG_LAUNCH_CHECK("philox4x32_debug launch");
  return UDASEG_OK;
}
