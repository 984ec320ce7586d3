// Device-side input pipeline: what the reference does per sample on the host between the decoded
// uint8 image and the model input --
//   src/data/dataset.py:116-138      uint8 RGB HWC image + uint8 label mask -> (float image, int64 mask)
//   src/models/augmentation.py:11-13 RandomRotate90 / Flip / Transpose: together an element of the dihedral group D4,
//                                    applied identically to image and mask
//   src/models/augmentation.py:36    A.Normalize(): (x - 255*mean) * (1 / (255*std)), fp32, ImageNet mean/std
// -- as ONE pass that writes the padded NHWC tensor the stem convolution reads (fp32 or bf16) and the int64 mask.
// HBM-bound byte shuffling: 4 B/pixel read, 4*cpad (or 2*cpad) + 8 B/pixel written.
#include "common.h"

namespace udaseg {

// D4 code: bit0 = transpose, bit1 = vertical flip (rows), bit2 = horizontal flip (columns), applied in that order:
//   out = fliph^b2( flipv^b1( transpose^b0( in ) ) )
template <bool BF16>
__global__ __launch_bounds__(256) void prepare_batch_kernel(const uint8_t* __restrict__ images, const uint8_t* __restrict__ masks,
                                                            const int32_t* __restrict__ d4, int h, int w, Normalize3 nm,
                                                            void* __restrict__ out, int cpad, int64_t* __restrict__ out_masks) {
  const int ni = blockIdx.y;
  const int code = d4 ? d4[ni] : 0;
  const int hw = h * w;
  const uint8_t* img = images + (size_t)ni * hw * 3;
  const uint8_t* msk = masks ? masks + (size_t)ni * hw : nullptr;
  for (int p = blockIdx.x * 256 + threadIdx.x; p < hw; p += gridDim.x * 256) {
    int y = p / w, x = p - y * w;
    if (code & 2) y = h - 1 - y;
    if (code & 4) x = w - 1 - x;
    const int sp = (code & 1) ? x * w + y : y * w + x;        // transpose needs h == w (checked by the caller)
    const uint8_t* px = img + (size_t)sp * 3;                 // sp * 3 passes 2^31 from 715 827 883 pixels on
    store_normalized<BF16>(out, ((size_t)ni * hw + p) * cpad, cpad, nm, (float)px[0], (float)px[1], (float)px[2]);
    if (msk) out_masks[(size_t)ni * hw + p] = (int64_t)msk[sp];
  }
}

}  // namespace udaseg

using namespace udaseg;

extern "C" int udaseg_prepare_batch_u8(const uint8_t* images, const uint8_t* masks, const int32_t* d4, int n, int h, int w,
                                       const float* mean255, const float* inv_std255, void* out_images, int cpad, int out_bf16,
                                       int64_t* out_masks, int square_checked, void* stream) {
  UDASEG_CHECK_ARG(images && out_images && mean255 && inv_std255 && n > 0 && h > 0 && w > 0, "prepare_batch_u8: bad arguments");
  UDASEG_CHECK_ARG(cpad >= 4 && cpad % (out_bf16 ? 8 : 4) == 0, "prepare_batch_u8: cpad must be a multiple of %d",
                   out_bf16 ? 8 : 4);
  UDASEG_CHECK_ARG((masks == nullptr) == (out_masks == nullptr), "prepare_batch_u8: masks and out_masks go together");
  UDASEG_CHECK_ARG(d4 == nullptr || h == w || square_checked, "prepare_batch_u8: transposing codes need square images; pass "
                   "square_checked=1 after making sure no code has bit 0 set");
  UDASEG_CHECK_ARG((int64_t)h * w < (1LL << 30), "prepare_batch_u8: image too large");
  const int gx = (h * w + 255) / 256 > 1024 ? 1024 : (h * w + 255) / 256;
  hipStream_t st = as_stream(stream);
  const Normalize3 nm = normalize3(mean255, inv_std255);
  if (out_bf16)
    hipLaunchKernelGGL(prepare_batch_kernel<true>, dim3(gx, n), dim3(256), 0, st, images, masks, d4, h, w, nm, out_images, cpad, out_masks);
  else
    hipLaunchKernelGGL(prepare_batch_kernel<false>, dim3(gx, n), dim3(256), 0, st, images, masks, d4, h, w, nm, out_images, cpad, out_masks);
  UDASEG_LAUNCH_CHECK("prepare_batch launch");
  return UDASEG_OK;
}
