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
#include "common.h"

namespace udaseg {

constexpr int SA_WORDS = 32;            // 4-byte words per record (include/udaseg.h: UDASEG_STRONG_AUG_WORDS)
constexpr int SA_NOISE = 1, SA_BLUR = 2, SA_AFFINE = 4, SA_STAGE5 = 8, SA_HSV = 16;
constexpr int SA_TILE = 16, SA_HALO = 2, SA_SIDE = SA_TILE + 2 * SA_HALO, SA_LD = SA_SIDE + 1;

struct SaRec {
  int flags, d4, blur_kind, blur_k, motion_dir, s5_kind;
  uint32_t key0, key1;
  float sigma, m[6], p5a, p5b, dh, ds, dv;
};

__device__ __forceinline__ SaRec sa_load(const int32_t* __restrict__ t) {
  SaRec r;
  r.flags = t[0]; r.d4 = t[1]; r.blur_kind = t[2]; r.blur_k = t[3]; r.motion_dir = t[4]; r.s5_kind = t[5];
  r.key0 = (uint32_t)t[6]; r.key1 = (uint32_t)t[7];
  r.sigma = __int_as_float(t[8]);
#pragma unroll
  for (int i = 0; i < 6; ++i) r.m[i] = __int_as_float(t[9 + i]);
  r.p5a = __int_as_float(t[15]); r.p5b = __int_as_float(t[16]);
  r.dh = __int_as_float(t[17]); r.ds = __int_as_float(t[18]); r.dv = __int_as_float(t[19]);
  return r;
}

// reflect-101 (cv2.BORDER_REFLECT_101, numpy "reflect"): period 2(L-1), any distance; L == 1 reads index 0
__device__ __forceinline__ int reflect101(int i, int L) {
  if (L == 1) return 0;
  const int p = 2 * (L - 1);
  i %= p;
  if (i < 0) i += p;
  return i < L ? i : p - i;
}

__device__ __forceinline__ float clamp255(float v) { return fminf(fmaxf(v, 0.f), 255.f); }

// Philox4x32-10 (Salmon et al., SC'11; Random123)
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t (&out)[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

__device__ __forceinline__ float sa_uniform(uint32_t r) { return ((float)(r >> 8) + 0.5f) * 5.9604644775390625e-08f; }  // 2^-24

// three standard normals of pixel `counter` (Box-Muller on the four words; accurate logf / sincosf)
__device__ __forceinline__ void sa_normals(uint32_t counter, uint32_t k0, uint32_t k1, float (&z)[3]) {
  uint32_t r[4];
  philox4x32_10(counter, 0u, 0u, 0u, k0, k1, r);
  const float two_pi = 6.283185307179586f;
  const float a0 = sqrtf(-2.f * logf(sa_uniform(r[0]))), a1 = sqrtf(-2.f * logf(sa_uniform(r[2])));
  float s0, c0, s1, c1;
  sincosf(two_pi * sa_uniform(r[1]), &s0, &c0);
  sincosf(two_pi * sa_uniform(r[3]), &s1, &c1);
  z[0] = a0 * c0; z[1] = a0 * s0; z[2] = a1 * c1;
}

// a transposing code on a non-square frame would read past the frame: the binding refuses it, the kernels drop the bit
__device__ __forceinline__ int sa_code(int d4, int h, int w) { return h == w ? (d4 & 7) : (d4 & 6); }

// source pixel of D4-output pixel (y, x): prepare_batch_kernel's gather
__device__ __forceinline__ int d4_source(int code, int y, int x, int h, int w) {
  if (code & 2) y = h - 1 - y;
  if (code & 4) x = w - 1 - x;
  return (code & 1) ? x * w + y : y * w + x;
}

template <int K>
__device__ __forceinline__ float sa_median(const float* __restrict__ t) {   // t: tile row-major with leading dimension SA_LD, at the window's corner
  float v[K * K];
#pragma unroll
  for (int i = 0; i < K; ++i)
#pragma unroll
    for (int j = 0; j < K; ++j) v[i * K + j] = t[i * SA_LD + j];
  float med = v[0];
#pragma unroll
  for (int i = 0; i < K * K; ++i) {        // rank by counting (ties broken by position): the element of rank K*K/2
    int rank = 0;
#pragma unroll
    for (int j = 0; j < K * K; ++j) rank += (v[j] < v[i] || (v[j] == v[i] && j < i)) ? 1 : 0;
    if (rank == K * K / 2) med = v[i];
  }
  return med;
}

__global__ __launch_bounds__(256) void strong_source_kernel(const uint8_t* __restrict__ images, const int32_t* __restrict__ table,
                                                            int n, int h, int w, f32x4* __restrict__ mid) {
  __shared__ float tile[3][SA_SIDE * SA_LD];
  const int ni = blockIdx.y, view = blockIdx.z;
  const SaRec rec = sa_load(table + ((size_t)view * n + ni) * SA_WORDS);
  if (!(rec.flags & (SA_NOISE | SA_BLUR))) return;            // block-uniform: the output pass reads the frame itself
  const int tiles_x = (w + SA_TILE - 1) / SA_TILE;
  const int ty0 = (blockIdx.x / tiles_x) * SA_TILE, tx0 = (blockIdx.x % tiles_x) * SA_TILE;
  const uint8_t* img = images + (size_t)ni * h * w * 3;
  const int code = sa_code(rec.d4, h, w);
  for (int i = threadIdx.x; i < SA_SIDE * SA_SIDE; i += 256) {
    const int ly = i / SA_SIDE, lx = i - ly * SA_SIDE;
    const int y = reflect101(ty0 - SA_HALO + ly, h), x = reflect101(tx0 - SA_HALO + lx, w);
    const int sp = d4_source(code, y, x, h, w);
    float v0 = (float)img[sp * 3 + 0], v1 = (float)img[sp * 3 + 1], v2 = (float)img[sp * 3 + 2];
    if (rec.flags & SA_NOISE) {
      float z[3];
      sa_normals((uint32_t)(y * w + x), rec.key0, rec.key1, z);
      v0 = clamp255(v0 + rec.sigma * z[0]);
      v1 = clamp255(v1 + rec.sigma * z[1]);
      v2 = clamp255(v2 + rec.sigma * z[2]);
    }
    tile[0][ly * SA_LD + lx] = v0;
    tile[1][ly * SA_LD + lx] = v1;
    tile[2][ly * SA_LD + lx] = v2;
  }
  __syncthreads();
  const int ly = threadIdx.x >> 4, lx = threadIdx.x & 15;
  const int y = ty0 + ly, x = tx0 + lx;
  if (y >= h || x >= w) return;
  const int cy = ly + SA_HALO, cx = lx + SA_HALO;
  float o[3];
  if (!(rec.flags & SA_BLUR)) {
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = tile[c][cy * SA_LD + cx];
  } else {
    const int k = rec.blur_k == 5 ? 5 : 3, r = k >> 1;        // k in {3, 5}: the window stays inside the tile's halo
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float* t = tile[c];
      if (rec.blur_kind == 0) {                               // box: mean of k x k
        float s = 0.f;
        for (int i = -r; i <= r; ++i)
          for (int j = -r; j <= r; ++j) s += t[(cy + i) * SA_LD + cx + j];
        o[c] = s / (float)(k * k);
      } else if (rec.blur_kind == 1) {                        // per-channel median of k x k
        const float* corner = t + (cy - r) * SA_LD + (cx - r);
        o[c] = (k == 3) ? sa_median<3>(corner) : sa_median<5>(corner);
      } else {                                                // motion: mean of the k taps on a line through the centre
        const int dy = (rec.motion_dir == 0) ? 0 : 1;
        const int dx = (rec.motion_dir == 1) ? 0 : (rec.motion_dir == 3 ? -1 : 1);
        float s = 0.f;
        for (int i = -r; i <= r; ++i) s += t[(cy + i * dy) * SA_LD + cx + i * dx];
        o[c] = s / (float)k;
      }
    }
  }
  mid[(((size_t)view * n + ni) * h + y) * w + x] = f32x4{o[0], o[1], o[2], 0.f};
}

struct SaSrc {
  const uint8_t* img;      // the sample's frame
  const f32x4* mid;        // the sample's / view's intermediate, or nullptr: read the frame through the D4 code
  int d4, h, w;
};

__device__ __forceinline__ void sa_fetch(const SaSrc& s, int y, int x, float (&v)[3]) {   // (y, x) inside the frame
  if (s.mid) {
    const f32x4 t = s.mid[y * s.w + x];
    v[0] = t[0]; v[1] = t[1]; v[2] = t[2];
  } else {
    const int sp = d4_source(s.d4, y, x, s.h, s.w);
    v[0] = (float)s.img[sp * 3 + 0]; v[1] = (float)s.img[sp * 3 + 1]; v[2] = (float)s.img[sp * 3 + 2];
  }
}

// the image after stage 4 at output-grid pixel (y, x) (inside the frame)
__device__ __forceinline__ void sa_stage4(const SaSrc& s, const SaRec& rec, int y, int x, float (&v)[3]) {
  if (!(rec.flags & SA_AFFINE)) {
    sa_fetch(s, y, x, v);
    return;
  }
  const float fx = (float)x, fy = (float)y;
  const float sx = rec.m[0] * fx + rec.m[1] * fy + rec.m[2];
  const float sy = rec.m[3] * fx + rec.m[4] * fy + rec.m[5];
  const float x0f = floorf(sx), y0f = floorf(sy);
  const float ax = sx - x0f, ay = sy - y0f;
  const int x0 = reflect101((int)x0f, s.w), x1 = reflect101((int)x0f + 1, s.w);
  const int y0 = reflect101((int)y0f, s.h), y1 = reflect101((int)y0f + 1, s.h);
  float a[3], b[3], c[3], d[3];
  sa_fetch(s, y0, x0, a);
  sa_fetch(s, y0, x1, b);
  sa_fetch(s, y1, x0, c);
  sa_fetch(s, y1, x1, d);
#pragma unroll
  for (int k = 0; k < 3; ++k)
    v[k] = (1.f - ay) * ((1.f - ax) * a[k] + ax * b[k]) + ay * ((1.f - ax) * c[k] + ax * d[k]);
}

__device__ __forceinline__ void sa_hsv_shift(float (&v)[3], float dh, float ds, float dv) {
  const float r = v[0], g = v[1], b = v[2];
  const float mx = fmaxf(r, fmaxf(g, b)), mn = fminf(r, fminf(g, b));
  const float delta = mx - mn;
  float hh = 0.f;                                               // OpenCV's 8-bit scales: h in [0,180), s and v in [0,255]
  if (delta > 0.f) {
    if (mx == r) hh = 30.f * (g - b) / delta;
    else if (mx == g) hh = 60.f + 30.f * (b - r) / delta;
    else hh = 120.f + 30.f * (r - g) / delta;
  }
  float ss = mx > 0.f ? 255.f * delta / mx : 0.f;
  hh += dh;
  hh -= 180.f * floorf(hh / 180.f);
  ss = clamp255(ss + ds);
  const float vv = clamp255(mx + dv);
  const float h6 = hh / 30.f;
  const float fl = floorf(h6);
  const float f = h6 - fl;
  const int sector = ((int)fl) % 6;
  const float s1 = ss / 255.f;
  const float p = vv * (1.f - s1), q = vv * (1.f - s1 * f), t = vv * (1.f - s1 * (1.f - f));
  float ro, go, bo;
  switch (sector) {
    case 0: ro = vv; go = t; bo = p; break;
    case 1: ro = q; go = vv; bo = p; break;
    case 2: ro = p; go = vv; bo = t; break;
    case 3: ro = p; go = q; bo = vv; break;
    case 4: ro = t; go = p; bo = vv; break;
    default: ro = vv; go = p; bo = q; break;
  }
  v[0] = clamp255(ro); v[1] = clamp255(go); v[2] = clamp255(bo);
}

template <bool BF16>
__global__ __launch_bounds__(256) void strong_output_kernel(const uint8_t* __restrict__ images, const int32_t* __restrict__ table,
                                                            const f32x4* __restrict__ mid, int n, int h, int w, float m0, float m1,
                                                            float m2, float r0, float r1, float r2, void* __restrict__ out, int cpad) {
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

extern "C" int udaseg_strong_aug_u8(const uint8_t* images, const int32_t* table, int views, int n, int h, int w, float* mid,
                                    const float* mean255, const float* inv_std255, void* out_images, int cpad, int out_bf16,
                                    int source_pass, void* stream) {
  UDASEG_CHECK_ARG(images && table && out_images && mean255 && inv_std255 && n > 0 && h > 0 && w > 0, "strong_aug_u8: bad arguments");
  UDASEG_CHECK_ARG(views == 1 || views == 2, "strong_aug_u8: views must be 1 or 2");
  UDASEG_CHECK_ARG(cpad >= 4 && cpad % (out_bf16 ? 8 : 4) == 0, "strong_aug_u8: cpad must be a multiple of %d", out_bf16 ? 8 : 4);
  UDASEG_CHECK_ARG((int64_t)h * w < (1LL << 30) && n <= 65535, "strong_aug_u8: batch too large");
  UDASEG_CHECK_ARG(!source_pass || mid, "strong_aug_u8: the source pass needs the intermediate buffer");
  UDASEG_CHECK_ARG(((uintptr_t)mid & 15) == 0 && ((uintptr_t)out_images & 15) == 0, "strong_aug_u8: buffers must be 16-byte aligned");
  hipStream_t st = as_stream(stream);
  if (source_pass) {
    const int tiles = cdiv(h, SA_TILE) * cdiv(w, SA_TILE);
    hipLaunchKernelGGL(strong_source_kernel, dim3(tiles, n, views), dim3(256), 0, st, images, table, n, h, w, (f32x4*)mid);
    UDASEG_LAUNCH_CHECK("strong_aug source pass launch");
  }
  const int gx = (h * w + 255) / 256 > 1024 ? 1024 : (h * w + 255) / 256;
  if (out_bf16)
    hipLaunchKernelGGL(strong_output_kernel<true>, dim3(gx, n, views), dim3(256), 0, st, images, table, (const f32x4*)mid, n, h, w,
                       mean255[0], mean255[1], mean255[2], inv_std255[0], inv_std255[1], inv_std255[2], out_images, cpad);
  else
    hipLaunchKernelGGL(strong_output_kernel<false>, dim3(gx, n, views), dim3(256), 0, st, images, table, (const f32x4*)mid, n, h, w,
                       mean255[0], mean255[1], mean255[2], inv_std255[0], inv_std255[1], inv_std255[2], out_images, cpad);
  UDASEG_LAUNCH_CHECK("strong_aug output pass launch");
  return UDASEG_OK;
}

extern "C" int udaseg_philox4x32_debug(const int32_t* counters, const int32_t* keys, int32_t* out, int count, void* stream) {
  UDASEG_CHECK_ARG(counters && keys && out && count > 0, "philox4x32_debug: bad arguments");
  hipLaunchKernelGGL(philox_debug_kernel, dim3(cdiv(count, 64)), dim3(64), 0, as_stream(stream), counters, keys, out, count);
  UDASEG_LAUNCH_CHECK("philox4x32_debug launch");
  return UDASEG_OK;
}
