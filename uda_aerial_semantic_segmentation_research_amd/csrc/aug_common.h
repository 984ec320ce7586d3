// Device helpers shared by the augmentation sources (augment.hip: the source and output pass of both pipelines, phase-3 views
// and labelled training batches; elastic_field.hip: the elastic field pass; clahe.hip: the CLAHE table pass): the record layout
// and loader, reflect-101, Philox4x32-10, the D4 gather, the k x k median, the stage-3 source pass, the frame / intermediate
// fetch, stage 4 (the affine gather), the 3 x 3 stage's kernel, the HSV shift, the training record with stages 4 + 4b (the
// composed gather), the per-block set-up of the passes that evaluate stage 4, and CLAHE's colour round trip and per-pixel
// table blend.  One definition each: both pipelines are held to the same arithmetic bit for bit.
#pragma once
#include "common.h"

namespace udaseg {

constexpr int SA_WORDS = 32;            // 4-byte words per record (include/udaseg.h: UDASEG_STRONG_AUG_WORDS)
constexpr int SA_NOISE = 1, SA_BLUR = 2, SA_AFFINE = 4, SA_STAGE5 = 8, SA_HSV = 16;
// word indices of the record (data.py keeps the same list as _W_*)
constexpr int SA_W_FLAGS = 0, SA_W_D4 = 1, SA_W_BLUR_KIND = 2, SA_W_BLUR_K = 3, SA_W_MOTION_DIR = 4, SA_W_S5_KIND = 5, SA_W_KEY = 6,
              SA_W_SIGMA = 8, SA_W_AFFINE = 9, SA_W_S5_PARAMS = 15, SA_W_HSV = 17;
constexpr int SA_TILE = 16, SA_HALO = 2, SA_SIDE = SA_TILE + 2 * SA_HALO, SA_LD = SA_SIDE + 1;

struct SaRec {
  int flags, d4, blur_kind, blur_k, motion_dir, s5_kind;
  uint32_t key0, key1;
  float sigma, m[6], p5a, p5b, dh, ds, dv;
};

__device__ __forceinline__ SaRec sa_load(const int32_t* __restrict__ t) {
  SaRec r;
  r.flags = t[SA_W_FLAGS]; r.d4 = t[SA_W_D4]; r.blur_kind = t[SA_W_BLUR_KIND]; r.blur_k = t[SA_W_BLUR_K];
  r.motion_dir = t[SA_W_MOTION_DIR]; r.s5_kind = t[SA_W_S5_KIND];
  r.key0 = (uint32_t)t[SA_W_KEY]; r.key1 = (uint32_t)t[SA_W_KEY + 1];
  r.sigma = __int_as_float(t[SA_W_SIGMA]);
#pragma unroll
  for (int i = 0; i < 6; ++i) r.m[i] = __int_as_float(t[SA_W_AFFINE + i]);
  r.p5a = __int_as_float(t[SA_W_S5_PARAMS]); r.p5b = __int_as_float(t[SA_W_S5_PARAMS + 1]);
  r.dh = __int_as_float(t[SA_W_HSV]); r.ds = __int_as_float(t[SA_W_HSV + 1]); r.dv = __int_as_float(t[SA_W_HSV + 2]);
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

// stage 1-3 of one sample (block = one 16 x 16 tile): D4 gather + noise into an LDS tile with a 2-pixel halo, blur from the tile,
// fp32 intermediate mid[slot][h][w][4].  Callers return before it when the record has neither noise nor blur.
__device__ __forceinline__ void sa_source_pass(const uint8_t* __restrict__ images, const SaRec& rec, int ni, size_t slot, int h, int w,
                                               f32x4* __restrict__ mid) {
  __shared__ float tile[3][SA_SIDE * SA_LD];
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
  mid[(slot * h + y) * w + x] = f32x4{o[0], o[1], o[2], 0.f};
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

// stage 5, kinds 0 and 1: the 3 x 3 stage's kernel (correlation, row-major)
__device__ __forceinline__ void sa_kernel3(const SaRec& rec, float (&k3)[9]) {
  const float a = rec.p5a, p = rec.p5b;
  if (rec.s5_kind == 0) {                                        // sharpen: (1-a) I + a [[-1,-1,-1],[-1,8+l,-1],[-1,-1,-1]]
#pragma unroll
    for (int i = 0; i < 9; ++i) k3[i] = -a;
    k3[4] = (1.f - a) + a * (8.f + p);
  } else {                                                       // emboss: (1-a) I + a [[-1-s,-s,0],[-s,1,s],[0,s,1+s]]
    k3[0] = a * (-1.f - p); k3[1] = a * -p; k3[2] = 0.f;
    k3[3] = a * -p; k3[4] = (1.f - a) + a; k3[5] = a * p;
    k3[6] = 0.f; k3[7] = a * p; k3[8] = a * (1.f + p);
  }
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

// ---------------------------------------------------------------------------------- the training record and stages 4 + 4b
constexpr int TA_WORDS = 64;            // 4-byte words per record (include/udaseg.h: UDASEG_TRAIN_AUG_WORDS); 0..31: the strong record
constexpr int TA_DISTORT = 32;          // flag bit of word 0
constexpr int TA_W_DISTORT_KIND = 32, TA_W_OPTICAL = 33, TA_W_GRID = 36, TA_W_ELASTIC_ALPHA = 48, TA_W_ELASTIC_KEY = 50;
constexpr int TA_OPTICAL = 1, TA_GRID = 2, TA_ELASTIC = 3;
constexpr int TA_MAX_RADIUS = 18;       // include/udaseg.h: UDASEG_ELASTIC_MAX_RADIUS
constexpr int TA_FT = 32;               // the field kernel's tile side
constexpr int TA_FS = TA_FT + 2 * TA_MAX_RADIUS;

typedef float ta_f2 __attribute__((ext_vector_type(2)));

struct TaWeights { float w[2 * TA_MAX_RADIUS + 1]; };

struct TaRec {
  SaRec s;
  int kind;                             // 0: no distortion
  float ok, odx, ody;                   // optical
  float alpha;                          // elastic (the grid's step factors go to LDS: ta_grid_table)
};

__device__ __forceinline__ TaRec ta_load(const int32_t* __restrict__ t) {
  TaRec r;
  r.s = sa_load(t);
  r.kind = (r.s.flags & TA_DISTORT) ? t[TA_W_DISTORT_KIND] : 0;
  r.ok = __int_as_float(t[TA_W_OPTICAL]); r.odx = __int_as_float(t[TA_W_OPTICAL + 1]); r.ody = __int_as_float(t[TA_W_OPTICAL + 2]);
  r.alpha = __int_as_float(t[TA_W_ELASTIC_ALPHA]);
  return r;
}

struct TaGeo {                          // what the block needs of the record's geometry, formed once
  int kind, affine, cw, ch;
  float cx, cy;                         // optical centre
  const float* grid;                    // LDS: x starts [6], x steps [6], y starts [6], y steps [6]
  const ta_f2* field;                   // the sample's field, or nullptr
};

// grid distortion: cell i of an axis starts at s_i on the source grid, s_0 = 0, s_{i+1} = s_i + cell * step_i (summed in this
// order); threads 0..11 form one entry each of the block's table
__device__ __forceinline__ void ta_grid_table(const int32_t* __restrict__ t, int cw, int ch, float* tab) {
  if (threadIdx.x < 12) {
    const int axis = threadIdx.x / 6, cell = threadIdx.x - axis * 6;
    const int32_t* steps = t + TA_W_GRID + 6 * axis;
    const float side = (float)(axis ? ch : cw);
    float s = 0.f;
    for (int i = 0; i < cell; ++i) s = s + side * __int_as_float(steps[i]);
    tab[12 * axis + cell] = s;
    tab[12 * axis + 6 + cell] = __int_as_float(steps[cell]);
  }
  __syncthreads();
}

__device__ __forceinline__ TaGeo ta_geometry(const TaRec& rec, const ta_f2* field, const float* grid, int h, int w) {
  TaGeo g;
  g.kind = rec.kind;
  g.affine = (rec.s.flags & SA_AFFINE) ? 1 : 0;
  g.field = field;
  g.grid = grid;
  g.cw = w / 5 > 0 ? w / 5 : 1;
  g.ch = h / 5 > 0 ? h / 5 : 1;
  g.cx = (float)(w - 1) * 0.5f + rec.odx;
  g.cy = (float)(h - 1) * 0.5f + rec.ody;
  if (g.kind == TA_ELASTIC && !field) g.kind = 0;               // the binding refuses such a call; never dereference a missing field
  return g;
}

__device__ __forceinline__ float ta_grid_axis(int x, int cw, const float* tab) {
  int i = x / cw;
  i = i < 5 ? i : 5;                                            // the last cell takes what remains of the axis
  return tab[i] + (float)(x - i * cw) * tab[6 + i];
}

// source position r of output pixel (y, x) (inside the frame): r = M (q(p), 1)
__device__ __forceinline__ void ta_position(const TaGeo& g, const TaRec& rec, int y, int x, int h, int w, float& rx, float& ry) {
  const float fx = (float)x, fy = (float)y;
  if (!g.kind) {                                                // shift-scale-rotate alone: sa_stage4's own expression
    rx = rec.s.m[0] * fx + rec.s.m[1] * fy + rec.s.m[2];
    ry = rec.s.m[3] * fx + rec.s.m[4] * fy + rec.s.m[5];
    return;
  }
  float qx = fx, qy = fy;
  if (g.kind == TA_OPTICAL) {
    const float ex = fx - g.cx, ey = fy - g.cy;
    const float u = ex / (float)w, v = ey / (float)h;
    const float r2 = u * u + v * v;
    const float f = 1.f + rec.ok * r2 + rec.ok * r2 * r2;
    qx = g.cx + ex * f;
    qy = g.cy + ey * f;
  } else if (g.kind == TA_GRID) {
    qx = ta_grid_axis(x, g.cw, g.grid);
    qy = ta_grid_axis(y, g.ch, g.grid + 12);
  } else if (g.kind == TA_ELASTIC) {
    const ta_f2 d = g.field[y * w + x];
    qx = fx + rec.alpha * d.x;
    qy = fy + rec.alpha * d.y;
  }
  if (g.affine) {
    rx = rec.s.m[0] * qx + rec.s.m[1] * qy + rec.s.m[2];
    ry = rec.s.m[3] * qx + rec.s.m[4] * qy + rec.s.m[5];
  } else {
    rx = qx;
    ry = qy;
  }
}

// the image after stages 4 and 4b at output-grid pixel (y, x) (inside the frame): one bilinear sample at r
// (the interpolation is written out as in sa_stage4, which stays as it is: its compiled arithmetic is what strong_views is pinned to)
__device__ __forceinline__ void ta_stage4(const SaSrc& s, const TaGeo& g, const TaRec& rec, int y, int x, float (&v)[3]) {
  if (!g.kind) {                                                // no distortion: the strong pipeline's stage 4, bit for bit
    sa_stage4(s, rec.s, y, x, v);
    return;
  }
  float sx, sy;
  ta_position(g, rec, y, x, s.h, s.w, sx, sy);
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

// What a block of a pass that evaluates stage 4 (the output pass, augment.hip; the table pass, clahe.hip) forms once from its
// record t: the record, the source and, for the training record, the geometry with the grid table in LDS (grid_tab: 24 floats;
// not touched with TRAIN == false, where the distortion kind is 0 and geo stays unset).  slot = view * n + ni.
struct AugBlock {
  TaRec rec;
  SaSrc src;
  TaGeo geo;
};

template <bool TRAIN>
__device__ __forceinline__ AugBlock aug_block(const int32_t* __restrict__ t, const uint8_t* __restrict__ images,
                                              const f32x4* __restrict__ mid, const ta_f2* __restrict__ field, int ni, size_t slot, int h,
                                              int w, float* grid_tab) {
  AugBlock b;
  if (TRAIN) {
    b.rec = ta_load(t);
  } else {
    b.rec.s = sa_load(t);
    b.rec.kind = 0;
  }
  const int hw = h * w;
  b.src.img = images + (size_t)ni * hw * 3;
  b.src.mid = ((b.rec.s.flags & (SA_NOISE | SA_BLUR)) && mid) ? mid + slot * hw : nullptr;
  b.src.d4 = sa_code(b.rec.s.d4, h, w); b.src.h = h; b.src.w = w;
  if (TRAIN) {
    b.geo = ta_geometry(b.rec, field ? field + slot * hw : nullptr, grid_tab, h, w);
    if (b.geo.kind == TA_GRID) ta_grid_table(t, b.geo.cw, b.geo.ch, grid_tab);   // block-uniform
  }
  return b;
}

template <bool TRAIN>
__device__ __forceinline__ void aug_stage4(const AugBlock& b, int y, int x, float (&v)[3]) {
  if (TRAIN) ta_stage4(b.src, b.geo, b.rec, y, x, v);
  else sa_stage4(b.src, b.rec.s, y, x, v);
}

// ------------------------------------------------------------------------------------------------------------------ CLAHE
// Stage-5 kind 3 ("CLAHE"): histogram equalisation of the Lab lightness of the stage-4 image on a fixed 8 x 8
// grid of tiles, clip limit in word 15.  The table pass (clahe.hip) writes uint8 lut[slot][8][8][256]; the output pass blends
// the four neighbouring tiles' entries of the pixel's own bin.  sRGB transfer function, D65 matrix rows divided by the white
// point (0.950456, 1, 1.088754); both matrices are formed in float64 and rounded once to fp32:
constexpr int SA_CLAHE = 3;             // word 5
constexpr int CL_GRID = 8, CL_BINS = 256, CL_TILES = CL_GRID * CL_GRID;
//   forward: (0.412453, 0.357580, 0.180423) / 0.950456 | (0.212671, 0.715160, 0.072169) | (0.019334, 0.119193, 0.950227) / 1.088754
constexpr float CL_M00 = 0.433952749f, CL_M01 = 0.376219422f, CL_M02 = 0.18982783f;
constexpr float CL_M10 = 0.212670997f, CL_M11 = 0.715160012f, CL_M12 = 0.0721689984f;
constexpr float CL_M20 = 0.017757915f, CL_M21 = 0.109476522f, CL_M22 = 0.872765541f;
//   inverse of the forward matrix (float64), rounded once to fp32
constexpr float CL_I00 = 3.07993484f, CL_I01 = -1.53715158f, CL_I02 = -0.542783439f;
constexpr float CL_I10 = -0.92123419f, CL_I11 = 1.87599003f, CL_I12 = 0.0452441797f;
constexpr float CL_I20 = 0.0528896824f, CL_I21 = -0.204041332f, CL_I22 = 1.15115166f;

__device__ __forceinline__ float cl_linear(float v) {           // sRGB level 0..255 -> linear 0..1
  const float c = v / 255.f;
  return c <= 0.04045f ? c / 12.92f : powf((c + 0.055f) / 1.055f, 2.4f);
}

__device__ __forceinline__ float cl_level(float lin) {          // linear -> sRGB level, clamped to 0..255
  const float c = lin <= 0.0031308f ? 12.92f * lin : 1.055f * powf(lin, 1.f / 2.4f) - 0.055f;
  return clamp255(c * 255.f);
}

__device__ __forceinline__ float cl_f(float t) { return t > 0.008856f ? cbrtf(t) : 7.787f * t + 16.f / 116.f; }

__device__ __forceinline__ float cl_f_inv(float f) {
  const float t3 = f * f * f;
  return t3 > 0.008856f ? t3 : (f - 16.f / 116.f) / 7.787f;
}

// lightness on the 8-bit scale (L8 = 2.55 L) and the pixel's own a, b
__device__ __forceinline__ void cl_rgb_to_lab(const float (&v)[3], float& l8, float& a, float& b) {
  const float r = cl_linear(v[0]), g = cl_linear(v[1]), bl = cl_linear(v[2]);
  const float fx = cl_f(CL_M00 * r + CL_M01 * g + CL_M02 * bl);
  const float fy = cl_f(CL_M10 * r + CL_M11 * g + CL_M12 * bl);
  const float fz = cl_f(CL_M20 * r + CL_M21 * g + CL_M22 * bl);
  l8 = 2.55f * (116.f * fy - 16.f);
  a = 500.f * (fx - fy);
  b = 200.f * (fy - fz);
}

__device__ __forceinline__ int cl_bin(float l8) {
  const int k = (int)floorf(l8 + 0.5f);
  return k < 0 ? 0 : (k > CL_BINS - 1 ? CL_BINS - 1 : k);
}

__device__ __forceinline__ void cl_lab_to_rgb(float l8, float a, float b, float (&v)[3]) {
  const float fy = (l8 / 2.55f + 16.f) / 116.f;
  const float x = cl_f_inv(fy + a / 500.f), y = cl_f_inv(fy), z = cl_f_inv(fy - b / 200.f);
  v[0] = cl_level(CL_I00 * x + CL_I01 * y + CL_I02 * z);
  v[1] = cl_level(CL_I10 * x + CL_I11 * y + CL_I12 * z);
  v[2] = cl_level(CL_I20 * x + CL_I21 * y + CL_I22 * z);
}

// position of pixel coordinate x on the axis of tile centres: the two neighbouring tiles and the weight of the second
__device__ __forceinline__ void cl_neighbours(int x, int tile, int& t0, int& t1, float& a) {
  const float tf = (float)x / (float)tile - 0.5f;
  const float fl = floorf(tf);
  a = tf - fl;
  const int i = (int)fl;
  t0 = i > 0 ? i : 0;
  t1 = i + 1 < CL_GRID - 1 ? i + 1 : CL_GRID - 1;
}

// the stage itself at output pixel (y, x): v = the stage-4 image there; lut = the slot's [8][8][256] table
__device__ __forceinline__ void cl_apply(float (&v)[3], const uint8_t* __restrict__ lut, int y, int x, int th, int tw) {
  float l8, a, b;
  cl_rgb_to_lab(v, l8, a, b);
  const int k = cl_bin(l8);
  int x0, x1, y0, y1;
  float ax, ay;
  cl_neighbours(x, tw, x0, x1, ax);
  cl_neighbours(y, th, y0, y1, ay);
  const float l00 = (float)lut[(y0 * CL_GRID + x0) * CL_BINS + k], l01 = (float)lut[(y0 * CL_GRID + x1) * CL_BINS + k];
  const float l10 = (float)lut[(y1 * CL_GRID + x0) * CL_BINS + k], l11 = (float)lut[(y1 * CL_GRID + x1) * CL_BINS + k];
  const float lo = (1.f - ay) * ((1.f - ax) * l00 + ax * l01) + ay * ((1.f - ax) * l10 + ax * l11);
  cl_lab_to_rgb(lo, a, b, v);
}

// the table pass (clahe.hip) for `words`-word records (32: strong, 64: training): one launch, samples not on CLAHE return at once
void clahe_launch_lut(const uint8_t* images, const int32_t* table, int words, int views, int n, int h, int w, const float* mid,
                      const float* field, uint8_t* lut, hipStream_t st);

// the field pass (elastic_field.hip) of n training records: float2 field[n][h][w], written for the samples on elastic alone;
// gauss_weights: 2 radius + 1 taps, radius in 0..TA_MAX_RADIUS (the entry points check both)
void elastic_launch_field(const int32_t* table, int n, int h, int w, const float* gauss_weights, int radius, float* field,
                          hipStream_t st);

}  // namespace udaseg
