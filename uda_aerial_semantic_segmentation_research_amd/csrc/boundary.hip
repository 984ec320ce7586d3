// Label boundary distances on the device: the exact squared Euclidean distance from every pixel to the nearest boundary pixel of
// its label map, capped at a radius R <= 32, and four products of it from ONE tile code: the distance itself, a table lookup
// (boundary weight maps), band erosion of a mask, and the band counters of Boundary IoU / trimap accuracy.
//
// The rule (include/udaseg.h states it in full; tests/_boundary_ref.py is its numpy mirror, bit for bit).  Per image [h][w]:
//   L(p)   the label: uint8, or int64 with a value outside [0, 255] read as 255; void when has_ignore and L(p) == ignore_index
//   B(p)   p is a boundary pixel: some 4-neighbour q INSIDE the image has L(q) != L(p), neither of the two void
//   D2(p)  min over the boundary pixels b of the image of (py - by)^2 + (px - bx)^2
//   d2(p)  D2(p) when D2(p) <= R^2, else R^2 + 1 ("far")
// and, exactly, in two passes because of the cap:
//   g(y, x)  = the smallest |dy| <= R with B(y + dy, x), else R + 1           (columns)
//   D2(y, x) = min over |dx| <= R of dx^2 + g(y, x + dx)^2                    (rows; a term with g = R + 1 is > R^2: far)
//
// Shape.  blockIdx.y is the image, blockIdx.x a tile of th x 64 outputs (th = 32 for R <= 16 and for the counters, 64 above: the
// halo of a 32 x 64 tile is 6.2 x its own labels at R = 32, of a 64 x 64 tile 4.1 x).  A block of 256 threads
//   1. stages the labels of the tile and a halo of R + 1 in LDS as 16-bit values (BD_DEAD for a void pixel and for a position
//      outside the image: such a position is never different from anything and never a boundary),
//   2. makes the flags B of the tile and a halo of R (bytes),
//   3. runs the column pass as a running scan down and a running scan up (a thread owns one column of one band of rows, and
//      walks R rows into the band's halo first): g, one byte per value, th x (64 + 2R) of them,
//   4. runs the row pass: a thread takes four consecutive pixels, reads the 4 + 2R bytes of g under them as 1 + ceil(R / 2)
//      words and folds every byte into its four minima (a byte further than R columns from a pixel has dx^2 > R^2 by itself and
//      needs no test),
//   5. hands the four d2 to the product's epilogue.  d2 goes to memory in udaseg_boundary_d2 only.
// The counters run the truth map and then the prediction through steps 1-4 in the same block, keep the truth's band (and label)
// of the tile in LDS between the two, count into an LDS table and flush it with one 64-bit atomic per non-zero counter: integer
// adds, the same maps give the same bits in any order.
#include "label_maps.h"

namespace udaseg {

constexpr int BD_THREADS = 256;
static_assert(BD_THREADS == 64 * 4, "BlockCounts<K>: four waves a block");
constexpr int BD_TW = 64;                      // tile width: 16 groups of four pixels
constexpr int BD_MAX_R = 32;
constexpr int BD_DEAD = 0x100;                 // a void pixel or a position outside the image
constexpr int BD_BAND = 0x8000;                // the truth's band bit beside its label (counters)

static inline int bd_tile_h(int R, bool stats) { return (!stats && R > 16) ? 64 : 32; }

struct BdGeom {
  int h, w, R, th;
  int lh, lw;                                  // staged labels: (th + 2R + 2) x (64 + 2R + 2), 16-bit
  int fh, fw;                                  // flags: (th + 2R) x (64 + 2R), bytes
  int gs;                                      // row stride of g in bytes, a multiple of 4 that covers the row pass's last word
  float rcp_lw, rcp_fw;
  int has_ignore, ignore_index;
  int off_g, off_flg, off_extra;               // byte offsets into the block's LDS (labels at 0)
};

static inline BdGeom bd_geom(int h, int w, int R, int th, int has_ignore, int ignore_index) {
  BdGeom G;
  G.h = h;
  G.w = w;
  G.R = R;
  G.th = th;
  G.lh = th + 2 * R + 2;
  G.lw = BD_TW + 2 * R + 2;
  G.fh = th + 2 * R;
  G.fw = BD_TW + 2 * R;
  G.gs = (BD_TW + 2 * R + 2 + 3) & ~3;
  G.rcp_lw = 1.0f / (float)G.lw;
  G.rcp_fw = 1.0f / (float)G.fw;
  G.has_ignore = has_ignore;
  G.ignore_index = ignore_index;
  G.off_g = (2 * G.lh * G.lw + 3) & ~3;
  G.off_flg = G.off_g + th * G.gs;
  G.off_extra = (G.off_flg + G.fh * G.fw + 3) & ~3;
  return G;
}

// Steps 1-3 for the tile at (ty0, tx0) of one image: leaves the staged labels in lab and g in gcol.  mask_img (may be null): a
// second map of the image whose void pixels are void here too (the prediction under the truth).  Ends with a barrier.
template <bool I64>
__device__ __forceinline__ void bd_tile(const BdGeom& G, const void* __restrict__ img, const void* __restrict__ mask_img, int ty0,
                                        int tx0, unsigned short* __restrict__ lab, uint8_t* __restrict__ flg,
                                        uint8_t* __restrict__ gcol) {
  const int tid = threadIdx.x;
  const int R = G.R, h = G.h, w = G.w, lw = G.lw, fw = G.fw;
  for (int i = tid; i < G.lh * lw; i += BD_THREADS) {
    const int ly = fast_div(i, lw, G.rcp_lw), lx = i - ly * lw;
    const int y = ty0 - R - 1 + ly, x = tx0 - R - 1 + lx;
    int v = BD_DEAD;
    if (y >= 0 && y < h && x >= 0 && x < w) {                      // every global read is inside the image
      const int64_t p = (int64_t)y * w + x;
      v = label_at<I64>(img, p);
      if (G.has_ignore && (v == G.ignore_index || (mask_img && label_at<I64>(mask_img, p) == G.ignore_index))) v = BD_DEAD;
    }
    lab[i] = (unsigned short)v;
  }
  __syncthreads();
  for (int i = tid; i < G.fh * fw; i += BD_THREADS) {
    const int fy = fast_div(i, fw, G.rcp_fw), fx = i - fy * fw;
    const unsigned short* c = lab + (fy + 1) * lw + fx + 1;         // the flags lie one inside the staged labels: all four neighbours exist
    const int l = c[0];
    bool f = false;
    if (l != BD_DEAD) {
      const int a = c[-1], b = c[1], u = c[-lw], d = c[lw];
      f = (a != BD_DEAD && a != l) || (b != BD_DEAD && b != l) || (u != BD_DEAD && u != l) || (d != BD_DEAD && d != l);
    }
    flg[i] = f ? 1 : 0;
  }
  __syncthreads();
  // tile row t is flag row t + R.  Bands of rows [y0, y1): 256 / fw of them (fw <= 128), a thread per (band, column).
  const int nseg = BD_THREADS / fw;
  const int seg_len = (G.th + nseg - 1) / nseg;
  const int seg = fast_div(tid, fw, G.rcp_fw), col = tid - seg * fw;
  const int y0 = seg * seg_len;
  const int y1 = y0 + seg_len < G.th ? y0 + seg_len : G.th;
  if (seg < nseg && y0 < y1) {
    int d = R + 1;
    for (int fr = y0; fr < y1 + R; ++fr) {                           // down: rows y0 - R .. y1 - 1 of the tile
      d = flg[fr * fw + col] ? 0 : (d < R + 1 ? d + 1 : R + 1);
      if (fr >= y0 + R) gcol[(fr - R) * G.gs + col] = (uint8_t)d;
    }
    d = R + 1;
    for (int fr = y1 - 1 + 2 * R; fr >= y0 + R; --fr) {              // up: rows y1 - 1 + R .. y0; fr < th + 2R = fh
      d = flg[fr * fw + col] ? 0 : (d < R + 1 ? d + 1 : R + 1);
      if (fr < y1 + R) {
        uint8_t* q = gcol + (fr - R) * G.gs + col;
        if (d < (int)*q) *q = (uint8_t)d;
      }
    }
  }
  __syncthreads();
}

// Step 4: emit(y, x0, d2[4]) for the four pixels (y, x0 .. x0 + 3) of the tile, every group of it once.  g column c is tile
// column c - R, so byte jj of the words under pixel x0 + e is dx = jj - e - R away from it.
template <typename F>
__device__ __forceinline__ void bd_rows(const BdGeom& G, const uint8_t* __restrict__ gcol, F&& emit) {
  const int R = G.R, far = R * R + 1;
  const int words = (2 * R + 4 + 3) >> 2;
  for (int q = threadIdx.x; q < G.th * (BD_TW / 4); q += BD_THREADS) {
    const int y = q >> 4, x0 = (q & 15) << 2;
    const unsigned int* row = reinterpret_cast<const unsigned int*>(gcol + y * G.gs + x0);
    int best[4] = {far, far, far, far};
    for (int j = 0; j < words; ++j) {
      const unsigned int v = row[j];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int gv = (int)((v >> (8 * k)) & 255u);
        const int g2 = gv * gv;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int dx = 4 * j + k - e - R;
          const int c = g2 + dx * dx;
          best[e] = c < best[e] ? c : best[e];
        }
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) best[e] = best[e] > R * R ? far : best[e];
    emit(y, x0, best);
  }
}

constexpr int BD_D2 = 0, BD_LOOKUP = 1, BD_ERODE = 2;

struct BdArgs {
  const void* labels;
  const void* truth;                 // counters: the truth map (labels is the prediction)
  void* out;
  const float* table;
  unsigned long long* counts;        // erode: [n][2]
  unsigned long long* stats;         // counters: [classes][3]
  unsigned long long* trimap;        // counters: [2]
  BdGeom G;
  int tiles_x, void_label, classes;
};

template <bool I64, int PRODUCT>
__global__ __launch_bounds__(BD_THREADS) void boundary_kernel(BdArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char bd_lds[];
  const BdGeom& G = A.G;
  unsigned short* lab = reinterpret_cast<unsigned short*>(bd_lds);
  uint8_t* gcol = bd_lds + G.off_g;
  uint8_t* flg = bd_lds + G.off_flg;
  float* tab = reinterpret_cast<float*>(bd_lds + G.off_extra);              // lookup: R^2 + 3 floats
  BlockCounts<2>::Slots& ecnt = *reinterpret_cast<BlockCounts<2>::Slots*>(bd_lds + G.off_extra);   // erode: voided, void
  const int tid = threadIdx.x, n = blockIdx.y;
  const int R = G.R, h = G.h, w = G.w;
  const int ty0 = ((int)blockIdx.x / A.tiles_x) * G.th, tx0 = ((int)blockIdx.x % A.tiles_x) * BD_TW;
  const int64_t HW = (int64_t)h * w;
  const uint8_t* img = reinterpret_cast<const uint8_t*>(A.labels) + (size_t)n * HW * (I64 ? 8 : 1);
  if (PRODUCT == BD_LOOKUP)
    for (int i = tid; i < R * R + 3; i += BD_THREADS) tab[i] = A.table[i];
  bd_tile<I64>(G, img, nullptr, ty0, tx0, lab, flg, gcol);                  // its barriers cover the fill above

  constexpr int ELT = PRODUCT == BD_ERODE ? 1 : 4;
  uint8_t* out_img = reinterpret_cast<uint8_t*>(A.out) + (size_t)n * HW * ELT;
  // four outputs of a group go out as one access when every group of the image is whole and aligned (uniform over the block)
  const bool vec = (w & 3) == 0 && (reinterpret_cast<uintptr_t>(out_img) & (4 * ELT - 1)) == 0;
  unsigned int ev[2] = {0, 0};                                               // voided, void
  bd_rows(G, gcol, [&](int y, int x0, const int (&d2)[4]) {
    const int gy = ty0 + y, gx = tx0 + x0;
    if (gy >= h || gx >= w) return;
    const int cnt = w - gx >= 4 ? 4 : w - gx;                                // pixels gx .. gx + cnt - 1 exist
    const unsigned short* lc = lab + (y + R + 1) * G.lw + x0 + R + 1;
    const int64_t p = (int64_t)gy * w + gx;
    if (PRODUCT == BD_D2) {
      int* dst = reinterpret_cast<int*>(out_img) + p;
      if (vec) {
        *reinterpret_cast<int4*>(dst) = make_int4(d2[0], d2[1], d2[2], d2[3]);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (e < cnt) dst[e] = d2[e];
      }
    } else if (PRODUCT == BD_LOOKUP) {
      float v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = tab[lc[e] == BD_DEAD ? R * R + 2 : d2[e]];   // lc[e] of a missing pixel is DEAD: a valid slot
      float* dst = reinterpret_cast<float*>(out_img) + p;
      if (vec) {
        *reinterpret_cast<f32x4*>(dst) = f32x4{v[0], v[1], v[2], v[3]};
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (e < cnt) dst[e] = v[e];
      }
    } else {
      unsigned int o[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int l = lc[e];
        if (l == BD_DEAD) {                                                  // void: its label is ignore_index
          o[e] = (unsigned int)G.ignore_index;
          if (e < cnt) ++ev[1];
        } else if (d2[e] <= R * R) {
          o[e] = (unsigned int)A.void_label;
          if (e < cnt) ++ev[0];
        } else {
          o[e] = (unsigned int)l;
        }
      }
      uint8_t* dst = out_img + p;
      if (vec) {
        *reinterpret_cast<unsigned int*>(dst) = o[0] | (o[1] << 8) | (o[2] << 16) | (o[3] << 24);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (e < cnt) dst[e] = (uint8_t)o[e];
      }
    }
  });
  if (PRODUCT == BD_ERODE && A.counts) BlockCounts<2>::add(ecnt, ev, A.counts + (size_t)n * 2);   // uniform over the block
}

template <bool I64>
__global__ __launch_bounds__(BD_THREADS) void boundary_stats_kernel(BdArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char bd_lds[];
  const BdGeom& G = A.G;
  unsigned short* lab = reinterpret_cast<unsigned short*>(bd_lds);
  uint8_t* gcol = bd_lds + G.off_g;
  uint8_t* flg = bd_lds + G.off_flg;
  unsigned int* cnt = reinterpret_cast<unsigned int*>(bd_lds + G.off_extra);           // [classes][3] then the trimap's two
  const int ncnt = 3 * A.classes + 2;
  unsigned short* tband = reinterpret_cast<unsigned short*>(cnt + ncnt);                // [th][64]: truth label | BD_BAND
  const int tid = threadIdx.x, n = blockIdx.y;
  const int R = G.R, h = G.h, w = G.w, classes = A.classes;
  const int ty0 = ((int)blockIdx.x / A.tiles_x) * G.th, tx0 = ((int)blockIdx.x % A.tiles_x) * BD_TW;
  const int64_t HW = (int64_t)h * w;
  const uint8_t* pred = reinterpret_cast<const uint8_t*>(A.labels) + (size_t)n * HW * (I64 ? 8 : 1);
  const uint8_t* truth = reinterpret_cast<const uint8_t*>(A.truth) + (size_t)n * HW * (I64 ? 8 : 1);
  for (int i = tid; i < ncnt; i += BD_THREADS) cnt[i] = 0;

  bd_tile<I64>(G, truth, nullptr, ty0, tx0, lab, flg, gcol);
  bd_rows(G, gcol, [&](int y, int x0, const int (&d2)[4]) {
    const unsigned short* lc = lab + (y + R + 1) * G.lw + x0 + R + 1;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int l = lc[e];                                                               // DEAD outside the image too
      tband[y * BD_TW + x0 + e] = (unsigned short)(l | ((l != BD_DEAD && d2[e] <= R * R) ? BD_BAND : 0));
    }
  });
  __syncthreads();                                                                       // lab and g are read above, rewritten below
  bd_tile<I64>(G, pred, truth, ty0, tx0, lab, flg, gcol);
  bd_rows(G, gcol, [&](int y, int x0, const int (&d2)[4]) {
    const unsigned short* lc = lab + (y + R + 1) * G.lw + x0 + R + 1;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int tv = tband[y * BD_TW + x0 + e];
      const int T = tv & 0x1ff, P = lc[e];
      const bool in_t = (tv & BD_BAND) != 0;                                             // false for void and outside the image
      const bool in_p = P != BD_DEAD && d2[e] <= R * R;
      if (in_t) {
        atomicAdd(&cnt[3 * classes], 1u);
        if (P == T) atomicAdd(&cnt[3 * classes + 1], 1u);
        if (T < classes) atomicAdd(&cnt[3 * T], 1u);
      }
      if (in_p && P < classes) atomicAdd(&cnt[3 * P + 1], 1u);
      if (in_t && in_p && P == T && T < classes) atomicAdd(&cnt[3 * T + 2], 1u);
    }
  });
  __syncthreads();
  for (int i = tid; i < ncnt; i += BD_THREADS) {
    const unsigned int v = cnt[i];
    if (v) atomicAdd(i < 3 * classes ? &A.stats[i] : &A.trimap[i - 3 * classes], (unsigned long long)v);
  }
}

// the argument rules every entry point shares; 0 or UDASEG_E_BADARG with the message set
static int bd_check(const char* who, int labels_i64, int n, int h, int w, int radius, int has_ignore, int ignore_index) {
  if (int rc = map_storage_ok(who, "labels_i64", labels_i64)) return rc;
  if (int rc = map_extent_ok(who, n, h, w)) return rc;
  UDASEG_CHECK_ARG(radius >= 0 && radius <= BD_MAX_R, "%s: need 0 <= radius <= %d (radius=%d)", who, BD_MAX_R, radius);
  return map_ignore_ok(who, has_ignore, ignore_index);
}

template <typename K>
static int bd_launch(const char* who, K kern, std::atomic<bool>* attr_done, BdArgs& A, int n, size_t extra, hipStream_t st) {
  const size_t lds = (size_t)A.G.off_extra + extra;
  if (lds > 48 * 1024 && !*attr_done) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024);
    if (e != hipSuccess) return hip_fail(e, "hipFuncSetAttribute(boundary)");
    *attr_done = true;
  }
  A.tiles_x = cdiv(A.G.w, BD_TW);
  const int64_t tiles = (int64_t)A.tiles_x * cdiv(A.G.h, A.G.th);
  hipLaunchKernelGGL(kern, dim3((unsigned int)tiles, (unsigned int)n), dim3(BD_THREADS), lds, st, A);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, who);
  return UDASEG_OK;
}

template <int PRODUCT>
static int bd_product(const char* who, const void* labels, int labels_i64, int n, int h, int w, int radius, int has_ignore,
                      int ignore_index, BdArgs& A, size_t extra, void* stream) {
  if (int rc = map_aligned_ok(who, "labels", labels_i64, labels)) return rc;
  A.labels = labels;
  A.truth = nullptr;
  A.G = bd_geom(h, w, radius, bd_tile_h(radius, false), has_ignore, ignore_index);
  static std::atomic<bool> attr_done[2] = {{false}, {false}};
  return dispatch_flags(
      [&](auto i64) {
        return bd_launch(who, boundary_kernel<decltype(i64)::value, PRODUCT>, &attr_done[decltype(i64)::value], A, n, extra,
                         as_stream(stream));
      },
      labels_i64 != 0);
}

}  // namespace udaseg

using namespace udaseg;

extern "C" int udaseg_boundary_tile(int radius, int stats) {
  UDASEG_CHECK_ARG(radius >= 0 && radius <= BD_MAX_R, "boundary_tile: need 0 <= radius <= %d (radius=%d)", BD_MAX_R, radius);
  return (bd_tile_h(radius, stats != 0) << 16) | BD_TW;
}

extern "C" int udaseg_boundary_d2(const void* labels, int labels_i64, int n, int h, int w, int radius, int has_ignore,
                                  int ignore_index, int32_t* d2, void* stream) {
  if (int rc = bd_check("boundary_d2", labels_i64, n, h, w, radius, has_ignore, ignore_index)) return rc;
  UDASEG_CHECK_ARG(labels && d2, "boundary_d2: NULL pointer (labels and d2 are required)");
  UDASEG_CHECK_ARG((reinterpret_cast<uintptr_t>(d2) & 3) == 0, "boundary_d2: d2 must be 4-byte aligned");
  BdArgs A = {};
  A.out = d2;
  return bd_product<BD_D2>("boundary_d2 launch", labels, labels_i64, n, h, w, radius, has_ignore, ignore_index, A, 0, stream);
}

extern "C" int udaseg_boundary_lookup(const void* labels, int labels_i64, int n, int h, int w, int radius, int has_ignore,
                                      int ignore_index, const float* table, float* out, void* stream) {
  if (int rc = bd_check("boundary_lookup", labels_i64, n, h, w, radius, has_ignore, ignore_index)) return rc;
  UDASEG_CHECK_ARG(labels && table && out, "boundary_lookup: NULL pointer (labels, table and out are required)");
  UDASEG_CHECK_ARG(((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(table)) & 3) == 0,
                   "boundary_lookup: table and out must be 4-byte aligned");
  BdArgs A = {};
  A.out = out;
  A.table = table;
  return bd_product<BD_LOOKUP>("boundary_lookup launch", labels, labels_i64, n, h, w, radius, has_ignore, ignore_index, A,
                               sizeof(float) * (size_t)(radius * radius + 3), stream);
}

extern "C" int udaseg_boundary_erode(const void* labels, int labels_i64, int n, int h, int w, int radius, int has_ignore,
                                     int ignore_index, int void_label, uint8_t* out, int64_t* counts, void* stream) {
  if (int rc = bd_check("boundary_erode", labels_i64, n, h, w, radius, has_ignore, ignore_index)) return rc;
  UDASEG_CHECK_ARG(void_label >= 0 && void_label <= 255, "boundary_erode: void_label must lie in [0, 255] (void_label=%d)", void_label);
  UDASEG_CHECK_ARG(labels && out, "boundary_erode: NULL pointer (labels and out are required)");
  UDASEG_CHECK_ARG((reinterpret_cast<uintptr_t>(counts) & 7) == 0, "boundary_erode: counts must be 8-byte aligned");
  BdArgs A = {};
  A.out = out;
  A.counts = reinterpret_cast<unsigned long long*>(counts);
  A.void_label = void_label;
  return bd_product<BD_ERODE>("boundary_erode launch", labels, labels_i64, n, h, w, radius, has_ignore, ignore_index, A,
                              sizeof(BlockCounts<2>::Slots), stream);
}

extern "C" int udaseg_boundary_stats(const void* pred, const void* truth, int labels_i64, int n, int h, int w, int radius,
                                     int classes, int has_ignore, int ignore_index, int64_t* stats, int64_t* trimap, void* stream) {
  if (int rc = bd_check("boundary_stats", labels_i64, n, h, w, radius, has_ignore, ignore_index)) return rc;
  UDASEG_CHECK_ARG(classes >= 1 && classes <= 255, "boundary_stats: need 1 <= classes <= 255 (classes=%d)", classes);
  UDASEG_CHECK_ARG(pred && truth && stats && trimap, "boundary_stats: NULL pointer (pred, truth, stats and trimap are required)");
  UDASEG_CHECK_ARG(((reinterpret_cast<uintptr_t>(stats) | reinterpret_cast<uintptr_t>(trimap)) & 7) == 0,
                   "boundary_stats: stats and trimap must be 8-byte aligned");
  if (int rc = map_aligned_ok("boundary_stats", "pred / truth", labels_i64, pred, truth)) return rc;
  BdArgs A = {};
  A.labels = pred;
  A.truth = truth;
  A.stats = reinterpret_cast<unsigned long long*>(stats);
  A.trimap = reinterpret_cast<unsigned long long*>(trimap);
  A.classes = classes;
  A.G = bd_geom(h, w, radius, bd_tile_h(radius, true), has_ignore, ignore_index);
  const size_t extra = sizeof(unsigned int) * (size_t)(3 * classes + 2) + sizeof(unsigned short) * (size_t)(A.G.th * BD_TW);
  static std::atomic<bool> attr_done[2] = {{false}, {false}};
  return dispatch_flags(
      [&](auto i64) {
        return bd_launch("boundary_stats launch", boundary_stats_kernel<decltype(i64)::value>, &attr_done[decltype(i64)::value], A, n,
                         extra, as_stream(stream));
      },
      labels_i64 != 0);
}
