// Window votes of label maps and the acquisition scores of active labelling (RIPU, Xie et al., CVPR 2022) on the device.
//
// The one primitive: n_c(p), the number of pixels of class c among the pixels of a (2R+1)^2 window around p that lie inside the
// image and are not void (include/udaseg.h states every rule in full; tests/_active_ref.py is the numpy mirror).  From it, in ONE
// tile code: the mode filter and the agreement (udaseg_window_mode), the impurity (udaseg_window_impurity) and the acquisition
// score and key (udaseg_acquire_score, which also box-sums the entropy map).
//
// Shape.  blockIdx.y is the image, blockIdx.x a tile of th x 64 outputs, th = 32 for R <= 8 and 16 above (the halo rows of a 32-row
// tile at R = 16 would be two thirds of the staged rows).  A block of 256 threads
//   1. stages the labels of the tile and a halo of R in LDS as bytes (WN_DEAD for a void pixel, a label >= classes and a position
//      outside the image: none of them counts in any window),
//   2. runs, for every group g of FOUR classes, two integer passes over 64-bit words that hold four 16-bit counters (a window
//      holds at most 33^2 = 1089 pixels, so no field carries into the next; 16-bit fields rather than 11-bit ones so that a count
//      leaves its word with a shift and a mask by a multiple of 16 -- at 23 classes that is six words against five):
//        a. down the columns: a thread owns one column of the staged tile and a band of tile rows, sums the first 2R + 1 one-hot
//           words and then slides (add the entering row, subtract the leaving one: integers, no field goes negative),
//        b. along the rows: thread (y, s) owns th / 4 consecutive pixels of tile row y and slides the same way over the column
//           sums; lanes of a wave lie on consecutive ROWS, and the row stride of the column sums is 97 words (1 mod 32), so the
//           64-bit reads of 32 lanes fall on distinct banks,
//      and folds the four counts of every pixel into its running n, its best (count, class), its centre's count and the impurity's
//      table sum -- in ascending class order, which is the order of the groups,
//   3. hands the th / 4 pixels to the product's epilogue.
// The score product first stages the entropy tile (0 at a dead position) and sums it DIRECTLY: a row pass of 2R + 1 terms left to
// right into LDS, then a column pass of 2R + 1 row sums top to bottom in the owner thread -- no running add / subtract, which would
// carry its cancellation error along the tile.
// No atomics on the maps; the counters take one LDS slot per wave and one 64-bit atomic per block and non-zero counter (BlockCounts).
#include "label_maps.h"
#include "scores_common.h"

namespace udaseg {

constexpr int WN_THREADS = 256;
static_assert(WN_THREADS == 64 * 4, "BlockCounts<K>: four waves a block");
constexpr int WN_TW = 64;
constexpr int WN_MAX_R = 16;
constexpr int WN_DEAD = 0xff;
constexpr int WN_CS = 97;                      // row stride of the packed column sums, in 64-bit words
constexpr int WN_ES = 65;                      // row stride of the entropy row sums, in floats

constexpr int WN_MODE = 0, WN_IMPURITY = 1, WN_SCORE = 2;

static inline int wn_tile_h(int R) { return R > 8 ? 16 : 32; }

struct WnGeom {
  int h, w, R, th, classes, groups;
  int lh, lw, lws;                             // staged labels: (th + 2R) x (64 + 2R) bytes, row stride lws
  float rcp_lw;
  int has_ignore, ignore_index;
  int off_col, off_tab, off_ent, off_cnt, lds; // byte offsets into the block's LDS (labels at 0)
  int tiles_x;
};

static inline WnGeom wn_geom(int h, int w, int R, int classes, int has_ignore, int ignore_index, int product) {
  WnGeom G;
  G.h = h;
  G.w = w;
  G.R = R;
  G.th = wn_tile_h(R);
  G.classes = classes;
  G.groups = (classes + 3) >> 2;
  G.lh = G.th + 2 * R;
  G.lw = WN_TW + 2 * R;
  G.lws = (G.lw + 3) & ~3;
  G.rcp_lw = 1.0f / (float)G.lw;
  G.has_ignore = has_ignore;
  G.ignore_index = ignore_index;
  G.off_col = (G.lh * G.lws + 7) & ~7;
  int col_bytes = G.th * WN_CS * 8;
  if (product == WN_SCORE && G.lh * WN_ES * 4 > col_bytes) col_bytes = (G.lh * WN_ES * 4 + 7) & ~7;   // the row sums share it
  G.off_tab = G.off_col + col_bytes;
  G.off_ent = G.off_tab + (product == WN_MODE ? 0 : 4 * ((2 * R + 1) * (2 * R + 1) + 1));
  G.off_cnt = G.off_ent + (product == WN_SCORE ? 4 * G.lh * G.lw : 0);
  G.lds = G.off_cnt + (int)sizeof(BlockCounts<3>::Slots);
  G.tiles_x = cdiv(w, WN_TW);
  return G;
}

struct WnArgs {
  const void* labels;
  const float* entropy;              // score
  const uint8_t* exclude;            // score, may be null
  const float* table;                // impurity, score: m log m, (2R+1)^2 + 1 entries
  void* out;                         // mode: uint8 labels; impurity: fp32; score: fp32 score
  float* out2;                       // mode: agreement (may be null); score: key
  unsigned long long* counts;        // mode: [n][3], may be null
  WnGeom G;
  int fill_void, void_label, kind;
  float log_classes;
};

// what a pixel of the window tells about itself after all groups
struct WnPixel {
  int n, best_cnt, best_cls, ctr_cnt;
  float tsum;
};

// SEG values of one tile row go out: as whole 16-byte (fp32) or 4-byte (uint8) accesses when `vec` (uniform over the block: every
// group of four pixels of the image is whole and aligned), else one by one below `cnt`.
template <int SEG>
__device__ __forceinline__ void wn_store(float* dst, const float (&v)[SEG], int cnt, bool vec) {
  if (vec) {
#pragma unroll
    for (int q = 0; q < SEG / 4; ++q)
      if (4 * q < cnt) *reinterpret_cast<f32x4*>(dst + 4 * q) = f32x4{v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]};
  } else {
#pragma unroll
    for (int e = 0; e < SEG; ++e)
      if (e < cnt) dst[e] = v[e];
  }
}
template <int SEG>
__device__ __forceinline__ void wn_store(uint8_t* dst, const unsigned int (&v)[SEG], int cnt, bool vec) {
  if (vec) {
#pragma unroll
    for (int q = 0; q < SEG / 4; ++q)
      if (4 * q < cnt)
        *reinterpret_cast<unsigned int*>(dst + 4 * q) = v[4 * q] | (v[4 * q + 1] << 8) | (v[4 * q + 2] << 16) | (v[4 * q + 3] << 24);
  } else {
#pragma unroll
    for (int e = 0; e < SEG; ++e)
      if (e < cnt) dst[e] = (uint8_t)v[e];
  }
}

template <bool I64, int TH, int PRODUCT>
__global__ __launch_bounds__(WN_THREADS) void window_kernel(WnArgs A) {
#pragma clang fp contract(off)                                       // key = 1.0f - A with A rounded: the mirror's two roundings
  extern __shared__ __attribute__((aligned(16))) unsigned char wn_lds[];
  constexpr int SEG = TH / 4;                                        // pixels of a tile row per thread: TH * 64 / SEG = 256 threads
  const WnGeom& G = A.G;
  uint8_t* lab = wn_lds;
  unsigned long long* col = reinterpret_cast<unsigned long long*>(wn_lds + G.off_col);
  float* erow = reinterpret_cast<float*>(wn_lds + G.off_col);      // score: the entropy row sums, before the first group
  float* tab = reinterpret_cast<float*>(wn_lds + G.off_tab);
  float* ent = reinterpret_cast<float*>(wn_lds + G.off_ent);
  BlockCounts<3>::Slots& bcnt = *reinterpret_cast<BlockCounts<3>::Slots*>(wn_lds + G.off_cnt);
  const int tid = threadIdx.x, img_i = blockIdx.y;
  const int R = G.R, h = G.h, w = G.w, lw = G.lw, lws = G.lws, lh = G.lh;
  const int ty0 = ((int)blockIdx.x / G.tiles_x) * TH, tx0 = ((int)blockIdx.x % G.tiles_x) * WN_TW;
  const int64_t HW = (int64_t)h * w;
  const uint8_t* img = reinterpret_cast<const uint8_t*>(A.labels) + (size_t)img_i * HW * (I64 ? 8 : 1);
  const float* ent_img = PRODUCT == WN_SCORE ? A.entropy + (size_t)img_i * HW : nullptr;

  // 1. the labels (and the entropy) of the tile and its halo
  for (int i = tid; i < lh * lw; i += WN_THREADS) {
    const int ly = fast_div(i, lw, G.rcp_lw), lx = i - ly * lw;
    const int y = ty0 - R + ly, x = tx0 - R + lx;
    int v = WN_DEAD;
    float e = 0.f;
    if (y >= 0 && y < h && x >= 0 && x < w) {                        // every global read is inside the image
      const int64_t p = (int64_t)y * w + x;
      v = label_at<I64>(img, p);
      if ((G.has_ignore && v == G.ignore_index) || v >= G.classes) v = WN_DEAD;
      if (PRODUCT == WN_SCORE && v != WN_DEAD) e = ent_img[p];
    }
    lab[ly * lws + lx] = (uint8_t)v;
    if (PRODUCT == WN_SCORE) ent[i] = e;
  }
  if (PRODUCT != WN_MODE)
    for (int i = tid; i < (2 * R + 1) * (2 * R + 1) + 1; i += WN_THREADS) tab[i] = A.table[i];
  __syncthreads();

  const int oy = tid % TH, ox0 = (tid / TH) * SEG;                   // the owner of pixels (oy, ox0 .. ox0 + SEG - 1) of the tile
  float usum[SEG];
  if (PRODUCT == WN_SCORE) {
    for (int i = tid; i < lh * WN_TW; i += WN_THREADS) {             // rows: 2R + 1 terms, left to right
      const int r = i >> 6, x = i & 63;
      const float* s = ent + r * lw + x;
      float a = s[0];
      for (int j = 1; j <= 2 * R; ++j) a += s[j];
      erow[r * WN_ES + x] = a;
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < SEG; ++e) {                                  // columns: 2R + 1 row sums, top to bottom
      const float* s = erow + oy * WN_ES + ox0 + e;
      float a = s[0];
      for (int j = 1; j <= 2 * R; ++j) a += s[j * WN_ES];
      usum[e] = a;
    }
    __syncthreads();                                                 // the column sums below overwrite the row sums
  }

  // 2. the box counts, four classes at a time
  WnPixel px[SEG];
#pragma unroll
  for (int e = 0; e < SEG; ++e) px[e] = WnPixel{0, 0, 0, 0, 0.f};
  const int nb = WN_THREADS / lw;                                    // bands of tile rows in pass a (lw <= 96: at least two)
  const int band_len = (TH + nb - 1) / nb;
  const int band = fast_div(tid, lw, G.rcp_lw), bx = tid - band * lw;
  const int by0 = band * band_len;
  const int by1 = by0 + band_len < TH ? by0 + band_len : TH;
  int ctr[SEG];
#pragma unroll
  for (int e = 0; e < SEG; ++e) ctr[e] = lab[(oy + R) * lws + ox0 + e + R];

  for (int g = 0; g < G.groups; ++g) {
    auto one_hot = [&](int l) -> unsigned long long { return (l >> 2) == g ? 1ull << ((l & 3) << 4) : 0ull; };
    if (band < nb && by0 < by1) {                                    // a. tile row y sums staged rows y .. y + 2R
      const uint8_t* c = lab + bx;
      unsigned long long s = 0;
      for (int r = by0; r <= by0 + 2 * R; ++r) s += one_hot(c[r * lws]);
      col[by0 * WN_CS + bx] = s;
      for (int y = by0 + 1; y < by1; ++y) {
        s += one_hot(c[(y + 2 * R) * lws]) - one_hot(c[(y - 1) * lws]);
        col[y * WN_CS + bx] = s;
      }
    }
    __syncthreads();
    {                                                                // b. tile column x sums staged columns x .. x + 2R
      const unsigned long long* c = col + oy * WN_CS + ox0;
      unsigned long long s = 0;
      for (int j = 0; j <= 2 * R; ++j) s += c[j];
#pragma unroll
      for (int e = 0; e < SEG; ++e) {
        if (e > 0) s += c[e + 2 * R] - c[e - 1];
        WnPixel& P = px[e];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int cnt = (int)((s >> (16 * k)) & 0xffffull);        // the fields of classes >= `classes` stay 0
          P.n += cnt;
          if (PRODUCT != WN_MODE) P.tsum += tab[cnt];
          if (cnt > P.best_cnt) { P.best_cnt = cnt; P.best_cls = 4 * g + k; }
        }
        if ((ctr[e] >> 2) == g) P.ctr_cnt = (int)((s >> ((ctr[e] & 3) << 4)) & 0xffffull);
      }
    }
    __syncthreads();
  }

  // 3. the products
  const int gy = ty0 + oy, gx = tx0 + ox0;
  unsigned int ev[3] = {0, 0, 0};                                    // changed, filled, left
  if (gy < h && gx < w) {
    const int cnt = w - gx >= SEG ? SEG : w - gx;                    // pixels gx .. gx + cnt - 1 exist
    const int64_t p = (int64_t)gy * w + gx;
    if (PRODUCT == WN_MODE) {
      uint8_t* out_img = reinterpret_cast<uint8_t*>(A.out) + (size_t)img_i * HW;
      unsigned int o[SEG];
      float ag[SEG];
#pragma unroll
      for (int e = 0; e < SEG; ++e) {
        const WnPixel& P = px[e];
        const int l = ctr[e];
        const int mode = (l != WN_DEAD && P.ctr_cnt == P.best_cnt) ? l : P.best_cls;
        ag[e] = P.n > 0 ? (float)P.best_cnt / (float)P.n : 0.f;
        if (l != WN_DEAD) {
          o[e] = (unsigned int)mode;
          if (e < cnt && mode != l) ++ev[0];
        } else if (A.fill_void && P.n > 0) {
          o[e] = (unsigned int)mode;
          if (e < cnt) ++ev[1];
        } else {
          o[e] = (unsigned int)A.void_label;
          if (e < cnt) ++ev[2];
        }
      }
      wn_store<SEG>(out_img + p, o, cnt, (w & 3) == 0 && (reinterpret_cast<uintptr_t>(out_img) & 3) == 0);
      if (A.out2) {
        float* ag_img = A.out2 + (size_t)img_i * HW;
        wn_store<SEG>(ag_img + p, ag, cnt, (w & 3) == 0 && (reinterpret_cast<uintptr_t>(ag_img) & 15) == 0);
      }
    } else {
      float imp[SEG];
#pragma unroll
      for (int e = 0; e < SEG; ++e) {
        const WnPixel& P = px[e];
        float v = 0.f;
        if (P.n > 1) {
          v = (tab[P.n] - P.tsum) / ((float)P.n * A.log_classes);
          v = v < 0.f ? 0.f : (v > 1.f ? 1.f : v);
        }
        imp[e] = v;
      }
      if (PRODUCT == WN_IMPURITY) {
        float* out_img = reinterpret_cast<float*>(A.out) + (size_t)img_i * HW;
        wn_store<SEG>(out_img + p, imp, cnt, (w & 3) == 0 && (reinterpret_cast<uintptr_t>(out_img) & 15) == 0);
      } else {
        const uint8_t* exc = A.exclude ? A.exclude + (size_t)img_i * HW + p : nullptr;
        float sc[SEG], key[SEG];
#pragma unroll
        for (int e = 0; e < SEG; ++e) {
          const WnPixel& P = px[e];
          const float unc = P.n > 0 ? usum[e] / (float)P.n : 0.f;
          const float a0 = A.kind == 0 ? imp[e] * unc : (A.kind == 1 ? imp[e] : unc);
          const float a = a0 > 1.f ? 1.f : a0;                       // an entropy of 1 + 1 ulp must not push the key below 0
          const bool excluded = exc && e < cnt && exc[e] != 0;       // e >= cnt: never stored
          const bool cand = ctr[e] != WN_DEAD && !excluded && a0 > 0.f && __builtin_isfinite(a0);
          sc[e] = cand ? a : 0.f;
          key[e] = cand ? 1.0f - a : -1.0f;
        }
        float* sc_img = reinterpret_cast<float*>(A.out) + (size_t)img_i * HW;
        float* key_img = A.out2 + (size_t)img_i * HW;
        wn_store<SEG>(sc_img + p, sc, cnt, (w & 3) == 0 && (reinterpret_cast<uintptr_t>(sc_img) & 15) == 0);
        wn_store<SEG>(key_img + p, key, cnt, (w & 3) == 0 && (reinterpret_cast<uintptr_t>(key_img) & 15) == 0);
      }
    }
  }
  if (PRODUCT == WN_MODE && A.counts) BlockCounts<3>::add(bcnt, ev, A.counts + (size_t)img_i * 3);   // uniform over the block
}

// ------------------------------------------------------------------------------------------------ scores -> labels and entropy
// The winner (first_max: THE tie rule) and the normalised entropy of every row, udaseg_entropy_loss's definition: with logits
// lp_c = (z_c - max) - log sum exp(z - max), p_c = exp(lp_c); with probs p_c as it is and lp_c = log p_c; H = sum over c, ascending,
// of -(s * (p_c * lp_c)) where p_c > 0, s = 1 / log(classes).  No contraction: the mirror rounds every product and sum.
template <int NV>
__global__ __launch_bounds__(256) void acquire_prepare_kernel(const float* __restrict__ scores, int ldc, int classes, int probs,
                                                              int64_t pixels, float s, uint8_t* __restrict__ labels,
                                                              float* __restrict__ entropy, unsigned long long* __restrict__ counters) {
#pragma clang fp contract(off)
  __shared__ BlockCounts<2>::Slots cnt;
  unsigned int ev[2] = {0, 0};                                       // finite, not finite
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < pixels; p += (int64_t)gridDim.x * 256) {
    f32x4 v[NV];
    load_row<NV>(scores + p * ldc, v);
    float m;
    const int am = first_max<NV>(v, classes, m);
    bool fin = true;
    float sum = 0.f;
#pragma unroll
    for (int q = 0; q < NV; ++q)
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (4 * q + e < classes) {
          fin &= __builtin_isfinite(v[q][e]);
          if (!probs) sum += expf(v[q][e] - m);
        }
    const float lg = probs ? 0.f : logf(sum);
    float hsum = 0.f;
#pragma unroll
    for (int q = 0; q < NV; ++q)
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (4 * q + e < classes) {
          const float x = v[q][e];
          const float lp = probs ? logf(x) : (x - m) - lg;
          const float pr = probs ? x : expf(lp);
          hsum += pr > 0.f ? -(s * (pr * lp)) : 0.f;
        }
    fin = fin && __builtin_isfinite(hsum);
    labels[p] = fin ? (uint8_t)am : (uint8_t)255;
    entropy[p] = fin ? hsum : 0.f;
    ev[0] += fin;
    ev[1] += !fin;
  }
  BlockCounts<2>::add(cnt, ev, counters);
}

// ------------------------------------------------------------------------------------------------------ cells, select, expand
// One wave per grid cell: lane l takes the cell's pixels l, l + 64, ... in the cell's raster order and the 64 partial sums fold in
// wave_sum_d's fixed order; float64, so the mean is the correctly rounded quotient of a sum that is exact to far below fp32.
__global__ __launch_bounds__(256) void acquire_cells_kernel(const float* __restrict__ key, int n, int h, int w, int cell_h, int cell_w,
                                                            int gh, int gw, float* __restrict__ cell_key) {
  const int lane = threadIdx.x & 63;
  const int64_t cells = (int64_t)n * gh * gw;
  for (int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); c < cells; c += (int64_t)gridDim.x * 4) {
    const int cx = (int)(c % gw), cy = (int)((c / gw) % gh), i = (int)(c / ((int64_t)gw * gh));
    const int y0 = cy * cell_h, x0 = cx * cell_w;
    const int ch = h - y0 < cell_h ? h - y0 : cell_h, cw = w - x0 < cell_w ? w - x0 : cell_w;
    const int64_t count = (int64_t)ch * cw;
    const float* src = key + (size_t)i * h * w;
    double s = 0.0;
    unsigned int cand = 0;
    for (int64_t j = lane; j < count; j += 64) {
      const int yy = (int)(j / cw), xx = (int)(j - (int64_t)yy * cw);
      const float k = src[(int64_t)(y0 + yy) * w + x0 + xx];
      if (k >= 0.f) {
        s += (double)(1.0f - k);
        ++cand;
      }
    }
    s = wave_sum_d(s);
    cand = wave_sum_u32(cand);
    if (lane == 0) cell_key[c] = cand ? 1.0f - (float)(s / (double)count) : -1.0f;
  }
}

__global__ __launch_bounds__(256) void acquire_select_kernel(const float* __restrict__ key, const float* __restrict__ thresholds,
                                                             int64_t items, uint8_t* __restrict__ mask,
                                                             unsigned long long* __restrict__ counts) {
  __shared__ BlockCounts<2>::Slots cnt;
  const int i = blockIdx.y;
  const float thr = thresholds[i];
  const float* k = key + (size_t)i * items;
  uint8_t* m = mask + (size_t)i * items;
  unsigned int ev[2] = {0, 0};                                       // new, candidates
  for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < items; j += (int64_t)gridDim.x * 256) {
    const float v = k[j];
    if (v >= 0.f) {
      ++ev[1];
      if (v <= thr) {
        if (m[j] == 0) ++ev[0];
        m[j] |= 1;
      }
    }
  }
  if (counts) BlockCounts<2>::add(cnt, ev, counts + (size_t)i * 2);
}

__global__ __launch_bounds__(256) void acquire_expand_kernel(const uint8_t* __restrict__ cell_mask, int h, int w, int cell_h, int cell_w,
                                                             int gh, int gw, uint8_t* __restrict__ mask) {
  const int i = blockIdx.y;
  const int64_t HW = (int64_t)h * w;
  const uint8_t* cm = cell_mask + (size_t)i * gh * gw;
  uint8_t* m = mask + (size_t)i * HW;
  for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < HW; j += (int64_t)gridDim.x * 256) {
    const int y = (int)(j / w), x = (int)(j - (int64_t)y * w);
    if (cm[(y / cell_h) * gw + x / cell_w]) m[j] |= 1;
  }
}

// the argument rules the window entry points share; 0 or UDASEG_E_BADARG with the message set
static int wn_check(const char* who, int labels_i64, int n, int h, int w, int radius, int classes, int has_ignore, int ignore_index) {
  if (int rc = map_storage_ok(who, "labels_i64", labels_i64)) return rc;
  if (int rc = map_extent_ok(who, n, h, w)) return rc;
  UDASEG_CHECK_ARG(radius >= 0 && radius <= WN_MAX_R, "%s: need 0 <= radius <= %d (radius=%d)", who, WN_MAX_R, radius);
  UDASEG_CHECK_ARG(classes >= 2 && classes <= 32, "%s: need 2 <= classes <= 32 (classes=%d)", who, classes);
  return map_ignore_ok(who, has_ignore, ignore_index);
}

template <int PRODUCT>
static int wn_launch(const char* who, WnArgs& A, int labels_i64, int n, hipStream_t st) {
  const WnGeom& G = A.G;
  const int64_t tiles = (int64_t)G.tiles_x * cdiv(G.h, G.th);
  const dim3 grid((unsigned int)tiles, (unsigned int)n), block(WN_THREADS);
  // the largest block (the score product at radius 8: 45 KB) is below the 48 KB a kernel may take without opting in
  if (G.lds > 48 * 1024) {
    set_error("%s: internal: %d bytes of LDS", who, G.lds);
    return UDASEG_E_UNSUPPORTED;
  }
  dispatch_flags(
      [&](auto i64, auto tall) {
        hipLaunchKernelGGL((window_kernel<decltype(i64)::value, decltype(tall)::value ? 32 : 16, PRODUCT>), grid, block, G.lds, st, A);
      },
      labels_i64 != 0, G.th == 32);
  UDASEG_LAUNCH_CHECK(who);
  return UDASEG_OK;
}

}  // namespace udaseg

using namespace udaseg;

extern "C" int udaseg_window_tile(int radius) {
  UDASEG_CHECK_ARG(radius >= 0 && radius <= WN_MAX_R, "window_tile: need 0 <= radius <= %d (radius=%d)", WN_MAX_R, radius);
  return (wn_tile_h(radius) << 16) | WN_TW;
}

extern "C" int udaseg_window_mode(const void* labels, int labels_i64, int n, int h, int w, int radius, int classes, int has_ignore,
                                  int ignore_index, int fill_void, int void_label, uint8_t* out, float* agreement, int64_t* counts,
                                  void* stream) {
  if (int rc = wn_check("window_mode", labels_i64, n, h, w, radius, classes, has_ignore, ignore_index)) return rc;
  UDASEG_CHECK_ARG(fill_void == 0 || fill_void == 1, "window_mode: fill_void must be 0 or 1, got %d", fill_void);
  UDASEG_CHECK_ARG(void_label >= 0 && void_label <= 255, "window_mode: void_label must lie in [0, 255] (void_label=%d)", void_label);
  UDASEG_CHECK_ARG(labels && out, "window_mode: NULL pointer (labels and out are required)");
  if (int rc = map_aligned_ok("window_mode", "labels", labels_i64, labels)) return rc;
  UDASEG_CHECK_ARG((reinterpret_cast<uintptr_t>(agreement) & 3) == 0 && (reinterpret_cast<uintptr_t>(counts) & 7) == 0,
                   "window_mode: agreement must be 4-byte and counts 8-byte aligned");
  WnArgs A = {};
  A.labels = labels;
  A.out = out;
  A.out2 = agreement;
  A.counts = reinterpret_cast<unsigned long long*>(counts);
  A.fill_void = fill_void;
  A.void_label = void_label;
  A.G = wn_geom(h, w, radius, classes, has_ignore, ignore_index, WN_MODE);
  return wn_launch<WN_MODE>("window_mode launch", A, labels_i64, n, as_stream(stream));
}

extern "C" int udaseg_window_impurity(const void* labels, int labels_i64, int n, int h, int w, int radius, int classes, int has_ignore,
                                      int ignore_index, const float* table, float* out, void* stream) {
  if (int rc = wn_check("window_impurity", labels_i64, n, h, w, radius, classes, has_ignore, ignore_index)) return rc;
  UDASEG_CHECK_ARG(labels && table && out, "window_impurity: NULL pointer (labels, table and out are required)");
  if (int rc = map_aligned_ok("window_impurity", "labels", labels_i64, labels)) return rc;
  UDASEG_CHECK_ARG(((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(table)) & 3) == 0,
                   "window_impurity: table and out must be 4-byte aligned");
  WnArgs A = {};
  A.labels = labels;
  A.table = table;
  A.out = out;
  A.log_classes = (float)log((double)classes);
  A.G = wn_geom(h, w, radius, classes, has_ignore, ignore_index, WN_IMPURITY);
  return wn_launch<WN_IMPURITY>("window_impurity launch", A, labels_i64, n, as_stream(stream));
}

extern "C" int udaseg_acquire_prepare(const float* scores, int ldc, int classes, int probs, int64_t pixels, uint8_t* labels,
                                      float* entropy, int64_t* counters, void* stream) {
  if (!scores_args_ok("acquire_prepare", pixels, classes, ldc)) return UDASEG_E_BADARG;
  UDASEG_CHECK_ARG(classes >= 2, "acquire_prepare: need classes >= 2 (1 / log(classes) scales the entropy; classes=%d)", classes);
  UDASEG_CHECK_ARG(probs == 0 || probs == 1, "acquire_prepare: probs must be 0 or 1, got %d", probs);
  UDASEG_CHECK_ARG(scores && labels && entropy && counters, "acquire_prepare: NULL pointer");
  UDASEG_CHECK_ARG((reinterpret_cast<uintptr_t>(scores) & 15) == 0 && (reinterpret_cast<uintptr_t>(entropy) & 3) == 0 &&
                       (reinterpret_cast<uintptr_t>(counters) & 7) == 0,
                   "acquire_prepare: scores must be 16-byte, entropy 4-byte and counters 8-byte aligned");
  const int grid = capped_grid(pixels, 256, 4096);
  const float s = 1.f / logf((float)classes);
  if (!dispatch_width<8>((classes + 3) / 4, [&](auto wd) {
        constexpr int NV = decltype(wd)::value;
        hipLaunchKernelGGL(acquire_prepare_kernel<NV>, dim3(grid), dim3(256), 0, as_stream(stream), scores, ldc, classes, probs, pixels,
                           s, labels, entropy, reinterpret_cast<unsigned long long*>(counters));
      }))
    return unsupported_width("acquire_prepare", "classes", classes);
  UDASEG_LAUNCH_CHECK("acquire_prepare launch");
  return UDASEG_OK;
}

extern "C" int udaseg_acquire_score(const uint8_t* labels, const float* entropy, const uint8_t* exclude, int n, int h, int w, int radius,
                                    int classes, int kind, const float* table, float* score, float* key, void* stream) {
  if (int rc = wn_check("acquire_score", 0, n, h, w, radius, classes, 0, 0)) return rc;
  UDASEG_CHECK_ARG(kind >= 0 && kind <= 2, "acquire_score: kind must be 0 (RIPU), 1 (impurity) or 2 (uncertainty), got %d", kind);
  UDASEG_CHECK_ARG(labels && entropy && table && score && key, "acquire_score: NULL pointer (only exclude may be NULL)");
  UDASEG_CHECK_ARG(((reinterpret_cast<uintptr_t>(entropy) | reinterpret_cast<uintptr_t>(table) | reinterpret_cast<uintptr_t>(score) |
                     reinterpret_cast<uintptr_t>(key)) & 3) == 0,
                   "acquire_score: entropy, table, score and key must be 4-byte aligned");
  WnArgs A = {};
  A.labels = labels;
  A.entropy = entropy;
  A.exclude = exclude;
  A.table = table;
  A.out = score;
  A.out2 = key;
  A.kind = kind;
  A.log_classes = (float)log((double)classes);
  A.G = wn_geom(h, w, radius, classes, 0, 0, WN_SCORE);
  return wn_launch<WN_SCORE>("acquire_score launch", A, 0, n, as_stream(stream));
}

extern "C" int udaseg_acquire_cells(const float* key, int n, int h, int w, int cell_h, int cell_w, float* cell_key, void* stream) {
  if (int rc = map_extent_ok("acquire_cells", n, h, w)) return rc;
  UDASEG_CHECK_ARG(cell_h >= 1 && cell_w >= 1, "acquire_cells: need cell_h, cell_w >= 1 (cell_h=%d cell_w=%d)", cell_h, cell_w);
  UDASEG_CHECK_ARG(key && cell_key, "acquire_cells: NULL pointer");
  UDASEG_CHECK_ARG(((reinterpret_cast<uintptr_t>(key) | reinterpret_cast<uintptr_t>(cell_key)) & 3) == 0,
                   "acquire_cells: key and cell_key must be 4-byte aligned");
  const int gh = cdiv(h, cell_h), gw = cdiv(w, cell_w);
  const int grid = capped_grid((int64_t)n * gh * gw, 4, 65536);
  hipLaunchKernelGGL(acquire_cells_kernel, dim3(grid), dim3(256), 0, as_stream(stream), key, n, h, w, cell_h, cell_w, gh, gw, cell_key);
  UDASEG_LAUNCH_CHECK("acquire_cells launch");
  return UDASEG_OK;
}

extern "C" int udaseg_acquire_select(const float* key, const float* thresholds, int n, int64_t items_per_image, uint8_t* mask,
                                     int64_t* counts, void* stream) {
  if (int rc = map_batch_ok("acquire_select", n)) return rc;
  UDASEG_CHECK_ARG(items_per_image > 0 && items_per_image < ((int64_t)1 << 31),
                   "acquire_select: need 0 < items_per_image < 2^31 (items_per_image=%lld)", (long long)items_per_image);
  UDASEG_CHECK_ARG(key && thresholds && mask, "acquire_select: NULL pointer (key, thresholds and mask are required)");
  UDASEG_CHECK_ARG(((reinterpret_cast<uintptr_t>(key) | reinterpret_cast<uintptr_t>(thresholds)) & 3) == 0 &&
                       (reinterpret_cast<uintptr_t>(counts) & 7) == 0,
                   "acquire_select: key and thresholds must be 4-byte and counts 8-byte aligned");
  const int grid = capped_grid(items_per_image, 256 * 4, 1024);
  hipLaunchKernelGGL(acquire_select_kernel, dim3(grid, n), dim3(256), 0, as_stream(stream), key, thresholds, items_per_image, mask,
                     reinterpret_cast<unsigned long long*>(counts));
  UDASEG_LAUNCH_CHECK("acquire_select launch");
  return UDASEG_OK;
}

extern "C" int udaseg_acquire_expand(const uint8_t* cell_mask, int n, int h, int w, int cell_h, int cell_w, uint8_t* mask,
                                     void* stream) {
  if (int rc = map_extent_ok("acquire_expand", n, h, w)) return rc;
  UDASEG_CHECK_ARG(cell_h >= 1 && cell_w >= 1, "acquire_expand: need cell_h, cell_w >= 1 (cell_h=%d cell_w=%d)", cell_h, cell_w);
  UDASEG_CHECK_ARG(cell_mask && mask, "acquire_expand: NULL pointer");
  const int gh = cdiv(h, cell_h), gw = cdiv(w, cell_w);
  const int grid = capped_grid((int64_t)h * w, 256 * 4, 1024);
  hipLaunchKernelGGL(acquire_expand_kernel, dim3(grid, n), dim3(256), 0, as_stream(stream), cell_mask, h, w, cell_h, cell_w, gh, gw, mask);
  UDASEG_LAUNCH_CHECK("acquire_expand launch");
  return UDASEG_OK;
}
