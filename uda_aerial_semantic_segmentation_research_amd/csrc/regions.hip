// Connected components of label maps on the device: the id and the area of every pixel's region, a sieve that voids the regions
// below a minimum area per class, and per-class region statistics.
//
// The rule (include/udaseg.h states it in full; tests/_regions_ref.py is its numpy mirror, compared for equality).  Per image:
//   L(p)     the label: uint8, or int64 with a value outside [0, 255] read as 255; void when has_ignore and L(p) == ignore_index
//            (udaseg_regions_label_i32: an int32 map, every value >= 0 a label of its own, void when negative)
//   adjacent two pixels of one image, neither void, with the same label, that are 4- or 8-neighbours (connectivity)
//   id(p)    the smallest y * w + x over the pixels of p's component (the transitive closure of "adjacent"); -1 on a void pixel
//   area(p)  the number of pixels of p's component; 0 on a void pixel
//
// Shape: a hierarchical union-find whose forest lives in ids itself, parent[p] = ids[p] <= p at every moment (a union only ever
// lowers a root's parent with atomicMin), so every chain ends at the smallest index of its tree and every loop over a chain ends.
//   1. tile     a block labels one 64 x 64 tile in LDS and writes the GLOBAL index of every pixel's tile-local root; the size of a
//               tile-local component goes to the root's slot of area, 0 to every other slot.
//   2. merge    level k = 1 .. K: a block owns a group of 2^k x 2^k tiles of one image (edge groups hold fewer) and unites the pairs
//               across the two seams through the group's middle, the only seams inside the group no lower level has seen.  Both
//               pixels of every pair, and therefore every root a chain from them can reach, lie inside the group: a block reads
//               and writes ids of its own group only.  K = ceil(log2(max tiles per side)); the last launch has one block per image.
//   3. resolve  per pixel r = find(p).  Only tile-roots (pixels that pointed to themselves after step 1) were ever relinked, and a
//               chain runs through tile-roots only.  So this launch READS tile-root words of ids and WRITES ids[p] = r only for the
//               other pixels.  A tile-root that is no root any more adds its tile-local size to area[r] (one atomic per
//               tile-component, not per pixel) and leaves ~r in its own area slot, which nobody else reads.
//   4. finish   tile-roots take their id from that slot; with want_area every pixel takes area[id(p)]: the roots' slots are only
//               read, every other slot is written by its own thread.
// No block reads a word that another block of the same launch writes; the hand-off between blocks is the launch boundary.  Within
// a block unions are atomicMin and every find reads ids with a relaxed agent-scope atomic load (L2-served, never a stale L1 line).
// There are no flags, spin-waits or inter-block counters.  The ids are unique, so two runs give the same bits in any order.
#include "label_maps.h"

namespace udaseg {

constexpr int RG_THREADS = 256;
static_assert(RG_THREADS == 64 * 4, "BlockCounts<K>: four waves a block");
constexpr int RG_TH = 64, RG_TW = 64;          // tile: 4096 pixels, 16 per thread; a wave owns one tile row per trip
constexpr int RG_TILE = RG_TH * RG_TW;
constexpr int RG_DEAD = 0x100;                 // a void pixel or a position outside the image
constexpr int RG_STAT_COLS = 34;               // components, pixels, hist[32]

struct RgArgs {
  const void* labels;
  int* ids;
  int* area;
  int h, w, tiles_x, tiles_y;
  int conn8, has_ignore, ignore_index;
  int level, groups_x;                         // merge
  int want_area;                               // finish
};

// the label kinds: uint8, int64 (a value outside [0, 255] reads as 255) and int32 (any value >= 0 is a label, a negative one void)
constexpr int RG_U8 = 0, RG_I64 = 1, RG_I32 = 2;
template <int KIND>
constexpr int rg_dead() { return KIND == RG_I32 ? -1 : RG_DEAD; }
template <int KIND>
constexpr size_t rg_bytes() { return KIND == RG_I64 ? 8 : KIND == RG_I32 ? 4 : 1; }

template <int KIND>
__device__ __forceinline__ int rg_load(const void* __restrict__ img, int64_t p, int has_ignore, int ignore_index) {
  if (KIND == RG_I32) {
    const int v = reinterpret_cast<const int*>(img)[p];
    return v < 0 ? -1 : v;
  }
  const int v = label_at<KIND == RG_I64>(img, p);
  return (has_ignore && v == ignore_index) ? RG_DEAD : v;
}

// ---- the forest in LDS (tile pass).  par[i] <= i always.
__device__ __forceinline__ int rg_find_lds(const int* par, int x) {
  for (;;) {                                   // ends: par[x] <= x, so x strictly decreases until par[x] == x
    const int p = __hip_atomic_load(par + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (p >= x) return x;
    x = p;
  }
}

__device__ __forceinline__ void rg_unite_lds(int* par, int a, int b) {
  for (;;) {                                   // ends: a + b strictly decreases on every trip that does not return
    a = rg_find_lds(par, a);
    b = rg_find_lds(par, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = atomicMin(par + a, b);     // a was a root when read; old < a: another thread has linked it meanwhile
    if (old >= a) return;                      // old == a: linked here (old > a cannot be)
    a = old;
  }
}

// ---- the forest in ids (merge levels, resolve).  ids[x] <= x always; x is never void.
__device__ __forceinline__ int rg_find(int* ids, int x) {
  for (;;) {                                   // ends: ids[x] <= x, so x strictly decreases until ids[x] == x
    const int p = __hip_atomic_load(ids + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (p >= x || p < 0) return x;             // p == x at a root; the other two cannot be and would leave the image
    x = p;
  }
}

__device__ __forceinline__ void rg_unite(int* ids, int a, int b) {
  for (;;) {                                   // ends: a + b strictly decreases on every trip that does not return
    a = rg_find(ids, a);
    b = rg_find(ids, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = atomicMin(ids + a, b);
    if (old >= a) return;                      // old == a: linked here (old > a cannot be)
    a = old;
  }
}

// the tile's labels in LDS: 16 bits hold a uint8 / int64 label or RG_DEAD; an int32 label takes the word (48 KB of LDS in all)
template <int KIND>
struct RgLab { typedef unsigned short type; };
template <>
struct RgLab<RG_I32> { typedef int type; };

template <int KIND>
__global__ __launch_bounds__(RG_THREADS) void regions_tile_kernel(RgArgs A) {
  typedef typename RgLab<KIND>::type lab_t;
  constexpr int RG_DEAD = rg_dead<KIND>();     // shadows the 16-bit kinds' constant inside this kernel
  __shared__ int par[RG_TILE];
  __shared__ unsigned int cnt[RG_TILE];
  __shared__ lab_t lab[RG_TILE];
  const int tid = threadIdx.x, h = A.h, w = A.w;
  const int ty0 = ((int)blockIdx.x / A.tiles_x) * RG_TH, tx0 = ((int)blockIdx.x % A.tiles_x) * RG_TW;
  const int64_t HW = (int64_t)h * w;
  const uint8_t* img = reinterpret_cast<const uint8_t*>(A.labels) + (size_t)blockIdx.y * HW * rg_bytes<KIND>();
  int* ids = A.ids + (size_t)blockIdx.y * HW;
  int* area = A.area + (size_t)blockIdx.y * HW;
  for (int i = tid; i < RG_TILE; i += RG_THREADS) {
    const int y = ty0 + (i >> 6), x = tx0 + (i & 63);
    int v = RG_DEAD;
    if (y < h && x < w) v = rg_load<KIND>(img, (int64_t)y * w + x, A.has_ignore, A.ignore_index);   // every read is inside the image
    lab[i] = (lab_t)v;
    // a wave holds one tile row (RG_TW == 64 lanes): every pixel starts at the first pixel of its horizontal run, so the row
    // needs no union at all.  Lane 0 always starts a run, so the mask below is never empty.
    const int lane = tid & 63;
    const int left = __shfl_up(v, 1, 64);
    const unsigned long long starts = __ballot(lane == 0 || v == RG_DEAD || left != v);
    par[i] = (i & ~63) + 63 - __clzll((long long)(starts & (~0ull >> (63 - lane))));
    cnt[i] = 0;
  }
  __syncthreads();
  // Runs of neighbouring rows are joined once per contact, not once per pixel.  A pixel under its own label unites upwards only
  // where its run starts or the label up-left differs: otherwise its left neighbour lies under the same upper run, and by
  // induction along the run is joined to it already.  A diagonal matters only under a differing label, and only where the left
  // (right) neighbour, which has that diagonal pixel straight above it, is not of the run.
  for (int i = tid; i < RG_TILE; i += RG_THREADS) {
    const int l = lab[i];
    if (l == RG_DEAD || i < RG_TW) continue;
    const int lx = i & 63;
    const bool run_start = lx == 0 || lab[i - 1] != l;
    if (lab[i - RG_TW] == l) {
      if (run_start || lab[i - RG_TW - 1] != l) rg_unite_lds(par, i, i - RG_TW);
    } else if (A.conn8) {
      if (lx > 0 && run_start && lab[i - RG_TW - 1] == l) rg_unite_lds(par, i, i - RG_TW - 1);
      if (lx < RG_TW - 1 && lab[i + 1] != l && lab[i - RG_TW + 1] == l) rg_unite_lds(par, i, i - RG_TW + 1);
    }
  }
  __syncthreads();
  int root[RG_TILE / RG_THREADS];
#pragma unroll
  for (int k = 0; k < RG_TILE / RG_THREADS; ++k) {
    const int i = tid + k * RG_THREADS;
    root[k] = lab[i] == RG_DEAD ? -1 : rg_find_lds(par, i);
  }
  // sizes: the lanes that share lane 0's root (a whole tile row inside one region, mostly) add once for all of them
#pragma unroll
  for (int k = 0; k < RG_TILE / RG_THREADS; ++k) {
    const int r = root[k];
    const int r0 = __shfl(r, 0, 64);
    const bool same = r >= 0 && r == r0;
    const unsigned long long m = __ballot(same);
    if (same) {
      if ((tid & 63) == __ffsll((long long)m) - 1) atomicAdd(&cnt[r], (unsigned int)__popcll(m));
    } else if (r >= 0) {
      atomicAdd(&cnt[r], 1u);
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < RG_TILE / RG_THREADS; ++k) {
    const int i = tid + k * RG_THREADS;
    const int y = ty0 + (i >> 6), x = tx0 + (i & 63);
    if (y >= h || x >= w) continue;
    const int64_t p = (int64_t)y * w + x;
    const int r = root[k];
    ids[p] = r < 0 ? -1 : (ty0 + (r >> 6)) * w + tx0 + (r & 63);   // < h * w < 2^31; the local order is the raster order
    area[p] = r == i ? (int)cnt[i] : 0;
  }
}

template <int KIND>
__global__ __launch_bounds__(RG_THREADS) void regions_merge_kernel(RgArgs A) {
  constexpr int RG_DEAD = rg_dead<KIND>();
  const int tid = threadIdx.x, h = A.h, w = A.w, k = A.level;
  const int64_t HW = (int64_t)h * w;
  const uint8_t* img = reinterpret_cast<const uint8_t*>(A.labels) + (size_t)blockIdx.y * HW * rg_bytes<KIND>();
  int* ids = A.ids + (size_t)blockIdx.y * HW;
  // the group's pixels: [gy0, gy1) x [gx0, gx1), clipped to the image (64-bit: 64 << k passes 2^31 for a one-row image)
  const int64_t gy0 = (int64_t)((int)blockIdx.x / A.groups_x) * ((int64_t)RG_TH << k);
  const int64_t gx0 = (int64_t)((int)blockIdx.x % A.groups_x) * ((int64_t)RG_TW << k);
  const int64_t gy1 = gy0 + ((int64_t)RG_TH << k) < h ? gy0 + ((int64_t)RG_TH << k) : h;
  const int64_t gx1 = gx0 + ((int64_t)RG_TW << k) < w ? gx0 + ((int64_t)RG_TW << k) : w;
  const int64_t ys = gy0 + ((int64_t)RG_TH << (k - 1)), xs = gx0 + ((int64_t)RG_TW << (k - 1));
  const int reach = A.conn8 ? 1 : 0;
  if (xs < gx1) {                              // the vertical seam between columns xs - 1 and xs, over the group's rows
    for (int64_t y = gy0 + tid; y < gy1; y += RG_THREADS) {
      const int64_t a = y * w + xs - 1;
      const int l = rg_load<KIND>(img, a, A.has_ignore, A.ignore_index);
      if (l == RG_DEAD) continue;
      for (int d = -reach; d <= reach; ++d) {  // a diagonal that leaves the group belongs to the level whose group holds both
        const int64_t yb = y + d;
        if (yb < gy0 || yb >= gy1) continue;
        const int64_t b = yb * w + xs;
        if (rg_load<KIND>(img, b, A.has_ignore, A.ignore_index) == l) rg_unite(ids, (int)a, (int)b);
      }
    }
  }
  if (ys < gy1) {                              // the horizontal seam between rows ys - 1 and ys, over the group's columns
    for (int64_t x = gx0 + tid; x < gx1; x += RG_THREADS) {
      const int64_t a = (ys - 1) * w + x;
      const int l = rg_load<KIND>(img, a, A.has_ignore, A.ignore_index);
      if (l == RG_DEAD) continue;
      for (int d = -reach; d <= reach; ++d) {
        const int64_t xb = x + d;
        if (xb < gx0 || xb >= gx1) continue;
        const int64_t b = ys * w + xb;
        if (rg_load<KIND>(img, b, A.has_ignore, A.ignore_index) == l) rg_unite(ids, (int)a, (int)b);
      }
    }
  }
}

__global__ __launch_bounds__(RG_THREADS) void regions_resolve_kernel(RgArgs A) {
  const int64_t HW = (int64_t)A.h * A.w;
  int* ids = A.ids + (size_t)blockIdx.y * HW;
  int* area = A.area + (size_t)blockIdx.y * HW;
  for (int64_t p = (int64_t)blockIdx.x * RG_THREADS + threadIdx.x; p < HW; p += (int64_t)gridDim.x * RG_THREADS) {
    const int v = ids[p];                      // a tile-root's word is written by nobody in this launch, another by this thread only
    if (v < 0 || v == (int)p) continue;        // void, or a root of the whole image: its id stands, its area slot takes the adds
    const int a = area[p];                     // > 0: a tile-root (the tile pass left its size here); the adds go to roots only
    const int r = rg_find(ids, v);             // reads tile-root words only
    if (a == 0) {
      ids[p] = r;
    } else {                                   // a tile-root that has been linked away: hand its size to the root
      atomicAdd(area + r, a);
      area[p] = ~r;
    }
  }
}

__global__ __launch_bounds__(RG_THREADS) void regions_finish_kernel(RgArgs A) {
  const int64_t HW = (int64_t)A.h * A.w;
  int* ids = A.ids + (size_t)blockIdx.y * HW;
  int* area = A.area + (size_t)blockIdx.y * HW;
  for (int64_t p = (int64_t)blockIdx.x * RG_THREADS + threadIdx.x; p < HW; p += (int64_t)gridDim.x * RG_THREADS) {
    const int a = area[p];                     // > 0 only in a root's slot, which no thread writes in this launch
    int r = ids[p];
    if (a < 0) {
      r = ~a;
      ids[p] = r;
    }
    if (A.want_area && r >= 0 && r != (int)p) area[p] = area[r];
  }
}

// ---- sieve and statistics: one pass over the labels, ids and per-pixel areas
struct RgScanArgs {
  const void* labels;
  const int* ids;
  const int* area;
  int h, w, has_ignore, ignore_index;
  const int* min_area;                         // sieve
  int void_label;
  uint8_t* out;
  unsigned long long* counts;                  // sieve: [n][3]
  unsigned long long* stats;                   // stats: [classes][34]
  int classes;
};

template <bool I64>
__global__ __launch_bounds__(RG_THREADS) void regions_sieve_kernel(RgScanArgs A) {
  __shared__ int min_area[256];
  __shared__ BlockCounts<3>::Slots cnt;
  const int tid = threadIdx.x;
  const int64_t HW = (int64_t)A.h * A.w;
  const uint8_t* img = reinterpret_cast<const uint8_t*>(A.labels) + (size_t)blockIdx.y * HW * (I64 ? 8 : 1);
  const int* ids = A.ids + (size_t)blockIdx.y * HW;
  const int* area = A.area + (size_t)blockIdx.y * HW;
  uint8_t* out = A.out + (size_t)blockIdx.y * HW;
  min_area[tid] = A.min_area[tid];             // RG_THREADS == 256 entries
  __syncthreads();
  unsigned int ev[3] = {0, 0, 0};              // voided pixels, removed components, kept components
  for (int64_t p = (int64_t)blockIdx.x * RG_THREADS + tid; p < HW; p += (int64_t)gridDim.x * RG_THREADS) {
    const int l = rg_load<I64>(img, p, 0, 0);
    int o = l;
    if (!(A.has_ignore && l == A.ignore_index)) {
      const bool small = area[p] < min_area[l];
      const bool root = ids[p] == (int)p;
      if (small) {
        o = A.void_label;
        ++ev[0];
      }
      ev[1] += root && small;
      ev[2] += root && !small;
    }
    out[p] = (uint8_t)o;
  }
  // a block sees fewer than 2^32 pixels: gridDim.x covers HW < 2^31 of them
  if (A.counts) BlockCounts<3>::add(cnt, ev, A.counts + (size_t)blockIdx.y * 3);
}

template <bool I64>
__global__ __launch_bounds__(RG_THREADS) void regions_stats_kernel(RgScanArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char rg_lds[];
  unsigned long long* pix = reinterpret_cast<unsigned long long*>(rg_lds);        // [classes]: areas add up past 2^32
  unsigned int* cnt = reinterpret_cast<unsigned int*>(pix + A.classes);           // [classes][33]: components, hist[32]
  const int tid = threadIdx.x, classes = A.classes;
  const int64_t HW = (int64_t)A.h * A.w;
  const uint8_t* img = reinterpret_cast<const uint8_t*>(A.labels) + (size_t)blockIdx.y * HW * (I64 ? 8 : 1);
  const int* ids = A.ids + (size_t)blockIdx.y * HW;
  const int* area = A.area + (size_t)blockIdx.y * HW;
  for (int i = tid; i < classes; i += RG_THREADS) pix[i] = 0;
  for (int i = tid; i < classes * 33; i += RG_THREADS) cnt[i] = 0;
  __syncthreads();
  for (int64_t p = (int64_t)blockIdx.x * RG_THREADS + tid; p < HW; p += (int64_t)gridDim.x * RG_THREADS) {
    if (ids[p] != (int)p) continue;            // a component counts at its root pixel; a void pixel has id -1
    const int l = rg_load<I64>(img, p, 0, 0);
    const int a = area[p];
    if (l >= classes || a < 1) continue;
    atomicAdd(&cnt[l * 33], 1u);
    atomicAdd(&cnt[l * 33 + 1 + (31 - __clz(a))], 1u);
    atomicAdd(&pix[l], (unsigned long long)a);
  }
  __syncthreads();
  for (int i = tid; i < classes * RG_STAT_COLS; i += RG_THREADS) {
    const int c = i / RG_STAT_COLS, j = i - c * RG_STAT_COLS;
    const unsigned long long v = j == 1 ? pix[c] : (unsigned long long)cnt[c * 33 + (j == 0 ? 0 : j - 1)];
    if (v) atomicAdd(&A.stats[i], v);
  }
}

// the argument rules every entry point shares; 0 or UDASEG_E_BADARG with the message set
static int rg_check(const char* who, int labels_i64, int n, int h, int w, int has_ignore, int ignore_index) {
  if (int rc = map_storage_ok(who, "labels_i64", labels_i64)) return rc;
  if (int rc = map_extent_ok(who, n, h, w)) return rc;
  return map_ignore_ok(who, has_ignore, ignore_index);
}

// blocks of a flat per-pixel pass over one image: 8 pixels per thread, at most 1024 blocks (the kernels walk the rest)
static inline unsigned int rg_flat_grid(int64_t hw) { return (unsigned int)capped_grid(hw, RG_THREADS * 8, 1024); }

#define RG_LAUNCHED(what)                                   \
  do {                                                      \
    hipError_t e__ = hipGetLastError();                     \
    if (e__ != hipSuccess) return hip_fail(e__, what);      \
  } while (0)

static int rg_label(RgArgs A, int kind, int n, hipStream_t st) {
  const int64_t hw = (int64_t)A.h * A.w;
  A.tiles_x = cdiv(A.w, RG_TW);
  A.tiles_y = cdiv(A.h, RG_TH);
  const dim3 tiles((unsigned int)((int64_t)A.tiles_x * A.tiles_y), (unsigned int)n);   // <= 2^31 / 4096 + the edge tiles
  if (kind == RG_I32) hipLaunchKernelGGL(regions_tile_kernel<RG_I32>, tiles, dim3(RG_THREADS), 0, st, A);
  else if (kind == RG_I64) hipLaunchKernelGGL(regions_tile_kernel<RG_I64>, tiles, dim3(RG_THREADS), 0, st, A);
  else hipLaunchKernelGGL(regions_tile_kernel<RG_U8>, tiles, dim3(RG_THREADS), 0, st, A);
  RG_LAUNCHED("regions_label tile launch");
  const int side = A.tiles_x > A.tiles_y ? A.tiles_x : A.tiles_y;
  for (int k = 1; (1 << (k - 1)) < side; ++k) {                                         // ceil(log2(side)) levels
    A.level = k;
    A.groups_x = cdiv(A.tiles_x, 1 << k);
    const dim3 groups((unsigned int)((int64_t)A.groups_x * cdiv(A.tiles_y, 1 << k)), (unsigned int)n);
    if (kind == RG_I32) hipLaunchKernelGGL(regions_merge_kernel<RG_I32>, groups, dim3(RG_THREADS), 0, st, A);
    else if (kind == RG_I64) hipLaunchKernelGGL(regions_merge_kernel<RG_I64>, groups, dim3(RG_THREADS), 0, st, A);
    else hipLaunchKernelGGL(regions_merge_kernel<RG_U8>, groups, dim3(RG_THREADS), 0, st, A);
    RG_LAUNCHED("regions_label merge launch");
  }
  const dim3 flat(rg_flat_grid(hw), (unsigned int)n);
  hipLaunchKernelGGL(regions_resolve_kernel, flat, dim3(RG_THREADS), 0, st, A);
  RG_LAUNCHED("regions_label resolve launch");
  hipLaunchKernelGGL(regions_finish_kernel, flat, dim3(RG_THREADS), 0, st, A);
  RG_LAUNCHED("regions_label finish launch");
  return UDASEG_OK;
}

// common.h: the 4-connected components of checked int32 maps (superpixels.hip's connect step labels its cluster map with it)
int regions_label_i32_launch(const int32_t* labels, int32_t* ids, int32_t* area, int n, int h, int w, int connectivity, int want_area,
                             hipStream_t st) {
  RgArgs A = {};
  A.labels = labels;
  A.ids = ids;
  A.area = area;
  A.h = h;
  A.w = w;
  A.conn8 = connectivity == 8;
  A.want_area = want_area;
  return rg_label(A, RG_I32, n, st);
}

}  // namespace udaseg

using namespace udaseg;

extern "C" int udaseg_regions_tile(void) { return (RG_TH << 16) | RG_TW; }

extern "C" int udaseg_regions_label(const void* labels, int labels_i64, int n, int h, int w, int connectivity, int has_ignore,
                                    int ignore_index, int32_t* ids, int32_t* area, void* stream) {
  if (int rc = rg_check("regions_label", labels_i64, n, h, w, has_ignore, ignore_index)) return rc;
  UDASEG_CHECK_ARG(connectivity == 4 || connectivity == 8, "regions_label: connectivity must be 4 or 8, got %d", connectivity);
  UDASEG_CHECK_ARG(labels && ids, "regions_label: NULL pointer (labels and ids are required)");
  UDASEG_CHECK_ARG(((reinterpret_cast<uintptr_t>(ids) | reinterpret_cast<uintptr_t>(area)) & 3) == 0,
                   "regions_label: ids and area must be 4-byte aligned");
  if (int rc = map_aligned_ok("regions_label", "labels", labels_i64, labels)) return rc;
  hipStream_t st = as_stream(stream);
  RgArgs A = {};
  A.labels = labels;
  A.ids = ids;
  A.area = area;
  A.h = h;
  A.w = w;
  A.conn8 = connectivity == 8;
  A.has_ignore = has_ignore;
  A.ignore_index = ignore_index;
  A.want_area = area != nullptr;
  if (area == nullptr) {                       // the tile sizes and the tile-roots' ids still need their [n][h][w] slots
    hipError_t e = hipMallocAsync(reinterpret_cast<void**>(&A.area), sizeof(int) * (size_t)n * h * w, st);
    if (e != hipSuccess) return hip_fail(e, "hipMallocAsync(regions_label)");
  }
  const int rc = rg_label(A, labels_i64, n, st);
  if (area == nullptr) {
    hipError_t e = hipFreeAsync(A.area, st);
    if (rc == UDASEG_OK && e != hipSuccess) return hip_fail(e, "hipFreeAsync(regions_label)");
  }
  return rc;
}

extern "C" int udaseg_regions_label_i32(const int32_t* labels, int n, int h, int w, int connectivity, int32_t* ids, int32_t* area,
                                        void* stream) {
  if (int rc = rg_check("regions_label_i32", 0, n, h, w, 0, 0)) return rc;
  UDASEG_CHECK_ARG(connectivity == 4 || connectivity == 8, "regions_label_i32: connectivity must be 4 or 8, got %d", connectivity);
  UDASEG_CHECK_ARG(labels && ids, "regions_label_i32: NULL pointer (labels and ids are required)");
  UDASEG_CHECK_ARG(((reinterpret_cast<uintptr_t>(labels) | reinterpret_cast<uintptr_t>(ids) | reinterpret_cast<uintptr_t>(area)) & 3) == 0,
                   "regions_label_i32: labels, ids and area must be 4-byte aligned");
  UDASEG_CHECK_ARG(static_cast<const void*>(labels) != static_cast<const void*>(ids),
                   "regions_label_i32: ids must not be labels itself (the seams are joined by reading labels after ids is written)");
  hipStream_t st = as_stream(stream);
  int32_t* scratch = nullptr;
  if (area == nullptr) {                       // the tile sizes and the tile-roots' ids still need their [n][h][w] slots
    hipError_t e = hipMallocAsync(reinterpret_cast<void**>(&scratch), sizeof(int) * (size_t)n * h * w, st);
    if (e != hipSuccess) return hip_fail(e, "hipMallocAsync(regions_label_i32)");
  }
  const int rc = regions_label_i32_launch(labels, ids, area ? area : scratch, n, h, w, connectivity, area != nullptr, st);
  if (scratch) {
    hipError_t e = hipFreeAsync(scratch, st);
    if (rc == UDASEG_OK && e != hipSuccess) return hip_fail(e, "hipFreeAsync(regions_label_i32)");
  }
  return rc;
}

extern "C" int udaseg_regions_sieve(const void* labels, int labels_i64, const int32_t* ids, const int32_t* area, int n, int h, int w,
                                    int has_ignore, int ignore_index, const int32_t* min_area, int void_label, uint8_t* out,
                                    int64_t* counts, void* stream) {
  if (int rc = rg_check("regions_sieve", labels_i64, n, h, w, has_ignore, ignore_index)) return rc;
  UDASEG_CHECK_ARG(void_label >= 0 && void_label <= 255, "regions_sieve: void_label must lie in [0, 255] (void_label=%d)", void_label);
  UDASEG_CHECK_ARG(labels && ids && area && min_area && out,
                   "regions_sieve: NULL pointer (labels, ids, area, min_area and out are required)");
  UDASEG_CHECK_ARG(((reinterpret_cast<uintptr_t>(ids) | reinterpret_cast<uintptr_t>(area) | reinterpret_cast<uintptr_t>(min_area)) & 3) == 0,
                   "regions_sieve: ids, area and min_area must be 4-byte aligned");
  UDASEG_CHECK_ARG((reinterpret_cast<uintptr_t>(counts) & 7) == 0, "regions_sieve: counts must be 8-byte aligned");
  if (int rc = map_aligned_ok("regions_sieve", "labels", labels_i64, labels)) return rc;
  RgScanArgs A = {};
  A.labels = labels;
  A.ids = ids;
  A.area = area;
  A.h = h;
  A.w = w;
  A.has_ignore = has_ignore;
  A.ignore_index = ignore_index;
  A.min_area = min_area;
  A.void_label = void_label;
  A.out = out;
  A.counts = reinterpret_cast<unsigned long long*>(counts);
  const dim3 grid(rg_flat_grid((int64_t)h * w), (unsigned int)n);
  dispatch_flags(
      [&](auto i64) { hipLaunchKernelGGL(regions_sieve_kernel<decltype(i64)::value>, grid, dim3(RG_THREADS), 0, as_stream(stream), A); },
      labels_i64 != 0);
  RG_LAUNCHED("regions_sieve launch");
  return UDASEG_OK;
}

extern "C" int udaseg_regions_stats(const void* labels, int labels_i64, const int32_t* ids, const int32_t* area, int n, int h, int w,
                                    int classes, int has_ignore, int ignore_index, int64_t* stats, void* stream) {
  if (int rc = rg_check("regions_stats", labels_i64, n, h, w, has_ignore, ignore_index)) return rc;
  UDASEG_CHECK_ARG(classes >= 1 && classes <= 255, "regions_stats: need 1 <= classes <= 255 (classes=%d)", classes);
  UDASEG_CHECK_ARG(labels && ids && area && stats, "regions_stats: NULL pointer (labels, ids, area and stats are required)");
  UDASEG_CHECK_ARG(((reinterpret_cast<uintptr_t>(ids) | reinterpret_cast<uintptr_t>(area)) & 3) == 0,
                   "regions_stats: ids and area must be 4-byte aligned");
  UDASEG_CHECK_ARG((reinterpret_cast<uintptr_t>(stats) & 7) == 0, "regions_stats: stats must be 8-byte aligned");
  if (int rc = map_aligned_ok("regions_stats", "labels", labels_i64, labels)) return rc;
  RgScanArgs A = {};
  A.labels = labels;
  A.ids = ids;
  A.area = area;
  A.h = h;
  A.w = w;
  A.has_ignore = has_ignore;
  A.ignore_index = ignore_index;
  A.stats = reinterpret_cast<unsigned long long*>(stats);
  A.classes = classes;
  const size_t lds = (size_t)classes * (sizeof(unsigned long long) + 33 * sizeof(unsigned int));   // <= 35700 bytes
  const dim3 grid(rg_flat_grid((int64_t)h * w), (unsigned int)n);
  dispatch_flags(
      [&](auto i64) { hipLaunchKernelGGL(regions_stats_kernel<decltype(i64)::value>, grid, dim3(RG_THREADS), lds, as_stream(stream), A); },
      labels_i64 != 0);
  RG_LAUNCHED("regions_stats launch");
  return UDASEG_OK;
}
