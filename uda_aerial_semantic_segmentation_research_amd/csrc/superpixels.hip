// Superpixels on the device: an integer SLIC whose every superpixel is one 4-connected piece, a majority vote of a label map per
// superpixel, the mean of a score map per superpixel, and a gather of a per-superpixel table back to the pixels.
//
// The rule (include/udaseg.h states it in full; tests/_superpixels_ref.py is its numpy mirror, compared for equality).  Everything
// is integer arithmetic: two runs give the same bits, whatever order the atomics arrive in.  There is no float atomic in this file.
//   grid     gh = ceil(h / S), gw = ceil(w / S), K = gh * gw clusters per image; cluster k = gy * gw + gx belongs to cell (gy, gx)
//   centres  int32 [n][K][6] = (Y, X, C0, C1, C2, count), Y .. C2 in units of 1/16; no gradient perturbation of the start values
//   assign   a pixel of cell (gy, gx) takes the smallest D = S^2 sum_i (16 c_i - C_i)^2 + m^2 ((16 y - Y)^2 + (16 x - X)^2) over the
//            clusters of the up to 9 cells around its own (64-bit; ties: the smallest k)
//   update   (16 sum + count / 2) / count per component, from the int32 sums of a cluster's pixels (count <= 9 S^2 <= 36864)
//   connect  4-connected components of the last labels; per cluster the main component (the one that holds pixel (0, 0), else the
//            largest, ties: the smallest root) is kept if its area >= min_area or it holds pixel (0, 0); every other component takes
//            the final label of the pixel just before its root, transitively
//
// Shape of the launches:
//   init     one thread per cluster: the start centre, zeroed sums.
//   assign   THE HOT PATH.  A block owns a tile of tc x tc whole cells (tc = max(1, 32 / S): 1024 pixels for S = 2 .. 16, one cell
//            above) and loads the centres of the (tc + 2)^2 cells its pixels can choose from into LDS.  A pixel's six integers go to
//            its cluster's LDS row with LDS atomics, summed over the wave first where many lanes share a cluster (SP_ROUNDS rounds of
//            "the first pending lane's cluster": four packed words, 24 shuffles a round); the block then adds its non-zero words to
//            the global sums, consecutive lanes on consecutive words.  Labels are written on request only (the last iteration).
//   finish   one thread per cluster: the new centre from the sums, which it zeroes for the next pass.
//   connect  udaseg::regions_label_i32_launch (regions.hip: tile / merge / resolve / finish) gives every pixel its component's root
//            and area.  main: every root offers (pixel-0 flag, area, ~root) to its cluster with ONE unsigned 64-bit atomicMax.
//            decide: every root compares its key with its cluster's maximum and leaves its final label (>= 0) or ~(the pixel before
//            it) in link[root].  walk: an absorbed root follows link / cid -- words the EARLIER launches wrote, read-only here --
//            down to a kept root (the roots strictly decrease, so the walk ends) and writes the label found to its own slot of
//            another array.  relabel: every pixel reads its root's slot.  No flags, spin-waits or inter-block counters: blocks hand
//            over at launch boundaries, as in regions.hip.
//   vote     count: int32 [n][K][C + 1] (class counts, then the size), one atomic per horizontal run of equal (cluster, class) within
//            a wave; decide: one thread per cluster; apply: one gather per pixel and the counters.
//   mean     accumulate: two unsigned 64-bit atomics per counted pixel (the value as rint(v 2^24), and 1); finish per cluster.
//   gather   mask[p] |= table[ids[p]].
// Every per-pixel launch is ONE thread per pixel (no capped grid: h * w < 2^31 gives at most 2^23 blocks).  A cluster index read from
// an ids / labels map is checked against K before it indexes a table: a caller's map cannot send a kernel out of bounds.
#include "label_maps.h"

namespace udaseg {

constexpr int SP_THREADS = 256;
static_assert(SP_THREADS == 64 * 4, "BlockCounts<K>: four waves a block");
constexpr int SP_MAX_TC = 16;                                  // cells per tile side at S = 2
constexpr int SP_SLOTS = (SP_MAX_TC + 2) * (SP_MAX_TC + 2);    // the cells a tile's pixels can choose from
constexpr int SP_ROUNDS = 2;                                   // wave-level sums per trip before the lanes fall back to their own atomics
constexpr int SP_SHARE = 8;                                    // lanes that must share a cluster for a wave-level sum to be taken
constexpr int SP_MAX_SIDE = 32768;

struct SpArgs {
  const uint8_t* frames;
  int* centres;                                // [n][K][6]
  int* accum;                                  // [n][K][6]
  int* labels;                                 // [n][h][w] or NULL
  int h, w, S, gh, gw, tc, tiles_x;
  long long S2, M2;
};

static inline int sp_tile_cells(int S) { return 32 / S > 1 ? 32 / S : 1; }

__global__ __launch_bounds__(SP_THREADS) void sp_init_kernel(SpArgs A) {
  const int K = A.gh * A.gw;
  const int k = (int)blockIdx.x * SP_THREADS + (int)threadIdx.x;
  if (k >= K) return;
  const int gy = k / A.gw, gx = k - gy * A.gw;
  const int y0 = min(gy * A.S + A.S / 2, A.h - 1), x0 = min(gx * A.S + A.S / 2, A.w - 1);
  const uint8_t* f = A.frames + ((size_t)blockIdx.y * A.h * A.w + (size_t)y0 * A.w + x0) * 3;
  int* c = A.centres + ((size_t)blockIdx.y * K + k) * 6;
  int* a = A.accum + ((size_t)blockIdx.y * K + k) * 6;
  c[0] = 16 * y0;
  c[1] = 16 * x0;
  c[2] = 16 * f[0];
  c[3] = 16 * f[1];
  c[4] = 16 * f[2];
  c[5] = 0;
#pragma unroll
  for (int j = 0; j < 6; ++j) a[j] = 0;
}

__device__ __forceinline__ int sp_wave_sum_i32(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(SP_THREADS) void sp_assign_kernel(SpArgs A) {
  __shared__ int cen[SP_SLOTS * 5];
  __shared__ int acc[SP_SLOTS * 6];
  const int tid = threadIdx.x, lane = tid & 63;
  const int S = A.S, tc = A.tc, h = A.h, w = A.w, gh = A.gh, gw = A.gw, K = gh * gw;
  const int cy0 = ((int)blockIdx.x / A.tiles_x) * tc, cx0 = ((int)blockIdx.x % A.tiles_x) * tc;   // the tile's first cell: inside the grid
  const int ly0 = cy0 - 1, lx0 = cx0 - 1, lw = tc + 2, nslots = lw * lw;                          // the window of cells in LDS
  const size_t HW = (size_t)h * w;
  const int* centres = A.centres + (size_t)blockIdx.y * K * 6;
  for (int i = tid; i < nslots; i += SP_THREADS) {
    const int gy = ly0 + i / lw, gx = lx0 + i % lw;
    const bool ok = gy >= 0 && gy < gh && gx >= 0 && gx < gw;                                      // every read is inside the table
#pragma unroll
    for (int j = 0; j < 5; ++j) cen[i * 5 + j] = ok ? centres[((size_t)gy * gw + gx) * 6 + j] : 0;
#pragma unroll
    for (int j = 0; j < 6; ++j) acc[i * 6 + j] = 0;
  }
  __syncthreads();
  const int py0 = cy0 * S, px0 = cx0 * S;                                                          // < h, < w: the cell is in the grid
  const int th = min(tc * S, h - py0), tw = min(tc * S, w - px0), npix = th * tw;                  // <= 64 x 64
  const uint8_t* f = A.frames + (size_t)blockIdx.y * HW * 3;
  for (int i0 = 0; i0 < npix; i0 += SP_THREADS) {                                                  // wave-uniform trips: the shuffles below
    const int i = i0 + tid;
    int pending = -1;                                                                              // the LDS row of the pixel's cluster
    int y = 0, x = 0, c0 = 0, c1 = 0, c2 = 0;
    if (i < npix) {
      const int ly = i / tw;
      y = py0 + ly;
      x = px0 + (i - ly * tw);
      const size_t p = (size_t)y * w + x;                                                          // y < h and x < w
      c0 = f[p * 3];
      c1 = f[p * 3 + 1];
      c2 = f[p * 3 + 2];
      const int gy = y / S, gx = x / S;
      const long long Y16 = 16 * y, X16 = 16 * x;
      const int q0 = 16 * c0, q1 = 16 * c1, q2 = 16 * c2;
      long long best = 0x7fffffffffffffffLL;
      int bk = 0;
      for (int dy = -1; dy <= 1; ++dy) {                                                           // ascending k: the first minimum wins
        const int cy = gy + dy;
        if (cy < 0 || cy >= gh) continue;
        for (int dx = -1; dx <= 1; ++dx) {
          const int cx = gx + dx;
          if (cx < 0 || cx >= gw) continue;
          const int s = (cy - ly0) * lw + (cx - lx0);                                              // in [0, nslots): |cy - cell row| <= 1
          const int* c = cen + s * 5;
          const long long ddy = Y16 - c[0], ddx = X16 - c[1];
          const int d0 = q0 - c[2], d1 = q1 - c[3], d2 = q2 - c[4];                                // |d| <= 4080: the sum fits 32 bits
          const long long D = A.S2 * (long long)(d0 * d0 + d1 * d1 + d2 * d2) + A.M2 * (ddy * ddy + ddx * ddx);
          if (D < best) {
            best = D;
            pending = s;
            bk = cy * gw + cx;
          }
        }
      }
      if (A.labels) A.labels[(size_t)blockIdx.y * HW + p] = bk;
    }
    // Lanes of one wave mostly share a few clusters (a wave covers one or two tile rows).  Per round the lanes of the first pending
    // lane's cluster are summed in registers and one lane adds the six sums; 64 lanes: y, x < 2^15 sum below 2^21, a colour below 2^14.
    for (int r = 0; r < SP_ROUNDS; ++r) {
      const unsigned long long m = __ballot(pending >= 0);
      if (m == 0) break;
      const int ls = __shfl(pending, __ffsll((long long)m) - 1, 64);
      const bool mine = pending == ls;
      const unsigned long long mm = __ballot(mine);
      if (__popcll(mm) < SP_SHARE) break;
      const int s0 = sp_wave_sum_i32(mine ? (y | (1 << 21)) : 0);                                  // sum y, and the count above it
      const int s1 = sp_wave_sum_i32(mine ? x : 0);
      const int s2 = sp_wave_sum_i32(mine ? (c0 | (c1 << 14)) : 0);
      const int s3 = sp_wave_sum_i32(mine ? c2 : 0);
      if (lane == __ffsll((long long)mm) - 1) {
        int* a = acc + ls * 6;
        atomicAdd(a + 0, s0 & 0x1fffff);
        atomicAdd(a + 1, s1);
        atomicAdd(a + 2, s2 & 0x3fff);
        atomicAdd(a + 3, s2 >> 14);
        atomicAdd(a + 4, s3);
        atomicAdd(a + 5, s0 >> 21);
      }
      if (mine) pending = -1;
    }
    if (pending >= 0) {
      int* a = acc + pending * 6;
      atomicAdd(a + 0, y);
      atomicAdd(a + 1, x);
      atomicAdd(a + 2, c0);
      atomicAdd(a + 3, c1);
      atomicAdd(a + 4, c2);
      atomicAdd(a + 5, 1);
    }
  }
  __syncthreads();
  int* accum = A.accum + (size_t)blockIdx.y * K * 6;
  for (int j = tid; j < nslots * 6; j += SP_THREADS) {                                             // consecutive lanes, consecutive words
    const int v = acc[j];
    if (v == 0) continue;                                                                          // a cell outside the grid is never chosen
    const int s = j / 6;
    const int gy = ly0 + s / lw, gx = lx0 + s % lw;
    atomicAdd(accum + ((size_t)gy * gw + gx) * 6 + (j - s * 6), v);
  }
}

__global__ __launch_bounds__(SP_THREADS) void sp_finish_kernel(SpArgs A) {
  const int K = A.gh * A.gw;
  const int k = (int)blockIdx.x * SP_THREADS + (int)threadIdx.x;
  if (k >= K) return;
  int* c = A.centres + ((size_t)blockIdx.y * K + k) * 6;
  int* a = A.accum + ((size_t)blockIdx.y * K + k) * 6;
  const int cnt = a[5];
  if (cnt > 0) {
#pragma unroll
    for (int j = 0; j < 5; ++j) c[j] = (int)((16LL * a[j] + cnt / 2) / cnt);
  }
  c[5] = cnt;                                  // a cluster without a pixel keeps its centre
#pragma unroll
  for (int j = 0; j < 6; ++j) a[j] = 0;
}

// ---- connect
struct SpConnArgs {
  const int* labels;                           // the clusters before the step
  const int* cid;                              // the component's root per pixel (-1: a negative label)
  int* area;                                   // the component's area per pixel; after the walk a root's slot holds its final label
  int* link;                                   // roots only: the final label, or ~(the pixel before the root)
  unsigned long long* mainkey;                 // [n][K]
  int* ids;
  unsigned long long* counts;                  // [n][4] or NULL
  int h, w, K, min_area;
};

__device__ __forceinline__ unsigned long long sp_key(int p, int area) {
  return ((unsigned long long)(p == 0) << 63) | ((unsigned long long)(unsigned int)area << 31) | (unsigned long long)(0x7fffffff - p);
}

__global__ __launch_bounds__(SP_THREADS) void sp_main_kernel(SpConnArgs A) {
  __shared__ BlockCounts<1>::Slots cnt;
  const size_t HW = (size_t)A.h * A.w, off = (size_t)blockIdx.y * HW;
  const size_t p = (size_t)blockIdx.x * SP_THREADS + threadIdx.x;
  unsigned int v[1] = {0};
  if (p < HW && A.cid[off + p] == (int)p) {
    const int k = A.labels[off + p];           // >= 0: a negative label has no component
    v[0] = 1;
    if (k < A.K) atomicMax(A.mainkey + (size_t)blockIdx.y * A.K + k, sp_key((int)p, A.area[off + p]));
  }
  if (A.counts) BlockCounts<1>::add(cnt, v, A.counts + (size_t)blockIdx.y * 4);          // counts[0]; block-uniform
}

__global__ __launch_bounds__(SP_THREADS) void sp_decide_kernel(SpConnArgs A) {
  __shared__ BlockCounts<2>::Slots cnt;
  const size_t HW = (size_t)A.h * A.w, off = (size_t)blockIdx.y * HW;
  const size_t p = (size_t)blockIdx.x * SP_THREADS + threadIdx.x;
  unsigned int v[2] = {0, 0};
  if (p < HW && A.cid[off + p] == (int)p) {
    const int k = A.labels[off + p], a = A.area[off + p];
    bool kept = true;                          // a label >= K is no cluster of this grid: it stands as it is
    if (k < A.K) {
      kept = A.mainkey[(size_t)blockIdx.y * A.K + k] == sp_key((int)p, a) && (a >= A.min_area || p == 0);
      v[kept ? 1 : 0] = 1;
    }
    // pixel 0's component carries the flag, the highest bit of the key: it is always kept, and every other root has a pixel before it
    const int x = (int)(p % (size_t)A.w);
    A.link[off + p] = kept ? k : ~(int)(x > 0 ? p - 1 : p - (size_t)A.w);
  }
  if (A.counts) {                              // block-uniform; v[0] goes to counts[1], v[1] to counts[3]
    BlockCounts<2>::put(cnt, v);
    __syncthreads();
    const unsigned int s = threadIdx.x < 2 ? BlockCounts<2>::total(cnt, threadIdx.x) : 0;
    if (s) atomicAdd(A.counts + (size_t)blockIdx.y * 4 + 1 + 2 * threadIdx.x, (unsigned long long)s);
  }
}

__global__ __launch_bounds__(SP_THREADS) void sp_walk_kernel(SpConnArgs A) {
  const size_t HW = (size_t)A.h * A.w, off = (size_t)blockIdx.y * HW;
  const size_t p = (size_t)blockIdx.x * SP_THREADS + threadIdx.x;
  if (p >= HW || A.cid[off + p] != (int)p) return;
  int l = A.link[off + p];
  while (l < 0) {                              // ends: q < the root it came from and cid[q] <= q, so the roots strictly decrease
    const int q = ~l;                          // the pixel before a root: inside the image (the decide launch wrote it)
    const int r = A.cid[off + q];
    if (r < 0) {                               // a negative label has no component: the label itself is what is taken
      l = A.labels[off + q];
      break;
    }
    l = A.link[off + r];
  }
  A.area[off + p] = l;                         // a root's own slot; nobody reads area in this launch
}

__global__ __launch_bounds__(SP_THREADS) void sp_relabel_kernel(SpConnArgs A) {
  __shared__ BlockCounts<1>::Slots cnt;
  const size_t HW = (size_t)A.h * A.w, off = (size_t)blockIdx.y * HW;
  const size_t p = (size_t)blockIdx.x * SP_THREADS + threadIdx.x;
  unsigned int v[1] = {0};
  if (p < HW) {
    const int old = A.labels[off + p], r = A.cid[off + p];
    const int now = r < 0 ? old : A.area[off + r];
    v[0] = now != old;
    A.ids[off + p] = now;                      // ids may be labels itself: this thread alone reads and writes the word
  }
  if (A.counts) BlockCounts<1>::add(cnt, v, A.counts + (size_t)blockIdx.y * 4 + 2);      // counts[2]; block-uniform
}

// ---- vote
struct SpVoteArgs {
  const int* ids;
  const void* masks;
  int* table;                                  // [n][K][classes + 1]
  int* winner;                                 // [n][K]: the class, -1: void
  uint8_t* out;
  unsigned long long* counts;                  // [n][3] or NULL
  int h, w, K, classes, has_ignore, ignore_index, void_label;
  double min_share, min_cover;
};

// The length of the run of equal keys that starts at this lane, 0 at every other lane and on a negative key.  Whole waves call.
__device__ __forceinline__ int sp_run_length(long long key) {
  const int lane = threadIdx.x & 63;
  const long long left = __shfl_up(key, 1, 64);
  const bool start = lane == 0 || left != key;
  const unsigned long long b = __ballot(start);
  const unsigned long long above = lane == 63 ? 0ull : b >> (lane + 1);
  const int next = above ? lane + __ffsll((long long)above) : 64;
  return (start && key >= 0) ? next - lane : 0;
}

template <bool I64>
__global__ __launch_bounds__(SP_THREADS) void sp_vote_count_kernel(SpVoteArgs A) {
  const size_t HW = (size_t)A.h * A.w, off = (size_t)blockIdx.y * HW;
  const size_t p = (size_t)blockIdx.x * SP_THREADS + threadIdx.x;
  const int C = A.classes;
  long long ksize = -1, kclass = -1;
  if (p < HW) {
    const int k = A.ids[off + p];
    if (k >= 0 && k < A.K) {
      const int m = label_at<I64>(A.masks, (int64_t)(off + p));
      ksize = (long long)k * (C + 1) + C;
      if (m < C && !(A.has_ignore && m == A.ignore_index)) kclass = (long long)k * (C + 1) + m;
    }
  }
  int* table = A.table + (size_t)blockIdx.y * A.K * (C + 1);
  const int ns = sp_run_length(ksize), nc = sp_run_length(kclass);
  if (ns) atomicAdd(table + ksize, ns);
  if (nc) atomicAdd(table + kclass, nc);
}

__global__ __launch_bounds__(SP_THREADS) void sp_vote_decide_kernel(SpVoteArgs A) {
  const int k = (int)blockIdx.x * SP_THREADS + (int)threadIdx.x;
  if (k >= A.K) return;
  const int C = A.classes;
  const int* row = A.table + ((size_t)blockIdx.y * A.K + k) * (C + 1);
  int win = 0, best = -1;
  long long labelled = 0;
  for (int c = 0; c < C; ++c) {
    const int v = row[c];
    labelled += v;
    if (v > win) {                             // the first largest count: ties go to the smallest class
      win = v;
      best = c;
    }
  }
  const bool ok = labelled > 0 && (double)win >= A.min_share * (double)labelled && (double)labelled >= A.min_cover * (double)row[C];
  A.winner[(size_t)blockIdx.y * A.K + k] = ok ? best : -1;
}

template <bool I64>
__global__ __launch_bounds__(SP_THREADS) void sp_vote_apply_kernel(SpVoteArgs A) {
  __shared__ BlockCounts<3>::Slots cnt;
  const size_t HW = (size_t)A.h * A.w, off = (size_t)blockIdx.y * HW;
  const size_t p = (size_t)blockIdx.x * SP_THREADS + threadIdx.x;
  unsigned int v[3] = {0, 0, 0};
  if (p < HW) {
    const int k = A.ids[off + p];
    const int m = label_at<I64>(A.masks, (int64_t)(off + p));
    const bool labelled = m < A.classes && !(A.has_ignore && m == A.ignore_index);
    const int d = (k >= 0 && k < A.K) ? A.winner[(size_t)blockIdx.y * A.K + k] : -1;
    A.out[off + p] = (uint8_t)(d >= 0 ? d : A.void_label);
    v[0] = labelled && d >= 0 && d != m;
    v[1] = !labelled && d >= 0;
    v[2] = labelled && d < 0;
  }
  if (A.counts) BlockCounts<3>::add(cnt, v, A.counts + (size_t)blockIdx.y * 3);          // block-uniform
}

// ---- mean, gather
struct SpMeanArgs {
  const float* values;
  const int* ids;
  unsigned long long* sums;                    // [n][K][2]: the quantised sum, the count
  float* mean;                                 // [n][K]
  const uint8_t* table;                        // gather: [n][K]
  uint8_t* mask;
  int h, w, K;
};

__global__ __launch_bounds__(SP_THREADS) void sp_mean_accumulate_kernel(SpMeanArgs A) {
  const size_t HW = (size_t)A.h * A.w, off = (size_t)blockIdx.y * HW;
  const size_t p = (size_t)blockIdx.x * SP_THREADS + threadIdx.x;
  if (p >= HW) return;
  const int k = A.ids[off + p];
  const float v = A.values[off + p];
  if (k < 0 || k >= A.K || !(v >= 0.f && v <= 1.f)) return;       // a NaN fails both comparisons
  unsigned long long* s = A.sums + ((size_t)blockIdx.y * A.K + k) * 2;
  atomicAdd(s, (unsigned long long)rintf(v * 16777216.f));        // the product is exact; < 2^24 + 1, and at most 2^31 of them
  atomicAdd(s + 1, 1ull);
}

__global__ __launch_bounds__(SP_THREADS) void sp_mean_finish_kernel(SpMeanArgs A) {
  const int k = (int)blockIdx.x * SP_THREADS + (int)threadIdx.x;
  if (k >= A.K) return;
  const unsigned long long* s = A.sums + ((size_t)blockIdx.y * A.K + k) * 2;
  A.mean[(size_t)blockIdx.y * A.K + k] = s[1] ? (float)((double)s[0] / ((double)s[1] * 16777216.0)) : -1.f;
}

__global__ __launch_bounds__(SP_THREADS) void sp_gather_kernel(SpMeanArgs A) {
  const size_t HW = (size_t)A.h * A.w, off = (size_t)blockIdx.y * HW;
  const size_t p = (size_t)blockIdx.x * SP_THREADS + threadIdx.x;
  if (p >= HW) return;
  const int k = A.ids[off + p];
  if (k < 0 || k >= A.K) return;
  const uint8_t t = A.table[(size_t)blockIdx.y * A.K + k];
  if (t) A.mask[off + p] |= t;
}

// ---- host side
#define SP_LAUNCHED(what)                                   \
  do {                                                      \
    hipError_t e__ = hipGetLastError();                     \
    if (e__ != hipSuccess) return hip_fail(e__, what);      \
  } while (0)

static inline bool sp_aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

static int sp_check_shape(const char* who, int n, int h, int w) {
  if (int rc = map_batch_ok(who, n)) return rc;
  UDASEG_CHECK_ARG(h >= 1 && w >= 1 && h <= SP_MAX_SIDE && w <= SP_MAX_SIDE && (int64_t)h * w < ((int64_t)1 << 31),
                   "%s: need 1 <= h, w <= 32768 and h * w < 2^31 (h=%d w=%d)", who, h, w);
  return UDASEG_OK;
}

static int sp_check_step(const char* who, int step) {
  UDASEG_CHECK_ARG(step >= 2 && step <= 64, "%s: step must lie in [2, 64] (step=%d)", who, step);
  return UDASEG_OK;
}

static int sp_check_clusters(const char* who, int clusters) {
  UDASEG_CHECK_ARG(clusters >= 1 && clusters <= (1 << 28), "%s: clusters must lie in [1, 2^28] (clusters=%d)", who, clusters);
  return UDASEG_OK;
}

static SpArgs sp_args(const uint8_t* frames, int h, int w, int step, int compactness, int* centres) {
  SpArgs A = {};
  A.frames = frames;
  A.centres = centres;
  A.h = h;
  A.w = w;
  A.S = step;
  A.gh = cdiv(h, step);
  A.gw = cdiv(w, step);
  A.tc = sp_tile_cells(step);
  A.tiles_x = cdiv(A.gw, A.tc);
  A.S2 = (long long)step * step;
  A.M2 = (long long)compactness * compactness;
  return A;
}

static inline dim3 sp_cluster_grid(int K, int n) { return dim3((unsigned int)cdiv(K, SP_THREADS), (unsigned int)n); }
static inline dim3 sp_pixel_grid(int h, int w, int n) {
  return dim3((unsigned int)cdiv64((int64_t)h * w, SP_THREADS), (unsigned int)n);                   // <= 2^23 blocks
}

// one iteration: labels = assign(centres), centres = update(labels); A.accum is zero on entry and on return
static int sp_iterate(const SpArgs& A, int n, hipStream_t st) {
  const dim3 tiles((unsigned int)((int64_t)A.tiles_x * cdiv(A.gh, A.tc)), (unsigned int)n);         // <= 2^28 blocks
  hipLaunchKernelGGL(sp_assign_kernel, tiles, dim3(SP_THREADS), 0, st, A);
  SP_LAUNCHED("superpixel assign launch");
  hipLaunchKernelGGL(sp_finish_kernel, sp_cluster_grid(A.gh * A.gw, n), dim3(SP_THREADS), 0, st, A);
  SP_LAUNCHED("superpixel finish launch");
  return UDASEG_OK;
}

// scratch of the connect step: mainkey [n][K] (64-bit), then cid, area, link [n][h][w] (32-bit)
static inline size_t sp_connect_bytes(int n, int h, int w, int K) {
  return sizeof(unsigned long long) * (size_t)n * K + 3 * sizeof(int) * (size_t)n * h * w;
}

static int sp_connect(const int* labels, int n, int h, int w, int K, int min_area, int* ids, int64_t* counts, void* scratch,
                      hipStream_t st) {
  const size_t nhw = (size_t)n * h * w;
  SpConnArgs A = {};
  A.labels = labels;
  A.mainkey = reinterpret_cast<unsigned long long*>(scratch);
  int* cid = reinterpret_cast<int*>(A.mainkey + (size_t)n * K);
  A.cid = cid;
  A.area = cid + nhw;
  A.link = cid + 2 * nhw;
  A.ids = ids;
  A.counts = reinterpret_cast<unsigned long long*>(counts);
  A.h = h;
  A.w = w;
  A.K = K;
  A.min_area = min_area;
  hipError_t e = hipMemsetAsync(A.mainkey, 0, sizeof(unsigned long long) * (size_t)n * K, st);
  if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync(superpixel connect)");
  if (int rc = regions_label_i32_launch(labels, cid, A.area, n, h, w, 4, 1, st)) return rc;
  const dim3 grid = sp_pixel_grid(h, w, n);
  hipLaunchKernelGGL(sp_main_kernel, grid, dim3(SP_THREADS), 0, st, A);
  SP_LAUNCHED("superpixel main launch");
  hipLaunchKernelGGL(sp_decide_kernel, grid, dim3(SP_THREADS), 0, st, A);
  SP_LAUNCHED("superpixel decide launch");
  hipLaunchKernelGGL(sp_walk_kernel, grid, dim3(SP_THREADS), 0, st, A);
  SP_LAUNCHED("superpixel walk launch");
  hipLaunchKernelGGL(sp_relabel_kernel, grid, dim3(SP_THREADS), 0, st, A);
  SP_LAUNCHED("superpixel relabel launch");
  return UDASEG_OK;
}

// stream-ordered scratch, the way udaseg_regions_label takes its own
struct SpScratch {
  void* ptr = nullptr;
  hipStream_t st;
  explicit SpScratch(hipStream_t s) : st(s) {}
  int take(size_t bytes, const char* what) {
    hipError_t e = hipMallocAsync(&ptr, bytes, st);
    if (e != hipSuccess) {
      ptr = nullptr;
      return hip_fail(e, what);
    }
    return UDASEG_OK;
  }
  int give(int rc, const char* what) {
    if (ptr == nullptr) return rc;
    hipError_t e = hipFreeAsync(ptr, st);
    ptr = nullptr;
    if (rc == UDASEG_OK && e != hipSuccess) return hip_fail(e, what);
    return rc;
  }
};

}  // namespace udaseg

using namespace udaseg;

extern "C" int udaseg_superpixel_slic(const uint8_t* frames, int n, int h, int w, int step, int compactness, int iterations,
                                      int min_area, int32_t* ids, int32_t* centres, int64_t* counts, void* stream) {
  if (int rc = sp_check_shape("superpixel_slic", n, h, w)) return rc;
  if (int rc = sp_check_step("superpixel_slic", step)) return rc;
  UDASEG_CHECK_ARG(compactness >= 1 && compactness <= 1024, "superpixel_slic: compactness must lie in [1, 1024] (compactness=%d)", compactness);
  UDASEG_CHECK_ARG(iterations >= 1 && iterations <= 64, "superpixel_slic: iterations must lie in [1, 64] (iterations=%d)", iterations);
  UDASEG_CHECK_ARG(min_area >= 0, "superpixel_slic: min_area must be >= 0 (min_area=%d)", min_area);
  UDASEG_CHECK_ARG(frames && ids && centres, "superpixel_slic: NULL pointer (frames, ids and centres are required)");
  UDASEG_CHECK_ARG(sp_aligned(ids, 4) && sp_aligned(centres, 4), "superpixel_slic: ids and centres must be 4-byte aligned");
  UDASEG_CHECK_ARG(sp_aligned(counts, 8), "superpixel_slic: counts must be 8-byte aligned");
  hipStream_t st = as_stream(stream);
  SpArgs A = sp_args(frames, h, w, step, compactness, centres);
  const int K = A.gh * A.gw;                   // <= 16384^2 = 2^28
  const size_t conn = sp_connect_bytes(n, h, w, K);
  SpScratch scratch(st);
  if (int rc = scratch.take(conn + sizeof(int) * 6 * (size_t)n * K, "hipMallocAsync(superpixel_slic)")) return rc;
  A.accum = reinterpret_cast<int*>(reinterpret_cast<uint8_t*>(scratch.ptr) + conn);                 // conn is a multiple of 4
  int rc = UDASEG_OK;
  hipLaunchKernelGGL(sp_init_kernel, sp_cluster_grid(K, n), dim3(SP_THREADS), 0, st, A);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) rc = hip_fail(e, "superpixel init launch");
  for (int t = 0; t < iterations && rc == UDASEG_OK; ++t) {
    A.labels = t == iterations - 1 ? ids : nullptr;                                                // the last labels only: in ids itself
    rc = sp_iterate(A, n, st);
  }
  if (rc == UDASEG_OK) rc = sp_connect(ids, n, h, w, K, min_area, ids, counts, scratch.ptr, st);
  return scratch.give(rc, "hipFreeAsync(superpixel_slic)");
}

extern "C" int udaseg_superpixel_assign(const uint8_t* frames, int n, int h, int w, int step, int compactness, int32_t* centres,
                                        int32_t* labels, void* stream) {
  if (int rc = sp_check_shape("superpixel_assign", n, h, w)) return rc;
  if (int rc = sp_check_step("superpixel_assign", step)) return rc;
  UDASEG_CHECK_ARG(compactness >= 1 && compactness <= 1024, "superpixel_assign: compactness must lie in [1, 1024] (compactness=%d)", compactness);
  UDASEG_CHECK_ARG(frames && centres, "superpixel_assign: NULL pointer (frames and centres are required)");
  UDASEG_CHECK_ARG(sp_aligned(centres, 4) && sp_aligned(labels, 4), "superpixel_assign: centres and labels must be 4-byte aligned");
  hipStream_t st = as_stream(stream);
  SpArgs A = sp_args(frames, h, w, step, compactness, centres);
  A.labels = labels;
  const size_t bytes = sizeof(int) * 6 * (size_t)n * A.gh * A.gw;
  SpScratch scratch(st);
  if (int rc = scratch.take(bytes, "hipMallocAsync(superpixel_assign)")) return rc;
  A.accum = reinterpret_cast<int*>(scratch.ptr);
  int rc = UDASEG_OK;
  hipError_t e = hipMemsetAsync(A.accum, 0, bytes, st);
  if (e != hipSuccess) rc = hip_fail(e, "hipMemsetAsync(superpixel_assign)");
  if (rc == UDASEG_OK) rc = sp_iterate(A, n, st);
  return scratch.give(rc, "hipFreeAsync(superpixel_assign)");
}

extern "C" int udaseg_superpixel_connect(const int32_t* labels, int n, int h, int w, int step, int min_area, int32_t* ids,
                                         int64_t* counts, void* stream) {
  if (int rc = sp_check_shape("superpixel_connect", n, h, w)) return rc;
  if (int rc = sp_check_step("superpixel_connect", step)) return rc;
  UDASEG_CHECK_ARG(min_area >= 0, "superpixel_connect: min_area must be >= 0 (min_area=%d)", min_area);
  UDASEG_CHECK_ARG(labels && ids, "superpixel_connect: NULL pointer (labels and ids are required)");
  UDASEG_CHECK_ARG(sp_aligned(labels, 4) && sp_aligned(ids, 4), "superpixel_connect: labels and ids must be 4-byte aligned");
  UDASEG_CHECK_ARG(sp_aligned(counts, 8), "superpixel_connect: counts must be 8-byte aligned");
  hipStream_t st = as_stream(stream);
  const int K = cdiv(h, step) * cdiv(w, step);
  SpScratch scratch(st);
  if (int rc = scratch.take(sp_connect_bytes(n, h, w, K), "hipMallocAsync(superpixel_connect)")) return rc;
  const int rc = sp_connect(labels, n, h, w, K, min_area, ids, counts, scratch.ptr, st);
  return scratch.give(rc, "hipFreeAsync(superpixel_connect)");
}

extern "C" int udaseg_superpixel_vote(const int32_t* ids, const void* masks, int masks_i64, int n, int h, int w, int clusters,
                                      int classes, int has_ignore, int ignore_index, float min_share, float min_cover,
                                      int void_label, uint8_t* out, int64_t* counts, void* stream) {
  if (int rc = sp_check_shape("superpixel_vote", n, h, w)) return rc;
  if (int rc = sp_check_clusters("superpixel_vote", clusters)) return rc;
  if (int rc = map_storage_ok("superpixel_vote", "masks_i64", masks_i64)) return rc;
  UDASEG_CHECK_ARG(classes >= 1 && classes <= 255, "superpixel_vote: need 1 <= classes <= 255 (classes=%d)", classes);
  if (int rc = map_ignore_ok("superpixel_vote", has_ignore, ignore_index)) return rc;
  UDASEG_CHECK_ARG(min_share >= 0.f && min_share <= 1.f, "superpixel_vote: min_share must lie in [0, 1] (min_share=%g)", (double)min_share);
  UDASEG_CHECK_ARG(min_cover >= 0.f && min_cover <= 1.f, "superpixel_vote: min_cover must lie in [0, 1] (min_cover=%g)", (double)min_cover);
  UDASEG_CHECK_ARG(void_label >= 0 && void_label <= 255, "superpixel_vote: void_label must lie in [0, 255] (void_label=%d)", void_label);
  UDASEG_CHECK_ARG(ids && masks && out, "superpixel_vote: NULL pointer (ids, masks and out are required)");
  UDASEG_CHECK_ARG(sp_aligned(ids, 4), "superpixel_vote: ids must be 4-byte aligned");
  UDASEG_CHECK_ARG(sp_aligned(counts, 8), "superpixel_vote: counts must be 8-byte aligned");
  if (int rc = map_aligned_ok("superpixel_vote", "masks", masks_i64, masks)) return rc;
  hipStream_t st = as_stream(stream);
  SpVoteArgs A = {};
  A.ids = ids;
  A.masks = masks;
  A.out = out;
  A.counts = reinterpret_cast<unsigned long long*>(counts);
  A.h = h;
  A.w = w;
  A.K = clusters;
  A.classes = classes;
  A.has_ignore = has_ignore;
  A.ignore_index = ignore_index;
  A.void_label = void_label;
  A.min_share = (double)min_share;
  A.min_cover = (double)min_cover;
  const size_t rows = (size_t)n * clusters, table = sizeof(int) * rows * (classes + 1);
  SpScratch scratch(st);
  if (int rc = scratch.take(table + sizeof(int) * rows, "hipMallocAsync(superpixel_vote)")) return rc;
  A.table = reinterpret_cast<int*>(scratch.ptr);
  A.winner = A.table + rows * (classes + 1);
  int rc = UDASEG_OK;
  hipError_t e = hipMemsetAsync(A.table, 0, table, st);
  if (e != hipSuccess) rc = hip_fail(e, "hipMemsetAsync(superpixel_vote)");
  const dim3 grid = sp_pixel_grid(h, w, n);
  if (rc == UDASEG_OK) {
    dispatch_flags(
        [&](auto i64) {
          hipLaunchKernelGGL(sp_vote_count_kernel<decltype(i64)::value>, grid, dim3(SP_THREADS), 0, st, A);
          hipLaunchKernelGGL(sp_vote_decide_kernel, sp_cluster_grid(clusters, n), dim3(SP_THREADS), 0, st, A);
          hipLaunchKernelGGL(sp_vote_apply_kernel<decltype(i64)::value>, grid, dim3(SP_THREADS), 0, st, A);
        },
        masks_i64 != 0);
    e = hipGetLastError();
    if (e != hipSuccess) rc = hip_fail(e, "superpixel vote launch");
  }
  return scratch.give(rc, "hipFreeAsync(superpixel_vote)");
}

extern "C" int udaseg_superpixel_mean(const float* values, const int32_t* ids, int n, int h, int w, int clusters, float* mean,
                                      void* stream) {
  if (int rc = sp_check_shape("superpixel_mean", n, h, w)) return rc;
  if (int rc = sp_check_clusters("superpixel_mean", clusters)) return rc;
  UDASEG_CHECK_ARG(values && ids && mean, "superpixel_mean: NULL pointer (values, ids and mean are required)");
  UDASEG_CHECK_ARG(sp_aligned(values, 4) && sp_aligned(ids, 4) && sp_aligned(mean, 4),
                   "superpixel_mean: values, ids and mean must be 4-byte aligned");
  hipStream_t st = as_stream(stream);
  SpMeanArgs A = {};
  A.values = values;
  A.ids = ids;
  A.mean = mean;
  A.h = h;
  A.w = w;
  A.K = clusters;
  const size_t bytes = 2 * sizeof(unsigned long long) * (size_t)n * clusters;
  SpScratch scratch(st);
  if (int rc = scratch.take(bytes, "hipMallocAsync(superpixel_mean)")) return rc;
  A.sums = reinterpret_cast<unsigned long long*>(scratch.ptr);
  int rc = UDASEG_OK;
  hipError_t e = hipMemsetAsync(A.sums, 0, bytes, st);
  if (e != hipSuccess) rc = hip_fail(e, "hipMemsetAsync(superpixel_mean)");
  if (rc == UDASEG_OK) {
    hipLaunchKernelGGL(sp_mean_accumulate_kernel, sp_pixel_grid(h, w, n), dim3(SP_THREADS), 0, st, A);
    hipLaunchKernelGGL(sp_mean_finish_kernel, sp_cluster_grid(clusters, n), dim3(SP_THREADS), 0, st, A);
    e = hipGetLastError();
    if (e != hipSuccess) rc = hip_fail(e, "superpixel mean launch");
  }
  return scratch.give(rc, "hipFreeAsync(superpixel_mean)");
}

extern "C" int udaseg_superpixel_gather(const int32_t* ids, const uint8_t* table, int n, int h, int w, int clusters, uint8_t* mask,
                                        void* stream) {
  if (int rc = sp_check_shape("superpixel_gather", n, h, w)) return rc;
  if (int rc = sp_check_clusters("superpixel_gather", clusters)) return rc;
  UDASEG_CHECK_ARG(ids && table && mask, "superpixel_gather: NULL pointer (ids, table and mask are required)");
  UDASEG_CHECK_ARG(sp_aligned(ids, 4), "superpixel_gather: ids must be 4-byte aligned");
  SpMeanArgs A = {};
  A.ids = ids;
  A.table = table;
  A.mask = mask;
  A.h = h;
  A.w = w;
  A.K = clusters;
  hipLaunchKernelGGL(sp_gather_kernel, sp_pixel_grid(h, w, n), dim3(SP_THREADS), 0, as_stream(stream), A);
  SP_LAUNCHED("superpixel gather launch");
  return UDASEG_OK;
}
