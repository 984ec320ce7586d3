// CRF refinement of class scores under the frame: windowed mean-field inference (ConvCRF, Teichmann & Cipolla 2018; the mean field of
// Kraehenbuehl & Koltun 2011 with the messages restricted to a (2R+1)^2 window of dilation d; an extension: the reference has no
// counterpart).  include/udaseg.h states the rule; tests/_crf_ref.py is its numpy mirror.  With torch this is an unfold of
// [N, C K^2, H W] per sweep; here it is two kernels:
//   udaseg_crf_prepare  ONE streaming pass over the scores: log P0, Q^0 = P0 and a valid flag per pixel
//   udaseg_crf_step     one Jacobi sweep Q^t -> Q^{t+1}; the host ping-pongs two buffers, one launch per sweep, so the hand-over
//                       between sweeps is the launch boundary (regions.hip's: no flags, no waits)
//
// The step is a stencil over class VECTORS with data-dependent weights: per (pixel, neighbour) about ten VALU operations form k_ij
// (two byte dot products give the exact integer colour distance, one native exponential, one fma) and 4 NV fused multiply-adds apply
// it to the neighbour's class row.  It is bound by the LDS reads of those rows and by the VALU, not by memory.  The plan:
//   tile       32 columns, one LANE PER COLUMN, so that the 16-lane groups of a ds_read_b128 hold 16 consecutive pixels of one row.
//              The Q halo lies in LDS as [vector q][halo row][halo column] of f32x4: consecutive lanes read consecutive 16-byte
//              slots, whatever the dilation shifts the window by (every lane shifts alike) -- no bank conflict, no padding.  (Rows
//              of pixels, [pixel][ldq], put lanes 16 NV bytes apart: a 2-way conflict at 24 floats, 4-way at 32.)
//   reuse      a thread owns CRF_PY = 2 pixels d ROWS apart: the neighbour rows of (y, x) and (y + d, x) are the same lattice
//              shifted by one, so one read of a Q_j row (and of its frame word) serves both; 2R + 2 reads per window column for two
//              pixels instead of 4R + 2.  The weights differ per pixel; the reads do not.  Owning horizontally adjacent pixels
//              instead would share reads only at d == 1 and put the lanes two slots apart (2-way conflicts), so the pair is
//              vertical.  The tile's height is 2 * rows of threads with rows = (8 / d) * d: 16, 16, 12, 16 rows for d = 1 .. 4.
//   frame      the halo's frame pixels are one uint32 each: R | G << 8 | B << 16 | valid << 24 -- 0 outside the image and for a
//              void pixel, whose Q is staged as zeros: it sends nothing, and its flag keeps it out of Z.
//   classes    the Q halo of (th + 2Rd)(32 + 2Rd) pixels at 16 NV bytes each exceeds half a CU's LDS from R d = 3 on at 23
//              classes, so the class vectors are staged in CHUNKS of CV <= NV vectors (the whole row where it fits 80 KB, else 3,
//              else 2): the accumulators of all NV vectors stay in registers, the weights are formed again per chunk.
//   tables     w_app S_alpha and w_smooth S_gamma are multiplied once per block into LDS (the centre is zeroed there: (0, 0) is
//              no neighbour); the window loops are uniform, so reading them is a broadcast.
// Tried and not kept (DESIGN.md "CRF refinement" has the figures): the tables read with scalar loads instead of from LDS, together
// with reading the next lattice row before the current one is applied.  Scalar loads and LDS reads share one counter and scalar
// loads return out of order, so every table load drained the LDS reads in flight: one step took 0.35 / 0.48 / 1.13 ms against
// 0.30 / 0.42 / 0.88 ms of this form at (R, d) = (3, 1), (3, 2), (5, 2).
#include "launch.h"
#include "scores_common.h"

namespace udaseg {

constexpr int CRF_TW = 32;                       // tile width: a lane per column
constexpr int CRF_PY = 2;                        // pixels of a thread, `dilation` rows apart
constexpr int CRF_MAX_R = 5, CRF_MAX_D = 4, CRF_MAX_HALO = 10;
constexpr int CRF_TAB = 128;                     // floats per staged table: (2 * 5 + 1)^2 = 121 at most
constexpr int CRF_LDS_BUDGET = 80 * 1024;        // two blocks per CU
constexpr int CRF_PREP_THREADS = 256, CRF_PREP_MAX_BLOCKS = 4096;

static inline int crf_thread_rows(int d) { return (8 / d) * d; }
static inline bool crf_window_ok(int radius, int dilation) {
  return radius >= 1 && radius <= CRF_MAX_R && dilation >= 1 && dilation <= CRF_MAX_D && radius * dilation <= CRF_MAX_HALO;
}
static inline int crf_lds_bytes(int halo_pixels, int cv) { return (16 * cv + 4) * halo_pixels + 2 * CRF_TAB * 4; }

template <int NV>
__global__ __launch_bounds__(CRF_PREP_THREADS) void crf_prepare_kernel(const float* __restrict__ scores, int ldc, int classes, int probs,
                                                                       int64_t pixels, float* __restrict__ logp,
                                                                       float* __restrict__ q0, int ldq, uint8_t* __restrict__ valid) {
  const float qnan = __builtin_nanf("");
  const int lv = ldq >> 2;
  for (int64_t p = (int64_t)blockIdx.x * CRF_PREP_THREADS + threadIdx.x; p < pixels; p += (int64_t)gridDim.x * CRF_PREP_THREADS) {
    f32x4 v[NV], e[NV];
    load_row<NV>(scores + p * ldc, v);
    float m;
    first_max<NV>(v, classes, m);
    bool ok = true;
    f32x4 s4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < NV; ++q)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const bool in = 4 * q + c < classes;
        const float x = v[q][c];
        ok &= !in || (probs ? (x >= 0.f && x <= 1.f) : __builtin_isfinite(x));
        v[q][c] = x - m;
        e[q][c] = in ? (probs ? x : expf(x - m)) : 0.f;
        s4[c] += e[q][c];
      }
    const float S = (s4[0] + s4[1]) + (s4[2] + s4[3]);
    ok &= __builtin_isfinite(S) && S > 0.f;
    const float logS = logf(S);
    float* lrow = logp + p * ldq;
    float* qrow = q0 + p * ldq;
#pragma unroll
    for (int q = 0; q < NV; ++q) {
      f32x4 lo, qo;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const bool in = 4 * q + c < classes;
        const float pc = e[q][c] / S;
        const float lp = probs ? logf(pc) : v[q][c] - logS;
        lo[c] = in ? (ok ? lp : qnan) : 0.f;
        qo[c] = in ? (ok ? pc : qnan) : 0.f;
      }
      *reinterpret_cast<f32x4*>(lrow + 4 * q) = lo;
      *reinterpret_cast<f32x4*>(qrow + 4 * q) = qo;
    }
    for (int q = NV; q < lv; ++q) {
      *reinterpret_cast<f32x4*>(lrow + 4 * q) = f32x4{0.f, 0.f, 0.f, 0.f};
      *reinterpret_cast<f32x4*>(qrow + 4 * q) = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    valid[p] = ok ? 1 : 0;
  }
}

struct CrfArgs {
  const float* logp;
  const float* q;
  const uint8_t* valid;
  const uint8_t* frames;
  const float* sa;
  const float* sg;
  float* out;
  int n, h, w, classes, ldq, R, d, rows, ntx, nty;     // rows: rows of threads of a block
  float wa, ws, inv2b, strength;
};

// sum of the squares of the three colour bytes of a frame word / the byte dot product of two (the flag byte is masked by the caller)
__device__ __forceinline__ int crf_dot(uint32_t a, uint32_t b) { return (int)__builtin_amdgcn_udot4(a, b, 0u, false); }

template <int NV, int CV>
__global__ __launch_bounds__(256) void crf_step_kernel(CrfArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char crf_lds[];
  constexpr int NCH = (NV + CV - 1) / CV;
  const int R = a.R, d = a.d, halo = R * d, K = 2 * R + 1;
  const int TH = a.rows * CRF_PY, HR = TH + 2 * halo, HW = CRF_TW + 2 * halo, HP = HR * HW;
  const int threads = a.rows * CRF_TW;
  f32x4* Qs = reinterpret_cast<f32x4*>(crf_lds);                     // [CV][HR][HW]
  uint32_t* Fs = reinterpret_cast<uint32_t*>(Qs + CV * HP);           // [HR][HW]
  float* tA = reinterpret_cast<float*>(Fs + HP);                      // [K][K] w_app * S_alpha, 0 at the centre
  float* tG = tA + CRF_TAB;                                           // [K][K] w_smooth * S_gamma, 0 at the centre

  int b = blockIdx.x;
  const int tile_x = b % a.ntx;
  b /= a.ntx;
  const int tile_y = b % a.nty, img = b / a.nty;
  const int x_base = tile_x * CRF_TW, y_base = tile_y * TH;
  const int64_t img_base = (int64_t)img * a.h * a.w;
  const int tid = threadIdx.x, tx = tid & (CRF_TW - 1), ty = tid >> 5;
  const float rcp_hw = 1.f / (float)HW;

  for (int i = tid; i < K * K; i += threads) {
    const bool centre = i == (K * K) / 2;
    tA[i] = centre ? 0.f : a.wa * a.sa[i];
    tG[i] = centre ? 0.f : a.ws * a.sg[i];
  }
  for (int i = tid; i < HP; i += threads) {
    const int ry = fast_div(i, HW, rcp_hw), rx = i - ry * HW;
    const int gy = y_base - halo + ry, gx = x_base - halo + rx;
    uint32_t word = 0;
    if (gy >= 0 && gy < a.h && gx >= 0 && gx < a.w) {
      const int64_t p = img_base + (int64_t)gy * a.w + gx;
      if (a.valid[p]) {
        const uint8_t* f = a.frames + p * 3;
        word = (uint32_t)f[0] | ((uint32_t)f[1] << 8) | ((uint32_t)f[2] << 16) | (1u << 24);
      }
    }
    Fs[i] = word;
  }
  __syncthreads();

  // the thread's pixels: tile rows ly0 and ly0 + d, column tx
  const int ly0 = (ty / d) * (d * CRF_PY) + ty % d;
  uint32_t am[CRF_PY];
  int aa[CRF_PY];
  bool own[CRF_PY];
#pragma unroll
  for (int k = 0; k < CRF_PY; ++k) {
    const uint32_t word = Fs[(ly0 + k * d + halo) * HW + tx + halo];
    own[k] = (word >> 24) != 0u;
    am[k] = word & 0xffffffu;
    aa[k] = crf_dot(am[k], am[k]);
  }
  f32x4 acc[CRF_PY][NV];
  float z[CRF_PY];
#pragma unroll
  for (int k = 0; k < CRF_PY; ++k) {
    z[k] = 0.f;
#pragma unroll
    for (int q = 0; q < NV; ++q) acc[k][q] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) {
    const int c0 = ch * CV;
    const int cvn = NV - c0 < CV ? NV - c0 : CV;                     // vectors of this chunk: a constant after unrolling
    if (ch > 0) __syncthreads();                                     // the previous chunk has been read
    for (int i = tid; i < HP * cvn; i += threads) {
      const int pix = i / cvn, qq = i - pix * cvn;                   // consecutive lanes: consecutive vectors of one pixel's row
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (Fs[pix] >> 24) {                                           // inside the image and valid
        const int ry = fast_div(pix, HW, rcp_hw), rx = pix - ry * HW;
        const int64_t p = img_base + (int64_t)(y_base - halo + ry) * a.w + (x_base - halo + rx);
        v = *reinterpret_cast<const f32x4*>(a.q + p * a.ldq + 4 * (c0 + qq));
      }
      Qs[qq * HP + pix] = v;
    }
    __syncthreads();

#pragma unroll 1
    for (int dxi = 0; dxi < K; ++dxi) {
      const int col = tx + dxi * d;                                  // halo column of the neighbour: tx + halo + (dxi - R) d
#pragma unroll 1
      for (int yi = 0; yi < K + CRF_PY - 1; ++yi) {                  // lattice row yi - R of pixel 0 = yi - 1 - R of pixel 1
        const int o = (ly0 + yi * d) * HW + col;
        const uint32_t word = Fs[o];
        f32x4 qv[CV];
#pragma unroll
        for (int q = 0; q < CV; ++q)
          if (q < cvn) qv[q] = Qs[q * HP + o];
        const uint32_t bm = word & 0xffffffu;
        const int bb = crf_dot(bm, bm);
        const bool bv = (word >> 24) != 0u;
#pragma unroll
        for (int k = 0; k < CRF_PY; ++k) {
          const int dyi = yi - k;
          if (dyi >= 0 && dyi < K) {                                 // uniform
            const float ta = tA[dyi * K + dxi], tg = tG[dyi * K + dxi];
            const int c2 = aa[k] + bb - 2 * crf_dot(am[k], bm);
            const float colr = __expf(-(float)c2 * a.inv2b);
            const float kw = fmaf(ta, colr, tg);
            if (ch == 0) z[k] += bv ? ta + tg : 0.f;
#pragma unroll
            for (int q = 0; q < CV; ++q)
              if (q < cvn) {
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[k][c0 + q][c] = fmaf(kw, qv[q][c], acc[k][c0 + q][c]);
              }
          }
        }
      }
    }
  }

  const float qnan = __builtin_nanf("");
  const int lv = a.ldq >> 2;
#pragma unroll
  for (int k = 0; k < CRF_PY; ++k) {
    const int gy = y_base + ly0 + k * d, gx = x_base + tx;
    if (gy >= a.h || gx >= a.w) continue;
    const int64_t p = img_base + (int64_t)gy * a.w + gx;
    float* orow = a.out + p * a.ldq;
    f32x4 t[NV];
    if (own[k]) {
      load_row<NV>(a.logp + p * a.ldq, t);
      const float sc = z[k] > 0.f ? a.strength / z[k] : 0.f;
      float mx = -INFINITY;
#pragma unroll
      for (int q = 0; q < NV; ++q)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          t[q][c] = 4 * q + c < a.classes ? fmaf(acc[k][q][c], sc, t[q][c]) : -INFINITY;
          mx = fmaxf(mx, t[q][c]);
        }
      f32x4 s4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int q = 0; q < NV; ++q)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          t[q][c] = expf(t[q][c] - mx);
          s4[c] += t[q][c];
        }
      const float S = (s4[0] + s4[1]) + (s4[2] + s4[3]);
#pragma unroll
      for (int q = 0; q < NV; ++q) *reinterpret_cast<f32x4*>(orow + 4 * q) = t[q] / S;
    } else {
#pragma unroll
      for (int q = 0; q < NV; ++q) {
        f32x4 o;
#pragma unroll
        for (int c = 0; c < 4; ++c) o[c] = 4 * q + c < a.classes ? qnan : 0.f;
        *reinterpret_cast<f32x4*>(orow + 4 * q) = o;
      }
    }
    for (int q = NV; q < lv; ++q) *reinterpret_cast<f32x4*>(orow + 4 * q) = f32x4{0.f, 0.f, 0.f, 0.f};
  }
}

template <int NV, int CV>
static int launch_crf_step(const CrfArgs& a, long long blocks, int halo_pixels, hipStream_t s) {
  static KernelRec rec("hipFuncSetAttribute(crf_step)", "crf_step_kernel<%d, %d>", NV, CV);
  const double bytes = (double)a.n * a.h * a.w * (12.0 * a.ldq + 4.0);       // logp and Q read, Q written, frame and flag
  return launch_kernel(rec, crf_step_kernel<NV, CV>, dim3((unsigned)blocks), dim3(a.rows * CRF_TW), crf_lds_bytes(halo_pixels, CV),
                       CRF_LDS_BUDGET, s, bytes, "crf_step launch", a);
}

}  // namespace udaseg

using namespace udaseg;

extern "C" int udaseg_crf_tile(int radius, int dilation) {
  if (!crf_window_ok(radius, dilation)) return 0;
  return (crf_thread_rows(dilation) * CRF_PY) << 16 | CRF_TW;
}

extern "C" int udaseg_crf_prepare(const float* scores, int ldc, int classes, int probs, int64_t pixels, float* logp, float* q0, int ldq,
                                  uint8_t* valid, void* stream) {
  if (!scores_args_ok("crf_prepare", pixels, classes, ldc)) return UDASEG_E_BADARG;
  if (!scores_args_ok("crf_prepare", pixels, classes, ldq, INT_MAX, "ldq")) return UDASEG_E_BADARG;
  UDASEG_CHECK_ARG(probs == 0 || probs == 1, "crf_prepare: probs must be 0 (logits) or 1 (probabilities), got %d", probs);
  UDASEG_CHECK_ARG(scores && logp && q0 && valid, "crf_prepare: NULL pointer");
  UDASEG_CHECK_ARG(((reinterpret_cast<uintptr_t>(scores) | reinterpret_cast<uintptr_t>(logp) | reinterpret_cast<uintptr_t>(q0)) & 15) == 0,
                   "crf_prepare: scores, logp and q0 must be 16-byte aligned");
  UDASEG_CHECK_ARG(logp != q0, "crf_prepare: logp and q0 must be two buffers");
  hipStream_t st = as_stream(stream);
  static KernelRec rec(nullptr, "crf_prepare_kernel");
  KTimer kt(rec, st, (double)pixels * (4.0 * ldc + 8.0 * ldq + 1.0));
  const int gx = capped_grid(pixels, CRF_PREP_THREADS, CRF_PREP_MAX_BLOCKS);
  if (!dispatch_width<8>(cdiv(classes, 4), [&](auto w) {
        hipLaunchKernelGGL(crf_prepare_kernel<decltype(w)::value>, dim3(gx), dim3(CRF_PREP_THREADS), 0, st, scores, ldc, classes, probs,
                           pixels, logp, q0, ldq, valid);
      }))
    return unsupported_width("crf_prepare", "classes", classes);
  UDASEG_LAUNCH_CHECK("crf_prepare launch");
  return UDASEG_OK;
}

extern "C" int udaseg_crf_step(const float* logp, const float* q, const uint8_t* valid, const uint8_t* frames, int n, int h, int w,
                               int classes, int ldq, int radius, int dilation, const float* s_alpha, const float* s_gamma, float w_app,
                               float w_smooth, float inv2b, float strength, float* q_out, void* stream) {
  UDASEG_CHECK_ARG(n > 0 && h >= 1 && w >= 1 && (int64_t)h * w < ((int64_t)1 << 31),
                   "crf_step: need n > 0, h, w >= 1, h * w < 2^31 (n=%d h=%d w=%d)", n, h, w);
  if (!scores_args_ok("crf_step", (int64_t)n * h * w, classes, ldq, INT_MAX, "ldq")) return UDASEG_E_BADARG;
  UDASEG_CHECK_ARG(crf_window_ok(radius, dilation),
                   "crf_step: need 1 <= radius <= %d, 1 <= dilation <= %d, radius * dilation <= %d (radius=%d dilation=%d)", CRF_MAX_R,
                   CRF_MAX_D, CRF_MAX_HALO, radius, dilation);
  UDASEG_CHECK_ARG(w_app >= 0.f && w_smooth >= 0.f && w_app + w_smooth > 0.f && w_app + w_smooth < INFINITY,
                   "crf_step: need finite w_app, w_smooth >= 0, not both 0 (w_app=%g w_smooth=%g)", (double)w_app, (double)w_smooth);
  UDASEG_CHECK_ARG(inv2b > 0.f && inv2b < INFINITY, "crf_step: need 0 < inv2b < inf (inv2b=%g)", (double)inv2b);
  UDASEG_CHECK_ARG(strength >= 0.f && strength < INFINITY, "crf_step: need 0 <= strength < inf (strength=%g)", (double)strength);
  UDASEG_CHECK_ARG(logp && q && valid && frames && s_alpha && s_gamma && q_out, "crf_step: NULL pointer");
  UDASEG_CHECK_ARG(((reinterpret_cast<uintptr_t>(logp) | reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(q_out)) & 15) == 0,
                   "crf_step: logp, q and q_out must be 16-byte aligned");
  UDASEG_CHECK_ARG(q != q_out && logp != q_out, "crf_step: q_out must not be q or logp (a Jacobi sweep reads the previous Q)");
  CrfArgs a;
  a.logp = logp, a.q = q, a.valid = valid, a.frames = frames, a.sa = s_alpha, a.sg = s_gamma, a.out = q_out;
  a.n = n, a.h = h, a.w = w, a.classes = classes, a.ldq = ldq, a.R = radius, a.d = dilation;
  a.rows = crf_thread_rows(dilation);
  a.ntx = cdiv(w, CRF_TW), a.nty = cdiv(h, a.rows * CRF_PY);
  a.wa = w_app, a.ws = w_smooth, a.inv2b = inv2b, a.strength = strength;
  const long long blocks = (long long)n * a.nty * a.ntx;
  UDASEG_CHECK_ARG(blocks <= INT_MAX, "crf_step: more than 2^31 - 1 tiles (n=%d h=%d w=%d)", n, h, w);
  const int halo = radius * dilation;
  const int hp = (a.rows * CRF_PY + 2 * halo) * (CRF_TW + 2 * halo);
  const auto fits = [&](int cv) { return crf_lds_bytes(hp, cv) <= CRF_LDS_BUDGET; };
  hipStream_t st = as_stream(stream);
  int rc = UDASEG_OK;
  if (!dispatch_width<8>(cdiv(classes, 4), [&](auto wd) {
        constexpr int NV = decltype(wd)::value;
        if constexpr (NV <= 2) {
          rc = launch_crf_step<NV, NV>(a, blocks, hp, st);
        } else if constexpr (NV == 3) {
          rc = fits(3) ? launch_crf_step<3, 3>(a, blocks, hp, st) : launch_crf_step<3, 2>(a, blocks, hp, st);
        } else {
          rc = fits(NV)  ? launch_crf_step<NV, NV>(a, blocks, hp, st)
               : fits(3) ? launch_crf_step<NV, 3>(a, blocks, hp, st)
                         : launch_crf_step<NV, 2>(a, blocks, hp, st);
        }
      }))
    return unsupported_width("crf_step", "classes", classes);
  return rc;
}
