// Halo-resident weight gradient, second form (round 4): stride-1 3x3 / pad 1 layers, bf16 tensors or fp32 tensors with the exact
// three-term split of conv_halo_f32x3.hip (six v_mfma_f32_32x32x16_bf16 products per operand pair), dW in fp32.
//
//   dW[co][tap][ci] += sum over pixels p of dy[p][co] * x[p + tap][ci]        (reference: loss.backward(), src/models/train.py:343)
//
// What round 3's kernels (conv_wgrad_halo_bf16_kernel / conv_wgrad_halo_f32x3_kernel, removed from conv_wgrad.hip) left on the table, measured
// (profiles/r04_wgrad_v2.txt): (1) the 4-row tile's 144-byte LDS pitch put two of the four pixel rows of every transposed fragment
// read on the same banks -- rocprofv3 SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE = 0.447 on the dominant symbol; (2) every tap
// re-read its own x fragment: 36 LDS reads for 30 MFMAs per 16-pixel K step; (3) the two tap groups of a wave pair shared one
// accumulator array across a wave-uniform branch inside the K loop, which the compiler reconciled with 40 v_mov_b64 + s_nop 10 per
// unrolled iteration.  Here:
//   * LDS holds 32-channel SUB-planes with 64-byte pixel rows: the four pixel rows x 64 bytes one half-wave of a transposed read
//     touches are 256 CONTIGUOUS bytes = every bank once, for any pixel alignment (the tap shift), no padding, no swizzle; sub-plane
//     strides are 64 (mod 128) bytes so that the 16-byte staging stores of a pixel's two channel halves do not collide either;
//   * a wave owns one 32 x 32 (co, ci) quadrant and the taps of ONE OR TWO kernel columns (waves 0-3: dx 0 and 1, waves 4-7: dx 2
//     and all of the staging): the x fragment of halo row r, column shift dx feeds the three taps (dy, dx) of the output rows
//     r, r - 1, r - 2 -- whose dy fragments wait in a three-row register ring -- so a 16-pixel step costs 6 + 6 reads for up to
//     18 / 36 MFMAs (bf16: 2 + 2 for 3 / 6) instead of 6 per tap;
//   * each role runs its own copy of the tile loop (no join inside it): accumulators stay where they are;
//   * blocks smaller than 64 x 64 channels (32 produced channels: the decoder's fourth block; reference smp.Unet decoder_channels
//     (256, 128, 64, 32, 16)) give the spare waves other K steps of the same quadrant (the 16-pixel halves of a row, then row
//     ranges), each wave adding its partial tile with its own atomics;
//   * 16-pixel-wide images (r18 layer4 at 512^2) take 8 x 16 pixel tiles (one K step per row) -- round 3 left them on the fp32
//     split-K kernel.
// Blocks are few and long-lived as before (one set of fp32 atomics per wave per launch, ~120 blocks beside the main stream's chain).
#include <stdlib.h>

#include <type_traits>

#include "common.h"
#include "halo_common.h"
#include "launch.h"

namespace udaseg {

typedef short h2_s16x4 __attribute__((ext_vector_type(4)));
typedef short h2_s16x8 __attribute__((ext_vector_type(8)));

struct WgradH2Args {
  const void* x;      // [n][h][w][cx], or the half-resolution a [n][h/2][w/2][up_ca] of a fused decoder input
  const void* x2;     // fused decoder input: the skip tensor [n][h][w][ci - up_ca]
  const void* dy;     // [n][h][w][co]
  float* dw;          // [co][9][ldw] fp32, accumulated onto: channels [dw_coff, dw_coff + ci) of every row (ldw = ci, dw_coff = 0: the whole row)
  int ldw, dw_coff;
  int n, h, w, ci, co, up_ca;
  int ntx, nty, ntiles, ncib, pairs, P;
  unsigned x_bytes, x2_bytes, dy_bytes;
  // fp32, single plain source: x is the raw output of a conv + BatchNorm + activation layer whose activation was never written
  // (engine.LazyAct); the staging applies act(fma(x, in_scale[c], in_shift[c])) -- bn_apply's arithmetic -- to the pieces inside
  // the image before the split.  null: x is used as it is.
  const float* in_scale;
  const float* in_shift;
  int in_act;
  float in_slope;
  unsigned long long* timeline;   // diagnosis (udaseg_debug_set_timeline, TL instantiation only): per (block, role) 8 x u64
};
extern unsigned long long* g_timeline;      // conv_igemm.hip
extern int g_timeline_blocks;

constexpr int h2_pad(int bytes) { return (bytes / 64) % 2 == 0 ? bytes + 64 : bytes; }     // sub-plane stride: 64 (mod 128)

template <int PL_, int COQ_, int CIQ_, int TR_, int TWK_, int NSTW_, bool DB_ = false>
struct H2 {
  static constexpr int PL = PL_, COQ = COQ_, CIQ = CIQ_, TR = TR_, TWK = TWK_, NSTW = NSTW_;
  static constexpr bool DB = DB_;                                  // two LDS buffers: tile t + 1 is staged during the MFMAs of tile t
  static constexpr int NT = 512;
  static constexpr int COB = 32 * COQ, CIB = 32 * CIQ, TW = 16 * TWK;
  static constexpr int HR = TR + 2, HWD = TW + 2, HP = HR * HWD, TP = TR * TW;
  static constexpr int NQ = COQ * CIQ, KS = 4 / NQ;                // waves per tap group that share a quadrant (K split)
  static constexpr int KSH = KS < TWK ? KS : TWK;                  // ... over the 16-pixel halves of a row
  static constexpr int KSR = KS / KSH;                             // ... and over row ranges
  static constexpr int RW = TR / KSR, NHF = TWK / KSH;
  static constexpr int XSP = h2_pad(HP * 64), DSP = h2_pad(TP * 64);          // bytes per 32-channel sub-plane
  static constexpr int XPLANE = CIQ * XSP, DPLANE = COQ * DSP;
  static constexpr int BUF = PL * (XPLANE + DPLANE);               // one buffer: the split planes of an x halo and a dy tile
  static constexpr int LDS = (DB ? 2 : 1) * BUF;
  static constexpr int ES = PL == 3 ? 4 : 2;                       // bytes per element in HBM
  static constexpr int NST = 64 * NSTW;                            // staging threads: the LAST NSTW waves
  static constexpr int XO = CIB / 8, DO = COB / 8;                 // 8-channel pieces per pixel
  static constexpr int XPC = HP * XO, DPC = TP * DO;
  static constexpr int NX = (XPC + NST - 1) / NST, ND = (DPC + NST - 1) / NST;
  static constexpr int LPP = PL == 3 ? 2 : 1;                      // 16-byte loads per piece
  static_assert(NQ == 1 || NQ == 2 || NQ == 4, "1, 2 or 4 quadrants");
  static_assert(TR % KSR == 0 && TWK % KSH == 0 && KSH * KSR == KS, "K split tiles the tile");
  static_assert(NSTW == 4 || NSTW == 8, "staging by waves 4-7 or by all");
  static_assert(LDS <= 160 * 1024, "LDS");
};

__device__ __forceinline__ bf16x8 h2_tr_fragment(const char* p) {
  // this lane's address in the first 4-pixel block of a 16-pixel K step; the second block is 4 pixel rows (256 bytes) further
  const h2_s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((h2_s16x4 __attribute__((address_space(3)))*)(p));
  const h2_s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((h2_s16x4 __attribute__((address_space(3)))*)(p + 256));
  const h2_s16x8 f = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(bf16x8, f);
}

// One role of a block: the tile loop of the waves that own kernel columns DX0 .. DX0 + NDX - 1; STG: these waves also stage.
template <typename C, int DX0, int NDX, bool STG, bool TL, bool XFT = false>
__device__ __forceinline__ void wgrad_h2_role(const WgradH2Args& a, char* smem, int tid, int lane, int wave) {
  constexpr int PL = C::PL;
  char* const Xs = smem;
  char* const Ds = smem + PL * C::XPLANE;
  const int lr = lane & 31, lh = lane >> 5;
  const int grp = lane >> 4, cb = 16 * (grp & 1), hk = grp >> 1, tq = (lane & 15) >> 2, tp = lane & 3;
  const int q = wave & 3;
  const int qi = q % C::NQ, ks = q / C::NQ;
  const int coq = qi / C::CIQ, ciq = qi % C::CIQ;
  const int ksh = ks % C::KSH, r0 = (ks / C::KSH) * C::RW;
  const int pair = (int)blockIdx.x % a.pairs, split = (int)blockIdx.x / a.pairs;
  const int cob = pair / a.ncib, cib = pair % a.ncib;
  const int H = a.h, W = a.w;

  // ---- staging (register-staged: the next tile's loads are in flight during the MFMA phase)
  const bool UPC = a.up_ca > 0;
  const bool second = UPC && cib * C::CIB >= a.up_ca;
  const int cx = UPC ? (second ? a.ci - a.up_ca : a.up_ca) : a.ci;          // channels of the tensor read
  const int c0 = second ? cib * C::CIB - a.up_ca : cib * C::CIB;
  const bool half_res = UPC && !second;
  __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(second ? a.x2 : a.x), 0,
                                                                  (int)(second ? a.x2_bytes : a.x_bytes), 0x00020000);
  __amdgpu_buffer_rsrc_t rs_d = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.dy), 0, (int)a.dy_bytes, 0x00020000);
  const int st = tid - (C::NT - C::NST);
  u32x4 sx[STG ? C::NX : 1][C::LPP], sd[STG ? C::ND : 1][C::LPP];
  // in-staging transform of x (WgradH2Args::in_scale): a staging thread's 8-channel piece is the same for every piece it owns
  // (NST is a multiple of the pieces per pixel), so its coefficients live in registers; x_in: bit i = piece i is inside the image
  constexpr bool XF = XFT && PL == 3 && STG;          // its own instantiation: the plain launches carry none of this
  static_assert(C::NST % C::XO == 0, "one channel octet per staging thread");
  unsigned x_in = 0;
  f32x4 xsc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}}, xsh[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  if constexpr (XF) {
    const int ch = c0 + (st % C::XO) * 8;
    xsc[0] = *reinterpret_cast<const f32x4*>(a.in_scale + ch);
    xsc[1] = *reinterpret_cast<const f32x4*>(a.in_scale + ch + 4);
    xsh[0] = *reinterpret_cast<const f32x4*>(a.in_shift + ch);
    xsh[1] = *reinterpret_cast<const f32x4*>(a.in_shift + ch + 4);
  }
  auto load_tile = [&](int tile) {
    if constexpr (STG) {
      x_in = 0;
      const int tx = tile % a.ntx;
      const int t2 = tile / a.ntx;
      const int ty = t2 % a.nty, img = t2 / a.nty;
      const int y0 = ty * C::TR, x0 = tx * C::TW;
#pragma unroll
      for (int i = 0; i < C::NX; ++i) {
        const int pc = st + i * C::NST;
        const int pix = pc / C::XO, oct = pc % C::XO;
        const int hy = pix / C::HWD, hx = pix - hy * C::HWD;
        const int iy = y0 + hy - 1, ix = x0 + hx - 1;
        const bool ok = pc < C::XPC && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
        const int p = half_res ? (img * (H >> 1) + (iy >> 1)) * (W >> 1) + (ix >> 1) : (img * H + iy) * W + ix;
        const unsigned off = ok ? (unsigned)((p * cx + c0 + oct * 8) * C::ES) : 0x80000000u;
        if constexpr (XF) x_in |= (ok ? 1u : 0u) << i;
#pragma unroll
        for (int l = 0; l < C::LPP; ++l) sx[i][l] = __builtin_amdgcn_raw_buffer_load_b128(rs_x, (int)off, 16 * l, 0);
      }
#pragma unroll
      for (int i = 0; i < C::ND; ++i) {
        const int pc = st + i * C::NST;
        const int pix = pc / C::DO, oct = pc % C::DO;
        const int oy = y0 + pix / C::TW, ox = x0 + pix % C::TW;
        const bool ok = pc < C::DPC && oy < H && ox < W;
        const unsigned off = ok ? (unsigned)((((img * H + oy) * W + ox) * a.co + cob * C::COB + oct * 8) * C::ES) : 0x80000000u;
#pragma unroll
        for (int l = 0; l < C::LPP; ++l) sd[i][l] = __builtin_amdgcn_raw_buffer_load_b128(rs_d, (int)off, 16 * l, 0);
      }
    }
  };
  auto store_piece = [&](char* dst, int plane_bytes, const u32x4 (&v)[C::LPP], unsigned sgn = 0u) {
    if constexpr (PL == 3) {
      u32x4 p0, p1, p2;
      split3(v[0] ^ sgn, v[C::LPP - 1] ^ sgn, p0, p1, p2);      // sgn = 0x80000000: the terms of -v are minus the terms of v
      *reinterpret_cast<u32x4*>(dst) = p0;
      *reinterpret_cast<u32x4*>(dst + plane_bytes) = p1;
      *reinterpret_cast<u32x4*>(dst + 2 * plane_bytes) = p2;
    } else {
      *reinterpret_cast<u32x4*>(dst) = v[0];
    }
  };
  // fp32 (PL == 3): the tiles [q1, q3) of this block's sequence are staged as -dy and accumulated on a negated accumulator, + - - +
  // like the forward kernels' K loop (halo_common.h f3_negated_groups: the bf16 MFMA adder truncates toward minus infinity, and a
  // weight gradient sums ~1000 pixels per block on top of the atomics)
  const int nseq = split < a.ntiles ? (a.ntiles - split + a.P - 1) / a.P : 0;
  const int sq1 = PL == 3 ? (nseq + 2) / 4 : 0, sq3 = PL == 3 ? nseq - sq1 : 0;
  auto store_tile = [&](int bo, int seq) {          // bo: byte offset of the LDS buffer; seq: the staged tile's place in the sequence
    const unsigned dsgn = (seq >= sq1 && seq < sq3) ? 0x80000000u : 0u;
    if constexpr (STG) {
#pragma unroll
      for (int i = 0; i < C::NX; ++i) {
        const int pc = st + i * C::NST;
        const int pix = pc / C::XO, oct = pc % C::XO;
        if constexpr (XF) {
          {
            const bool in = (x_in >> i) & 1u;
#pragma unroll
            for (int l = 0; l < 2; ++l) {
              f32x4 v = __builtin_bit_cast(f32x4, sx[i][l]);
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                const float t = act_apply(__builtin_fmaf(v[e], xsc[l][e], xsh[l][e]), a.in_act, a.in_slope);
                v[e] = in ? t : 0.f;
              }
              sx[i][l] = __builtin_bit_cast(u32x4, v);
            }
          }
        }
        if (i < C::NX - 1 || pc < C::XPC) store_piece(Xs + bo + (oct >> 2) * C::XSP + pix * 64 + (oct & 3) * 16, C::XPLANE, sx[i]);
      }
#pragma unroll
      for (int i = 0; i < C::ND; ++i) {
        const int pc = st + i * C::NST;
        const int pix = pc / C::DO, oct = pc % C::DO;
        if (i < C::ND - 1 || pc < C::DPC) store_piece(Ds + bo + (oct >> 2) * C::DSP + pix * 64 + (oct & 3) * 16, C::DPLANE, sd[i], dsgn);
      }
    }
  };

  f32x16 acc[3 * NDX];        // [dy][dxi]
#pragma unroll
  for (int t = 0; t < 3 * NDX; ++t)
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[t][v] = 0.f;

  // this lane's byte address inside a 16-pixel K step (transposed reads), at this wave's first row / first half
  const int lane_off = (8 * hk + tq) * 64 + (cb + 4 * tp) * 2;
  const char* const dbase0 = Ds + coq * C::DSP + (r0 * C::TW + 16 * ksh) * 64 + lane_off;
  const char* const xbase0 = Xs + ciq * C::XSP + (r0 * C::HWD + 16 * ksh + DX0) * 64 + lane_off;

  // TL: shader-clock cycles this wave spends per phase, summed over its tiles (s_memtime at the phase boundaries, where the
  // LDS counter is drained anyway), and the launch's wall-clock ticks for the clock the chip held
  unsigned long long c_store = 0, c_b1 = 0, c_mfma = 0, c_b2 = 0, t0 = 0, t1 = 0, t2 = 0, t3 = 0, tw0 = 0, tc0 = 0;
  int ntl = 0;
  if constexpr (TL) {
    tw0 = __builtin_amdgcn_s_memrealtime();
    tc0 = __builtin_amdgcn_s_memtime();
  }
  int cur = 0;                     // DB: byte offset of the buffer the MFMAs of this iteration read
  if (split < a.ntiles) load_tile(split);
  if constexpr (C::DB) {
    // two buffers: the staging waves split tile t + 1 into the OTHER buffer while every wave's MFMAs read tile t (their vector
    // instructions issue beside the older waves' MFMAs), and request tile t + 2; ONE barrier per tile
    store_tile(0, 0);
    if (split + a.P < a.ntiles) load_tile(split + a.P);
    __syncthreads();
  }
  int seq = 0;
  bool negated = false;
  for (int tile = split; tile < a.ntiles; tile += a.P, ++seq) {
    if constexpr (TL) t0 = __builtin_amdgcn_s_memtime();
    if constexpr (PL == 3) {
      if ((seq >= sq1 && seq < sq3) != negated) {        // uniform; twice per block
        negated = !negated;
#pragma unroll
        for (int t = 0; t < 3 * NDX; ++t) acc[t] = -acc[t];
      }
    }
    if constexpr (C::DB) {
      if (tile + a.P < a.ntiles) {
        store_tile(cur ^ C::BUF, seq + 1);
        if (tile + 2 * a.P < a.ntiles) load_tile(tile + 2 * a.P);
      }
      if constexpr (TL) t1 = t2 = __builtin_amdgcn_s_memtime();
    } else {
      store_tile(0, seq);
      if constexpr (TL) t1 = __builtin_amdgcn_s_memtime();
      __syncthreads();
      if constexpr (TL) t2 = __builtin_amdgcn_s_memtime();
      if (tile + a.P < a.ntiles) load_tile(tile + a.P);
    }
    const char* const dbase = dbase0 + cur;
    const char* const xbase = xbase0 + cur;
    if constexpr (C::DB) cur ^= C::BUF;
#pragma unroll
    for (int hfi = 0; hfi < C::NHF; ++hfi) {
      bf16x8 A[3][PL];
#pragma unroll
      for (int rr = 0; rr < C::RW + 2; ++rr) {
        if (rr < C::RW) {
#pragma unroll
          for (int pl = 0; pl < PL; ++pl)
            A[rr % 3][pl] = h2_tr_fragment(dbase + pl * C::DPLANE + (rr * C::TW + 16 * C::KSH * hfi) * 64);
        }
        bf16x8 B[NDX][PL];
#pragma unroll
        for (int dxi = 0; dxi < NDX; ++dxi)
#pragma unroll
          for (int pl = 0; pl < PL; ++pl)
            B[dxi][pl] = h2_tr_fragment(xbase + pl * C::XPLANE + (rr * C::HWD + 16 * C::KSH * hfi + dxi) * 64);
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
          const int j = rr - dy;               // output row (relative to r0) whose tap (dy, dx) reads halo row rr
          if (j >= 0 && j < C::RW) {
#pragma unroll
            for (int dxi = 0; dxi < NDX; ++dxi) {
              if constexpr (PL == 3) {
                // smallest terms first: (dy piece i) x (x piece ij - i), i + j <= 2
#pragma unroll
                for (int ij = 2; ij >= 0; --ij)
#pragma unroll
                  for (int i = 0; i <= ij; ++i)
                    acc[dy * NDX + dxi] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[j % 3][i], B[dxi][ij - i], acc[dy * NDX + dxi], 0, 0, 0);
              } else {
                acc[dy * NDX + dxi] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[j % 3][0], B[dxi][0], acc[dy * NDX + dxi], 0, 0, 0);
              }
            }
          }
        }
      }
    }
    if constexpr (TL) t3 = __builtin_amdgcn_s_memtime();
    __syncthreads();
    if constexpr (TL) {
      const unsigned long long t4 = __builtin_amdgcn_s_memtime();
      c_store += t1 - t0; c_b1 += t2 - t1; c_mfma += t3 - t2; c_b2 += t4 - t3;
      ++ntl;
    }
  }
  if constexpr (TL) {
    if (a.timeline != nullptr && lane == 0 && (wave & 3) == 0) {
      unsigned long long* t = a.timeline + ((size_t)blockIdx.x * 2 + (wave >> 2)) * 8;
      t[0] = c_store; t[1] = c_b1; t[2] = c_mfma; t[3] = c_b2;
      t[4] = __builtin_amdgcn_s_memtime() - tc0; t[5] = __builtin_amdgcn_s_memrealtime() - tw0; t[6] = (unsigned long long)ntl;
      t[7] = 1;
    }
  }

  if (negated) {      // a sequence too short for the pattern to close (one or two tiles)
#pragma unroll
    for (int t = 0; t < 3 * NDX; ++t) acc[t] = -acc[t];
  }
  // dW[co][tap][ci] += acc: register v of a tap = one co row, 32 consecutive ci per half-wave (two 128-byte segments per
  // wave-instruction: the full-rate shape of the memory-side float atomics)
  const int ci_g = cib * C::CIB + ciq * 32 + lr;
#pragma unroll
  for (int dy = 0; dy < 3; ++dy)
#pragma unroll
    for (int dxi = 0; dxi < NDX; ++dxi)
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int co_g = cob * C::COB + coq * 32 + (v & 3) + 8 * (v >> 2) + 4 * lh;
        atomicAdd(a.dw + ((size_t)co_g * 9 + dy * 3 + DX0 + dxi) * a.ldw + a.dw_coff + ci_g, acc[dy * NDX + dxi][v]);
      }
}

template <int PL, int COQ, int CIQ, int TR, int TWK, int NSTW, bool DB, bool TL = false, bool XF = false>
__global__ __launch_bounds__(512, 2) void conv_wgrad_h2_kernel(const WgradH2Args a) {
  using C = H2<PL, COQ, CIQ, TR, TWK, NSTW, DB>;
  extern __shared__ __attribute__((aligned(16))) char h2smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  if (wave < 4) wgrad_h2_role<C, 0, 2, NSTW == 8, TL, XF>(a, h2smem, tid, lane, wave);
  else wgrad_h2_role<C, 2, 1, true, TL, XF>(a, h2smem, tid, lane, wave);
}

// ------------------------------------------------------------------------------------------------------------------------------------
// Pair-packed form for 16-channel tensors (the full-resolution decoder tail: block-5 conv2 16 -> 16, the head 16 -> 24).  A
// 16-channel NHWC row of W pixels is, byte for byte, a 32-channel row of W / 2 pixel PAIRS, so the 32 x 32 x 16 MFMA of the kernel
// above runs on it with k = one pair:
//     A[m][k] = dy[2k + (m >= 16)][m % 16]        B[k][n] = x[2k + s + (n >= 16)][n % 16]         (s: the group's shift in pixels)
// and the four 16 x 16 blocks of the accumulator are  (m<16, n<16): tap s over the even pixels,  (m>=16, n>=16): tap s over the odd
// pixels,  (m<16, n>=16): tap s + 1 over the even pixels,  (m>=16, n<16): tap s - 1 over the odd pixels.  Two shift groups give the
// three kernel columns: s = -1 holds column 0 (both diagonal blocks) and the even half of column 1, s = +1 column 2 and the odd half
// of column 1; the (m>=16, n<16) block of s = -1 and the (m<16, n>=16) block of s = +1 are the offsets -2 / +2 and are dropped in the
// epilogue.  36 MFMAs per 32 pixels, 75 % of them useful (plain channel padding to 32 x 32: 25 %).
// LDS planes are linear pixel arrays of 32 bytes (16 bf16) per pixel: halo pixel hx of a row is image column x0 + hx - 1, so group
// s = -1 reads its 64-byte pair rows from byte 0 of the row and s = +1 from byte 64 -- every transposed read still covers 256
// contiguous bytes.  Zero padding comes from the halo's range-checked loads, ragged tiles from dy's: no edge fix-up.
// Waves: group = wave & 1, the other four split the tile's K (the two 32-pixel halves of a 64-pixel row x two row ranges); all
// eight stage (register-staged, two LDS buffers, one barrier per tile) and all eight run MFMAs.  Blocks of 16 produced channels:
// a layer with 24 has two, the second half empty (its dy pieces load as zero, its dW rows are never written).
template <int TR_, int TWK_>
struct H2P {
  static constexpr int PL = 3, TR = TR_, TWK = TWK_;               // TWK: 16-pair (32-pixel) K steps per tile row
  static constexpr bool UP = false;
  static constexpr int NT = 512;
  static constexpr int TW = 32 * TWK, HR = TR + 2, HWD = TW + 2, HP = HR * HWD, TP = TR * TW;
  static constexpr int KS = 4;                                     // waves per shift group
  static constexpr int KSH = KS < TWK ? KS : TWK, KSR = KS / KSH;
  static constexpr int RW = TR / KSR, NHF = TWK / KSH;
  static constexpr int XPLANE = HP * 32, DPLANE = TP * 32;         // bytes per split plane
  static constexpr int BUF = PL * (XPLANE + DPLANE);
  static constexpr int LDS = 2 * BUF;
  static constexpr int XPC = HP * 2, DPC = TP * 2;                 // 8-channel pieces
  static constexpr int NX = (XPC + NT - 1) / NT, ND = (DPC + NT - 1) / NT;
  static_assert(TR % KSR == 0 && TWK % KSH == 0 && KSH * KSR == KS, "K split tiles the tile");
  static_assert(LDS <= 160 * 1024 && 6 * 24 * 64 * 4 <= LDS, "LDS");
};

template <typename C, bool XF>
__device__ __forceinline__ void wgrad_h2p_role(const WgradH2Args& a, char* smem, int tid, int lane, int wave) {
  constexpr int PL = 3;
  char* const Xs = smem;
  char* const Ds = smem + PL * C::XPLANE;
  const int lr = lane & 31, lh = lane >> 5;
  const int grp = lane >> 4, cb = 16 * (grp & 1), hk = grp >> 1, tq = (lane & 15) >> 2, tp = lane & 3;
  const int sg = wave & 1, ks = wave >> 1;                          // shift group (0: s = -1, 1: s = +1), K share
  const int ksh = ks % C::KSH, r0 = (ks / C::KSH) * C::RW;
  const int cob = (int)blockIdx.x % a.pairs, split = (int)blockIdx.x / a.pairs;
  const int H = a.h, W = a.w;
  __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.x), 0, (int)a.x_bytes, 0x00020000);
  __amdgpu_buffer_rsrc_t rs_d = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.dy), 0, (int)a.dy_bytes, 0x00020000);
  u32x4 sx[C::NX][2], sd[C::ND][2];
  // in-staging transform of x: a thread's channel octet is the same for every piece it owns (NT is even)
  unsigned x_in = 0;
  f32x4 xsc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}}, xsh[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  if constexpr (XF) {
    const int ch = (tid & 1) * 8;
    xsc[0] = *reinterpret_cast<const f32x4*>(a.in_scale + ch);
    xsc[1] = *reinterpret_cast<const f32x4*>(a.in_scale + ch + 4);
    xsh[0] = *reinterpret_cast<const f32x4*>(a.in_shift + ch);
    xsh[1] = *reinterpret_cast<const f32x4*>(a.in_shift + ch + 4);
  }
  const int dch = cob * 16 + (tid & 1) * 8;                         // this thread's dy channel octet; >= co: the empty half of a block
  auto load_tile = [&](int tile) {
    x_in = 0;
    const int tx = tile % a.ntx;
    const int t2 = tile / a.ntx;
    const int ty = t2 % a.nty, img = t2 / a.nty;
    const int y0 = ty * C::TR, x0 = tx * C::TW;
#pragma unroll
    for (int i = 0; i < C::NX; ++i) {
      const int pc = tid + i * C::NT;
      const int pix = pc >> 1, oct = pc & 1;
      const int hy = pix / C::HWD, hx = pix - hy * C::HWD;
      const int iy = y0 + hy - 1, ix = x0 + hx - 1;
      const bool ok = pc < C::XPC && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
      const unsigned off = ok ? (unsigned)((((img * H + iy) * W + ix) * 16 + oct * 8) * 4) : 0x80000000u;
      if constexpr (XF) x_in |= (ok ? 1u : 0u) << i;
#pragma unroll
      for (int l = 0; l < 2; ++l) sx[i][l] = __builtin_amdgcn_raw_buffer_load_b128(rs_x, (int)off, 16 * l, 0);
    }
#pragma unroll
    for (int i = 0; i < C::ND; ++i) {
      const int pc = tid + i * C::NT;
      const int pix = pc >> 1;
      const int oy = y0 + pix / C::TW, ox = x0 + pix % C::TW;
      const bool ok = pc < C::DPC && oy < H && ox < W && dch < a.co;
      const unsigned off = ok ? (unsigned)((((img * H + oy) * W + ox) * a.co + dch) * 4) : 0x80000000u;
#pragma unroll
      for (int l = 0; l < 2; ++l) sd[i][l] = __builtin_amdgcn_raw_buffer_load_b128(rs_d, (int)off, 16 * l, 0);
    }
  };
  auto store_piece = [&](char* dst, int plane_bytes, const u32x4 (&v)[2], unsigned sgn) {
    u32x4 p0, p1, p2;
    split3(v[0] ^ sgn, v[1] ^ sgn, p0, p1, p2);
    *reinterpret_cast<u32x4*>(dst) = p0;
    *reinterpret_cast<u32x4*>(dst + plane_bytes) = p1;
    *reinterpret_cast<u32x4*>(dst + 2 * plane_bytes) = p2;
  };
  const int nseq = split < a.ntiles ? (a.ntiles - split + a.P - 1) / a.P : 0;
  const int sq1 = (nseq + 2) / 4, sq3 = nseq - sq1;               // + - - + over the block's tile sequence (see wgrad_h2_role)
  auto store_tile = [&](int bo, int seq) {
    const unsigned dsgn = (seq >= sq1 && seq < sq3) ? 0x80000000u : 0u;
#pragma unroll
    for (int i = 0; i < C::NX; ++i) {
      const int pc = tid + i * C::NT;
      if constexpr (XF) {
        const bool in = (x_in >> i) & 1u;
#pragma unroll
        for (int l = 0; l < 2; ++l) {
          f32x4 v = __builtin_bit_cast(f32x4, sx[i][l]);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float t = act_apply(__builtin_fmaf(v[e], xsc[l][e], xsh[l][e]), a.in_act, a.in_slope);
            v[e] = in ? t : 0.f;
          }
          sx[i][l] = __builtin_bit_cast(u32x4, v);
        }
      }
      if (i < C::NX - 1 || pc < C::XPC) store_piece(Xs + bo + pc * 16, C::XPLANE, sx[i], 0u);
    }
#pragma unroll
    for (int i = 0; i < C::ND; ++i) {
      const int pc = tid + i * C::NT;
      if (i < C::ND - 1 || pc < C::DPC) store_piece(Ds + bo + pc * 16, C::DPLANE, sd[i], dsgn);
    }
  };

  f32x16 acc[3];        // [kernel row]
#pragma unroll
  for (int t = 0; t < 3; ++t)
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[t][v] = 0.f;

  const int lane_off = (8 * hk + tq) * 64 + (cb + 4 * tp) * 2;
  const char* const dbase0 = Ds + (r0 * C::TW + 32 * ksh) * 32 + lane_off;
  const char* const xbase0 = Xs + (r0 * C::HWD + 32 * ksh + 2 * sg) * 32 + lane_off;

  int cur = 0;
  if (split < a.ntiles) load_tile(split);
  store_tile(0, 0);
  if (split + a.P < a.ntiles) load_tile(split + a.P);
  __syncthreads();
  int seq = 0;
  bool negated = false;
  for (int tile = split; tile < a.ntiles; tile += a.P, ++seq) {
    if ((seq >= sq1 && seq < sq3) != negated) {
      negated = !negated;
#pragma unroll
      for (int t = 0; t < 3; ++t) acc[t] = -acc[t];
    }
    if (tile + a.P < a.ntiles) {
      store_tile(cur ^ C::BUF, seq + 1);
      if (tile + 2 * a.P < a.ntiles) load_tile(tile + 2 * a.P);
    }
    const char* const dbase = dbase0 + cur;
    const char* const xbase = xbase0 + cur;
    cur ^= C::BUF;
#pragma unroll
    for (int hfi = 0; hfi < C::NHF; ++hfi) {
      bf16x8 A[3][PL];
#pragma unroll
      for (int rr = 0; rr < C::RW + 2; ++rr) {
        if (rr < C::RW) {
#pragma unroll
          for (int pl = 0; pl < PL; ++pl)
            A[rr % 3][pl] = h2_tr_fragment(dbase + pl * C::DPLANE + (rr * C::TW + 32 * C::KSH * hfi) * 32);
        }
        bf16x8 B[PL];
#pragma unroll
        for (int pl = 0; pl < PL; ++pl) B[pl] = h2_tr_fragment(xbase + pl * C::XPLANE + (rr * C::HWD + 32 * C::KSH * hfi) * 32);
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
          const int j = rr - ky;               // output row (relative to r0) whose kernel row ky reads halo row rr
          if (j >= 0 && j < C::RW) {
#pragma unroll
            for (int ij = 2; ij >= 0; --ij)
#pragma unroll
              for (int i = 0; i <= ij; ++i)
                acc[ky] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[j % 3][i], B[ij - i], acc[ky], 0, 0, 0);
          }
        }
      }
    }
    __syncthreads();
  }
  if (negated) {
#pragma unroll
    for (int t = 0; t < 3; ++t) acc[t] = -acc[t];
  }
  // accumulator -> taps.  Register v < 8 of lane (lh, lr) is row m = (v & 3) + 8 (v >> 2) + 4 lh < 16, column n = lr; register v + 8
  // is row m + 16.  One exchange across lr ^ 16 brings the odd-pixel blocks to the lanes that hold their even-pixel partners:
  //   s = -1: lanes n < 16 add (m + 16, n + 16) -> column 0;  lanes n >= 16 keep (m, n) -> column 1;  (m + 16, n < 16) is dropped
  //   s = +1: lanes n < 16 add (m + 16, n + 16) -> column 2;  lanes n >= 16 take (m + 16, n - 16) -> column 1;  (m, n >= 16) is dropped
  // The four K shares of a shift group meet in LDS (free after the last tile) before ONE set of atomics per block and group: the
  // rounding of the fp32 atomics onto a growing dW is what a long sum's error is made of, a quarter of the partials halves it.
  const bool lo = lr < 16;
  float out[24];
#pragma unroll
  for (int ky = 0; ky < 3; ++ky)
#pragma unroll
    for (int v = 0; v < 8; ++v) {
      const float other = __shfl_xor(acc[ky][v + 8], 16);
      out[ky * 8 + v] = lo ? acc[ky][v] + other : (sg ? other : acc[ky][v]);
    }
  float* const red = reinterpret_cast<float*>(smem);                 // [3 shares][2 groups][24][64 lanes]
  if (ks != 0) {
#pragma unroll
    for (int j = 0; j < 24; ++j) red[(((ks - 1) * 2 + sg) * 24 + j) * 64 + lane] = out[j];
  }
  __syncthreads();
  if (ks != 0) return;
#pragma unroll
  for (int k2 = 0; k2 < 3; ++k2)
#pragma unroll
    for (int j = 0; j < 24; ++j) out[j] += red[((k2 * 2 + sg) * 24 + j) * 64 + lane];
  const int ci_g = lr & 15;
  const int kx = lo ? 2 * sg : 1;
#pragma unroll
  for (int ky = 0; ky < 3; ++ky)
#pragma unroll
    for (int v = 0; v < 8; ++v) {
      const int co_g = cob * 16 + (v & 3) + 8 * (v >> 2) + 4 * lh;
      if (co_g < a.co) atomicAdd(a.dw + ((size_t)co_g * 9 + ky * 3 + kx) * a.ldw + a.dw_coff + ci_g, out[ky * 8 + v]);
    }
}

// The same for a decoder conv1 WITHOUT a skip half whose 32 gathered channels are the nearest x2 up-sampling of `a` (block 5:
// 32 -> 16 at full resolution).  dy is paired as above; x has 32 channels, so B carries one pixel per k:
//     B[k][n] = x_up[2k + s][n] = a[y >> 1][j + floor(s / 2)][n]
// -- contiguous pixel rows of the half-resolution source, shifted by e = floor(s / 2) in {-1, 0, +1}.  The shifts s = 0 and s = 1 read
// the same rows of `a` and therefore ARE the same product: three products e = -1, 0, +1 stand for the four shift groups,
//     column 0 = P(-1)[m<16] + P(0)[m>=16]      column 1 = P(0)[m<16] + P(0)[m>=16]      column 2 = P(0)[m<16] + P(+1)[m>=16]
// (m < 16: the even pixels, m >= 16: the odd ones; P(-1)[m>=16] and P(+1)[m<16] are the offsets -2 / +2 and are dropped).  Rows
// repeat in the same way: the three kernel rows of an output row y read only two rows of `a` -- (y >> 1) + py - 1 + u, u in {0, 1},
// py = y & 1 -- which stand for the kernel rows {0}, {1, 2} (py = 0) or {0, 1}, {2} (py = 1).  A wave owns one output row of the
// 4 x 64 pixel tile's parity py = wave & 1 and one 32-pixel half of it: 2 x 3 accumulators, 36 MFMAs per tile like the form above.
template <int TR_, int TWK_>
struct H2PU {
  static constexpr int PL = 3, TR = TR_, TWK = TWK_;
  static constexpr bool UP = true;
  static constexpr int NT = 512;
  static constexpr int TW = 32 * TWK, AR = TR / 2 + 2, AW = TW / 2 + 2, AP = AR * AW, TP = TR * TW;      // halo of `a`: AR rows x AW pixels
  static constexpr int XPLANE = AP * 64, DPLANE = TP * 32;
  static constexpr int BUF = PL * (XPLANE + DPLANE);
  static constexpr int LDS = 2 * BUF;
  static constexpr int XPC = AP * 4, DPC = TP * 2;
  static constexpr int NX = (XPC + NT - 1) / NT, ND = (DPC + NT - 1) / NT;
  static_assert(TR % 2 == 0 && (TR / 2) * TWK == 4, "one (row, half) of each parity per wave");
  static_assert(LDS <= 160 * 1024 && 6 * 48 * 64 * 4 <= LDS, "LDS");
};

template <typename C>
__device__ __forceinline__ void wgrad_h2pu_role(const WgradH2Args& a, char* smem, int tid, int lane, int wave) {
  constexpr int PL = 3;
  char* const Xs = smem;
  char* const Ds = smem + PL * C::XPLANE;
  const int lr = lane & 31, lh = lane >> 5;
  const int grp = lane >> 4, cb = 16 * (grp & 1), hk = grp >> 1, tq = (lane & 15) >> 2, tp = lane & 3;
  const int py = wave & 1, ks = wave >> 1;
  const int ksh = ks % C::TWK, rsel = ks / C::TWK;                  // this wave's output row of the tile: 2 rsel + py
  const int split = (int)blockIdx.x;
  const int H = a.h, W = a.w, HA = a.h >> 1, WA = a.w >> 1;
  __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.x), 0, (int)a.x_bytes, 0x00020000);
  __amdgpu_buffer_rsrc_t rs_d = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.dy), 0, (int)a.dy_bytes, 0x00020000);
  u32x4 sx[C::NX][2], sd[C::ND][2];
  auto load_tile = [&](int tile) {
    const int tx = tile % a.ntx;
    const int t2 = tile / a.ntx;
    const int ty = t2 % a.nty, img = t2 / a.nty;
    const int y0 = ty * C::TR, x0 = tx * C::TW;
#pragma unroll
    for (int i = 0; i < C::NX; ++i) {
      const int pc = tid + i * C::NT;
      const int pix = pc >> 2, oct = pc & 3;
      const int hy = pix / C::AW, hx = pix - hy * C::AW;
      const int iy = (y0 >> 1) + hy - 1, ix = (x0 >> 1) + hx - 1;
      const bool ok = pc < C::XPC && (unsigned)iy < (unsigned)HA && (unsigned)ix < (unsigned)WA;
      const unsigned off = ok ? (unsigned)((((img * HA + iy) * WA + ix) * 32 + oct * 8) * 4) : 0x80000000u;
#pragma unroll
      for (int l = 0; l < 2; ++l) sx[i][l] = __builtin_amdgcn_raw_buffer_load_b128(rs_x, (int)off, 16 * l, 0);
    }
#pragma unroll
    for (int i = 0; i < C::ND; ++i) {
      const int pc = tid + i * C::NT;
      const int pix = pc >> 1, oct = pc & 1;
      const int oy = y0 + pix / C::TW, ox = x0 + pix % C::TW;
      const bool ok = pc < C::DPC && oy < H && ox < W;
      const unsigned off = ok ? (unsigned)((((img * H + oy) * W + ox) * 16 + oct * 8) * 4) : 0x80000000u;
#pragma unroll
      for (int l = 0; l < 2; ++l) sd[i][l] = __builtin_amdgcn_raw_buffer_load_b128(rs_d, (int)off, 16 * l, 0);
    }
  };
  auto store_piece = [&](char* dst, int plane_bytes, const u32x4 (&v)[2], unsigned sgn) {
    u32x4 p0, p1, p2;
    split3(v[0] ^ sgn, v[1] ^ sgn, p0, p1, p2);
    *reinterpret_cast<u32x4*>(dst) = p0;
    *reinterpret_cast<u32x4*>(dst + plane_bytes) = p1;
    *reinterpret_cast<u32x4*>(dst + 2 * plane_bytes) = p2;
  };
  const int nseq = split < a.ntiles ? (a.ntiles - split + a.P - 1) / a.P : 0;
  const int sq1 = (nseq + 2) / 4, sq3 = nseq - sq1;               // + - - + over the block's tile sequence (see wgrad_h2_role)
  auto store_tile = [&](int bo, int seq) {
    const unsigned dsgn = (seq >= sq1 && seq < sq3) ? 0x80000000u : 0u;
#pragma unroll
    for (int i = 0; i < C::NX; ++i) {
      const int pc = tid + i * C::NT;
      if (i < C::NX - 1 || pc < C::XPC) store_piece(Xs + bo + pc * 16, C::XPLANE, sx[i], 0u);
    }
#pragma unroll
    for (int i = 0; i < C::ND; ++i) {
      const int pc = tid + i * C::NT;
      if (i < C::ND - 1 || pc < C::DPC) store_piece(Ds + bo + pc * 16, C::DPLANE, sd[i], dsgn);
    }
  };

  f32x16 acc[6];        // [u][e + 1]
#pragma unroll
  for (int t = 0; t < 6; ++t)
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[t][v] = 0.f;

  const int lane_off = (8 * hk + tq) * 64 + (cb + 4 * tp) * 2;
  const char* const dbase0 = Ds + ((2 * rsel + py) * C::TW + 32 * ksh) * 32 + lane_off;
  const char* const xbase0 = Xs + ((rsel + py) * C::AW + 16 * ksh) * 64 + lane_off;      // halo row (y >> 1) + py - 1 + u, pixel j - 1 + (e + 1)

  int cur = 0;
  if (split < a.ntiles) load_tile(split);
  store_tile(0, 0);
  if (split + a.P < a.ntiles) load_tile(split + a.P);
  __syncthreads();
  int seq = 0;
  bool negated = false;
  for (int tile = split; tile < a.ntiles; tile += a.P, ++seq) {
    if ((seq >= sq1 && seq < sq3) != negated) {
      negated = !negated;
#pragma unroll
      for (int t = 0; t < 6; ++t) acc[t] = -acc[t];
    }
    if (tile + a.P < a.ntiles) {
      store_tile(cur ^ C::BUF, seq + 1);
      if (tile + 2 * a.P < a.ntiles) load_tile(tile + 2 * a.P);
    }
    const char* const dbase = dbase0 + cur;
    const char* const xbase = xbase0 + cur;
    cur ^= C::BUF;
    bf16x8 A[PL];
#pragma unroll
    for (int pl = 0; pl < PL; ++pl) A[pl] = h2_tr_fragment(dbase + pl * C::DPLANE);
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int e = 0; e < 3; ++e) {
        bf16x8 B[PL];
#pragma unroll
        for (int pl = 0; pl < PL; ++pl) B[pl] = h2_tr_fragment(xbase + pl * C::XPLANE + (u * C::AW + e) * 64);
#pragma unroll
        for (int ij = 2; ij >= 0; --ij)
#pragma unroll
          for (int i = 0; i <= ij; ++i)
            acc[u * 3 + e] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[i], B[ij - i], acc[u * 3 + e], 0, 0, 0);
      }
    __syncthreads();
  }
  if (negated) {
#pragma unroll
    for (int t = 0; t < 6; ++t) acc[t] = -acc[t];
  }
  // accumulator -> taps: register v < 8 is the even-pixel row m = (v & 3) + 8 (v >> 2) + 4 lh, register v + 8 its odd-pixel twin, the
  // lane's column is the gathered channel.  Kernel rows of (py, u): py = 0: {0}, {1, 2};  py = 1: {0, 1}, {2}.
  // The columns are formed first, then the four K shares of a row parity meet in LDS (free after the last tile): one set of atomics
  // per block and parity.
  float out[48];        // [u][kx][v]
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int v = 0; v < 8; ++v) {
      out[(u * 3 + 0) * 8 + v] = acc[u * 3 + 0][v] + acc[u * 3 + 1][v + 8];
      out[(u * 3 + 1) * 8 + v] = acc[u * 3 + 1][v] + acc[u * 3 + 1][v + 8];
      out[(u * 3 + 2) * 8 + v] = acc[u * 3 + 1][v] + acc[u * 3 + 2][v + 8];
    }
  float* const red = reinterpret_cast<float*>(smem);                 // [3 shares][2 parities][48][64 lanes]
  if (ks != 0) {
#pragma unroll
    for (int j = 0; j < 48; ++j) red[(((ks - 1) * 2 + py) * 48 + j) * 64 + lane] = out[j];
  }
  __syncthreads();
  if (ks != 0) return;
#pragma unroll
  for (int k2 = 0; k2 < 3; ++k2)
#pragma unroll
    for (int j = 0; j < 48; ++j) out[j] += red[((k2 * 2 + py) * 48 + j) * 64 + lane];
  auto emit = [&](int u, int ky) {
#pragma unroll
    for (int v = 0; v < 8; ++v) {
      const int co_g = (v & 3) + 8 * (v >> 2) + 4 * lh;
      float* const row = a.dw + ((size_t)co_g * 9 + ky * 3) * a.ldw + a.dw_coff + lr;
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) atomicAdd(row + kx * a.ldw, out[(u * 3 + kx) * 8 + v]);
    }
  };
  if (py == 0) {
    emit(0, 0); emit(1, 1); emit(1, 2);
  } else {
    emit(0, 0); emit(0, 1); emit(1, 2);
  }
}

// its own template under the same name: the profiling symbol is conv_wgrad_h2_kernel<3, udaseg::H2P<TR, TWK>, XF> (H2PU: the up-sampled form)
template <int PL, typename C, bool XF>
__global__ __launch_bounds__(512, 1) void conv_wgrad_h2_kernel(const WgradH2Args a) {
  static_assert(PL == 3, "the pair-packed form is fp32 split only");
  extern __shared__ __attribute__((aligned(16))) char h2smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  if constexpr (C::UP) wgrad_h2pu_role<C>(a, h2smem, tid, lane, wave);
  else wgrad_h2p_role<C, XF>(a, h2smem, tid, lane, wave);
}

// the pair-packed form serves d (UDASEG_OPT_WGRAD_PAIR: bit 0 the 16 -> 16 layers, bit 1 the layers of two produced-channel blocks,
// bit 2 the up-sampled 32 -> 16 layer without a skip half -- the one geometry with up_ca == ci)
static bool h2_pair_up_config(const udaseg_conv_desc* d, int up_ca, bool f32) {
  if (!f32 || up_ca != 32 || d->ci != 32 || d->co != 16) return false;
  if (d->hi % 2 != 0 || d->wi % 2 != 0 || d->wi < 16) return false;
  return (opt_get(UDASEG_OPT_WGRAD_PAIR) & 4) != 0;
}
static bool h2_pair_config(const udaseg_conv_desc* d, int up_ca, bool f32) {
  if (!f32 || up_ca != 0 || d->ci != 16 || d->co < 8 || d->co > 32 || d->co % 8 != 0) return false;
  if (d->wi % 2 != 0 || d->wi < 16) return false;
  return (opt_get(UDASEG_OPT_WGRAD_PAIR) & (d->co <= 16 ? 1 : 2)) != 0;
}

// which configuration serves (d, up_ca): 0 = none
//   1: 64 x 64 channel blocks, 4 x 32 pixel tiles (f32x3) / 8 x 32 (bf16)      2: 64 x 64, 8 x 16 pixel tiles (16-pixel-wide images)
//   3: 32 produced x 64 gathered channels, 4 x 32 (f32x3) / 8 x 32 (bf16)      4: 32 x 32 channels
//   5: 16 gathered channels, pair-packed, 4 x 64 pixel tiles (fp32 only)      6: 32 up-sampled -> 16, no skip half, pair-packed dy
static int h2_config(const udaseg_conv_desc* d, int up_ca, bool f32) {
  if (d->kh != 3 || d->kw != 3 || d->stride != 1 || d->pad != 1) return 0;
  if (d->n <= 0 || d->hi <= 0 || d->wi <= 0 || d->ho != d->hi || d->wo != d->wi || d->ci <= 0 || d->co <= 0) return 0;
  const long long px = (long long)d->n * d->hi * d->wi;
  const int es = f32 ? 4 : 2;
  if (px * d->ci * es >= (1LL << 31) || px * d->co * es >= (1LL << 31)) return 0;
  if (h2_pair_config(d, up_ca, f32)) return 5;
  if (h2_pair_up_config(d, up_ca, f32)) return 6;
  int cfg = 0;
  if (d->ci % 64 == 0 && d->co % 64 == 0) cfg = d->wi < 32 ? 2 : 1;
  else if (d->ci % 64 == 0 && d->co % 32 == 0) cfg = 3;
  else if (d->ci % 32 == 0 && d->co % 32 == 0) cfg = 4;
  if (cfg == 0 || d->wi < 16) return 0;
  if (cfg != 2 && d->wi < 32) return 0;
  if (up_ca > 0) {
    if (up_ca >= d->ci || d->hi % 2 != 0 || d->wi % 2 != 0) return 0;
    if (up_ca % 64 != 0) {            // the source boundary must fall between two gathered-channel blocks: 32-channel blocks
      if (up_ca % 32 != 0 || d->wi < 32) return 0;
      cfg = 4;
    }
  }
  return cfg;
}

bool wgrad_h2_applicable(const udaseg_conv_desc* d, int up_ca, bool f32) { return d != nullptr && h2_config(d, up_ca, f32) != 0; }

struct H2In {        // WgradH2Args::in_*
  const float* scale = nullptr;
  const float* shift = nullptr;
  int act = 0;
  float slope = 0.f;
  int ldw = 0, dw_coff = 0;      // > 0: dW rows are ldw channels long and this launch fills [dw_coff, dw_coff + ci) (a slice of a wider layer)
};

template <int PL, int COQ, int CIQ, int TR, int TWK, int NSTW, bool DB = false>
static int launch_h2_t(const udaseg_conv_desc* d, const void* x, const void* x2, int up_ca, const void* dy, float* dw, hipStream_t s,
                       int target, const H2In& in = H2In()) {
  using C = H2<PL, COQ, CIQ, TR, TWK, NSTW, DB>;
  WgradH2Args a = {};
  a.x = x; a.x2 = x2; a.dy = dy; a.dw = dw;
  a.ldw = in.ldw > 0 ? in.ldw : d->ci; a.dw_coff = in.ldw > 0 ? in.dw_coff : 0;
  a.in_scale = in.scale; a.in_shift = in.shift; a.in_act = in.act; a.in_slope = in.slope;
  a.n = d->n; a.h = d->hi; a.w = d->wi; a.ci = d->ci; a.co = d->co; a.up_ca = up_ca;
  a.ntx = cdiv(d->wi, C::TW); a.nty = cdiv(d->hi, C::TR); a.ntiles = d->n * a.ntx * a.nty;
  a.ncib = d->ci / C::CIB; a.pairs = a.ncib * (d->co / C::COB);
  int P = target / a.pairs;
  if (P < 1) P = 1;
  if (P > a.ntiles) P = a.ntiles;
  a.P = P;
  const long long px = (long long)d->n * d->hi * d->wi;
  a.x_bytes = (unsigned)(up_ca > 0 ? (long long)d->n * (d->hi / 2) * (d->wi / 2) * up_ca * C::ES : px * d->ci * C::ES);
  a.x2_bytes = (unsigned)(up_ca > 0 ? px * (d->ci - up_ca) * C::ES : 0);
  a.dy_bytes = (unsigned)(px * d->co * C::ES);
  // the kernel of this launch, its record and its text; the stamped twin is booked under the plain symbol
  static KernelRec plain("hipFuncSetAttribute(conv_wgrad_h2)", "conv_wgrad_h2_kernel<%d, %d, %d, %d, %d, %d, %s, false, false>", PL, COQ, CIQ,
                         TR, TWK, NSTW, DB ? "true" : "false");
  KernelRec* rec = &plain;
  auto kern = conv_wgrad_h2_kernel<PL, COQ, CIQ, TR, TWK, NSTW, DB>;
  const char* what = "conv_wgrad_h2 launch";
  if constexpr (PL == 3 && COQ == 2 && CIQ == 2 && TWK == 2) {      // the dominant configuration has a stamped twin (diagnosis only)
    // (never for a launch that transforms x while staging: the twin has no XF form and would multiply the RAW tensor)
    if (g_timeline != nullptr && a.in_scale == nullptr && (long long)a.pairs * P * 16 <= (long long)g_timeline_blocks * 6) {
      static KernelRec tl("hipFuncSetAttribute(conv_wgrad_h2 timeline twin)", "conv_wgrad_h2_kernel<%d, %d, %d, %d, %d, %d, %s, false, false>",
                          PL, COQ, CIQ, TR, TWK, NSTW, DB ? "true" : "false");
      rec = &tl;
      kern = conv_wgrad_h2_kernel<PL, COQ, CIQ, TR, TWK, NSTW, DB, true>;
      what = "conv_wgrad_h2 (timeline) launch";
      a.timeline = g_timeline;
    }
  }
  if constexpr (PL == 3) {
    if (a.in_scale != nullptr) {          // the instantiation that transforms x while it stages (WgradH2Args::in_scale)
      static KernelRec xf("hipFuncSetAttribute(conv_wgrad_h2, in-staging transform)",
                          "conv_wgrad_h2_kernel<%d, %d, %d, %d, %d, %d, %s, false, true>", PL, COQ, CIQ, TR, TWK, NSTW, DB ? "true" : "false");
      rec = &xf;
      kern = conv_wgrad_h2_kernel<PL, COQ, CIQ, TR, TWK, NSTW, DB, false, true>;
      what = "conv_wgrad_h2 (in-staging transform) launch";
    }
  }
  return launch_kernel(*rec, kern, dim3((unsigned)(a.pairs * P)), dim3(C::NT), C::LDS, C::LDS, s, 2.0 * (double)px * d->co * 9.0 * d->ci, what, a);
}

template <typename C>
static int launch_h2p_t(const udaseg_conv_desc* d, const void* x, const void* dy, float* dw, hipStream_t s, int target, const H2In& in) {
  WgradH2Args a = {};
  a.x = x; a.dy = dy; a.dw = dw;
  a.ldw = in.ldw > 0 ? in.ldw : d->ci; a.dw_coff = in.ldw > 0 ? in.dw_coff : 0;
  a.in_scale = in.scale; a.in_shift = in.shift; a.in_act = in.act; a.in_slope = in.slope;
  a.n = d->n; a.h = d->hi; a.w = d->wi; a.ci = d->ci; a.co = d->co;
  a.ntx = cdiv(d->wi, C::TW); a.nty = cdiv(d->hi, C::TR); a.ntiles = d->n * a.ntx * a.nty;
  a.ncib = 1; a.pairs = cdiv(d->co, 16);
  int P = target / a.pairs;
  if (P < 1) P = 1;
  if (P > a.ntiles) P = a.ntiles;
  a.P = P;
  const long long px = (long long)d->n * d->hi * d->wi;
  a.x_bytes = (unsigned)((C::UP ? px / 4 : px) * d->ci * 4);
  a.dy_bytes = (unsigned)(px * d->co * 4);
  if (C::UP && a.in_scale != nullptr) {          // the up-sampled form has no in-staging transform
    set_error("conv2d_wgrad_halo: the pair-packed up-sampled form takes a written source only");
    return UDASEG_E_UNSUPPORTED;
  }
  const bool xf = a.in_scale != nullptr;
  auto kern = conv_wgrad_h2_kernel<3, C, false>;
  if constexpr (!C::UP) {
    if (xf) kern = conv_wgrad_h2_kernel<3, C, true>;
  }
  static KernelRec rec[2] = {{"hipFuncSetAttribute(conv_wgrad_h2, pair-packed)", "conv_wgrad_h2_kernel<3, udaseg::H2P%s<%d, %d>, false>",
                              C::UP ? "U" : "", C::TR, C::TWK},
                             {"hipFuncSetAttribute(conv_wgrad_h2, pair-packed)", "conv_wgrad_h2_kernel<3, udaseg::H2P%s<%d, %d>, true>",
                              C::UP ? "U" : "", C::TR, C::TWK}};
  return launch_kernel(rec[xf], kern, dim3((unsigned)(a.pairs * P)), dim3(C::NT), C::LDS, C::LDS, s, 2.0 * (double)px * d->co * 9.0 * d->ci,
                       "conv_wgrad_h2 (pair-packed) launch", a);
}

int launch_wgrad_h2(const udaseg_conv_desc* d, const void* x, const void* x2, int up_ca, const void* dy, float* dw, bool f32,
                    hipStream_t s, const float* in_scale, const float* in_shift, int in_act, float in_slope, int ldw, int dw_coff) {
  H2In in;
  in.scale = in_scale; in.shift = in_shift; in.act = in_act; in.slope = in_slope;
  in.ldw = ldw; in.dw_coff = dw_coff;
  if (in_scale != nullptr && (!f32 || up_ca != 0 || in_shift == nullptr)) {
    set_error("conv2d_wgrad_halo: the in-staging transform needs fp32 operands and a single plain source");
    return UDASEG_E_UNSUPPORTED;
  }
  const int cfg = h2_config(d, up_ca, f32);
  if (cfg == 0) {
    set_error("conv2d_wgrad_halo: geometry not supported (ask the _ok query first)");
    return UDASEG_E_UNSUPPORTED;
  }
  // blocks per launch: few and long-lived (one set of atomics per wave; the kernel runs beside the main stream's chain).
  // UDASEG_WGRAD_F3_BLOCKS / UDASEG_WGRAD_HALO_BLOCKS: tuning aids
  int tf3 = opt_get(UDASEG_OPT_WGRAD_F3_BLOCKS), tbf = opt_get(UDASEG_OPT_WGRAD_HALO_BLOCKS);
  const int tdeep_o = opt_get(UDASEG_OPT_WGRAD_DEEP_BLOCKS);
  const int tdeep = tdeep_o >= 1 ? tdeep_o : 256;        // 16-pixel-wide images, bf16
  const int tdeep3 = tdeep_o >= 1 ? tdeep_o : 128;       // ... fp32 split: 64 / 96 / 128 / 160 / 256 / 384 blocks -> 979.3 / 980.6 / 987.3 /
                                                         // 985.5 / 983.5 images/s on one box, 942.1 (128) / 942.3 (192) / 937.1 / 936.9 on another
  if (tf3 < 1) tf3 = 120;
  if (tbf < 1) tbf = 96;
  const int db = opt_get(UDASEG_OPT_WGRAD_DB);      // 0: the single-buffer 4-row form of the 64 x 64 fp32 configuration (A/B)
  if (f32) {
    if (cfg == 5) {          // UDASEG_OPT_WGRAD_PAIR_BLOCKS: tuning aid
      const int tp = opt_get(UDASEG_OPT_WGRAD_PAIR_BLOCKS);
      return launch_h2p_t<H2P<4, 2>>(d, x, dy, dw, s, tp >= 1 ? tp : 120, in);
    }
    if (cfg == 6) {
      const int tp = opt_get(UDASEG_OPT_WGRAD_PAIR_BLOCKS);
      return launch_h2p_t<H2PU<4, 2>>(d, x, dy, dw, s, tp >= 1 ? tp : 120, in);
    }
    if (cfg == 1 && db) return launch_h2_t<3, 2, 2, 2, 2, 4, true>(d, x, x2, up_ca, dy, dw, s, tf3, in);
    if (cfg == 1) return launch_h2_t<3, 2, 2, 4, 2, 4>(d, x, x2, up_ca, dy, dw, s, tf3, in);
    if (cfg == 2) return launch_h2_t<3, 2, 2, 8, 1, 4>(d, x, x2, up_ca, dy, dw, s, tdeep3, in);
    if (cfg == 3) return launch_h2_t<3, 1, 2, 4, 2, 4>(d, x, x2, up_ca, dy, dw, s, tf3, in);
    return launch_h2_t<3, 1, 1, 4, 2, 4>(d, x, x2, up_ca, dy, dw, s, tf3, in);
  }
  if (cfg == 1) return launch_h2_t<1, 2, 2, 8, 2, 8>(d, x, x2, up_ca, dy, dw, s, tbf);
  if (cfg == 2) return launch_h2_t<1, 2, 2, 8, 1, 8>(d, x, x2, up_ca, dy, dw, s, tdeep);
  if (cfg == 3) return launch_h2_t<1, 1, 2, 8, 2, 8>(d, x, x2, up_ca, dy, dw, s, tbf);
  return launch_h2_t<1, 1, 1, 8, 2, 8>(d, x, x2, up_ca, dy, dw, s, tbf);
}

// ------------------------------------------------------------------------------------------------------------------------------------
// Round 5: the weight gradient of a decoder conv1's UP-SAMPLED half in the phase form of conv_up_f32x3.hip.
//   conv3x3(nearest_x2(a)) = four 2x2 phase convolutions of a with pre-summed weights W'_{py,px}[u][v], so
//   T_{py,px}[u][v][co][ci] = sum_{q,r} dy[2q+py, 2r+px][co] * a[q + py - 1 + u, r + px - 1 + v][ci]          (16 correlations at a's size)
//   dW[ky][kx] += T_{py,px}[u][v]  for every (py, u) with ky in Ky(py, u) and (px, v) with kx in Kx(px, v)      (each tap: 4 of the 16)
// -- 16 tap evaluations per pixel of `a` instead of 4 x 9 = 36 (reference: loss.backward(), src/models/train.py:343, through
// aten::upsample_nearest2d + aten::_convolution of smp's DecoderBlock).  The h2 scheme in a's coordinates: a block owns a
// (32 COQ) x (32 CIQ) block of dW and ONE column phase px, and walks tiles of TR rows x 16 TWK pixels of `a`; it stages the a-halo
// once per tile and the 2 TR rows x TW pixels of dy that are the phases (0, px), (1, px) of the tile (pixels two apart in memory:
// the same 16-byte pieces as any other gather); waves 0-3 own the halo column offset ex = px (v = 0), waves 4-7 ex = px + 1 (v = 1),
// each its (py, u) in {0,1}^2 accumulators of a 32 x 32 quadrant: an x fragment of halo row rr feeds the dy rows 2 (rr - py - u) + py.
// All eight waves stage (the MFMA work per staged byte is 4/9 of the nine-tap kernel's); two LDS buffers, one barrier per tile.
// The accumulators leave as fp32 atomics into the one, two or four taps their phase tap stands for.
struct WgradUpArgs {
  const float* x;     // a [n][h][w][ca]
  const float* dy;    // [n][2h][2w][co]
  float* dw;          // [co][9][ldw] fp32, accumulated onto (channels [0, ca) of the rows)
  int n, h, w, ca, co, ldw;
  int ntx, nty, ntiles, ncib, pairs, P;
  unsigned x_bytes, dy_bytes;
};

template <int COQ_, int CIQ_, int TR_, int TWK_>
struct H2Up {
  static constexpr int PL = 3, COQ = COQ_, CIQ = CIQ_, TR = TR_, TWK = TWK_;
  static constexpr int NT = 512;
  static constexpr int COB = 32 * COQ, CIB = 32 * CIQ, TW = 16 * TWK;
  static constexpr int HR = TR + 2, HWD = TW + 2, HP = HR * HWD, TP = 2 * TR * TW;       // dy: rows 2 q + py of the tile
  static constexpr int NQ = COQ * CIQ, KS = 4 / NQ;
  static constexpr int KSH = KS < TWK ? KS : TWK, KSR = KS / KSH;
  static constexpr int RW = TR / KSR, NHF = TWK / KSH;
  static constexpr int XSP = h2_pad(HP * 64), DSP = h2_pad(TP * 64);
  static constexpr int XPLANE = CIQ * XSP, DPLANE = COQ * DSP;
  static constexpr int BUF = PL * (XPLANE + DPLANE);
  static constexpr int LDS = 2 * BUF;
  static constexpr int XO = CIB / 8, DO = COB / 8;
  static constexpr int XPC = HP * XO, DPC = TP * DO;
  static constexpr int NX = (XPC + NT - 1) / NT, ND = (DPC + NT - 1) / NT;
  static_assert(NQ == 2 || NQ == 4, "2 or 4 quadrants");
  static_assert(TR % KSR == 0 && TWK % KSH == 0 && KSH * KSR == KS, "K split tiles the tile");
  static_assert(LDS <= 160 * 1024, "LDS");
};

template <typename C, int V>
__device__ __forceinline__ void wgrad_up_role(const WgradUpArgs& a, char* smem, int tid, int lane, int wave) {
  constexpr int PL = 3;
  char* const Xs = smem;
  char* const Ds = smem + PL * C::XPLANE;
  const int lr = lane & 31, lh = lane >> 5;
  const int grp = lane >> 4, cb = 16 * (grp & 1), hk = grp >> 1, tq = (lane & 15) >> 2, tp = lane & 3;
  const int q = wave & 3;
  const int qi = q % C::NQ, ks = q / C::NQ;
  const int coq = qi / C::CIQ, ciq = qi % C::CIQ;
  const int ksh = ks % C::KSH, r0 = (ks / C::KSH) * C::RW;
  int bidx = (int)blockIdx.x;
  const int px = bidx & 1;                 // this block's column phase
  bidx >>= 1;
  const int pair = bidx % a.pairs, split = bidx / a.pairs;
  const int cob = pair / a.ncib, cib = pair % a.ncib;
  const int H = a.h, W = a.w;
  __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.x), 0, (int)a.x_bytes, 0x00020000);
  __amdgpu_buffer_rsrc_t rs_d = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.dy), 0, (int)a.dy_bytes, 0x00020000);
  u32x4 sx[C::NX][2], sd[C::ND][2];
  auto load_tile = [&](int tile) {
    const int tx = tile % a.ntx;
    const int t2 = tile / a.ntx;
    const int ty = t2 % a.nty, img = t2 / a.nty;
    const int y0 = ty * C::TR, x0 = tx * C::TW;
#pragma unroll
    for (int i = 0; i < C::NX; ++i) {
      const int pc = tid + i * C::NT;
      const int pix = pc / C::XO, oct = pc % C::XO;
      const int hy = pix / C::HWD, hx = pix - hy * C::HWD;
      const int iy = y0 + hy - 1, ix = x0 + hx - 1;
      const bool ok = pc < C::XPC && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
      const unsigned off = ok ? (unsigned)((((img * H + iy) * W + ix) * a.ca + cib * C::CIB + oct * 8) * 4) : 0x80000000u;
#pragma unroll
      for (int l = 0; l < 2; ++l) sx[i][l] = __builtin_amdgcn_raw_buffer_load_b128(rs_x, (int)off, 16 * l, 0);
    }
#pragma unroll
    for (int i = 0; i < C::ND; ++i) {
      const int pc = tid + i * C::NT;
      const int pix = pc / C::DO, oct = pc % C::DO;
      const int row2 = pix / C::TW, col = pix % C::TW;          // row2 = 2 (row of the tile) + py
      const int qy = y0 + (row2 >> 1), qx = x0 + col;
      const bool ok = pc < C::DPC && qy < H && qx < W;
      const unsigned off = ok ? (unsigned)((((img * 2 * H + 2 * qy + (row2 & 1)) * (2 * W) + 2 * qx + px) * a.co + cob * C::COB + oct * 8) * 4)
                              : 0x80000000u;
#pragma unroll
      for (int l = 0; l < 2; ++l) sd[i][l] = __builtin_amdgcn_raw_buffer_load_b128(rs_d, (int)off, 16 * l, 0);
    }
  };
  auto store_piece = [&](char* dst, int plane_bytes, const u32x4 (&v)[2], unsigned sgn) {
    u32x4 p0, p1, p2;
    split3(v[0] ^ sgn, v[1] ^ sgn, p0, p1, p2);
    *reinterpret_cast<u32x4*>(dst) = p0;
    *reinterpret_cast<u32x4*>(dst + plane_bytes) = p1;
    *reinterpret_cast<u32x4*>(dst + 2 * plane_bytes) = p2;
  };
  const int nseq = split < a.ntiles ? (a.ntiles - split + a.P - 1) / a.P : 0;
  const int sq1 = (nseq + 2) / 4, sq3 = nseq - sq1;             // + - - + over the block's tile sequence (see wgrad_h2_role)
  auto store_tile = [&](int bo, int seq) {
    const unsigned dsgn = (seq >= sq1 && seq < sq3) ? 0x80000000u : 0u;
#pragma unroll
    for (int i = 0; i < C::NX; ++i) {
      const int pc = tid + i * C::NT;
      const int pix = pc / C::XO, oct = pc % C::XO;
      if (i < C::NX - 1 || pc < C::XPC) store_piece(Xs + bo + (oct >> 2) * C::XSP + pix * 64 + (oct & 3) * 16, C::XPLANE, sx[i], 0u);
    }
#pragma unroll
    for (int i = 0; i < C::ND; ++i) {
      const int pc = tid + i * C::NT;
      const int pix = pc / C::DO, oct = pc % C::DO;
      if (i < C::ND - 1 || pc < C::DPC) store_piece(Ds + bo + (oct >> 2) * C::DSP + pix * 64 + (oct & 3) * 16, C::DPLANE, sd[i], dsgn);
    }
  };

  f32x16 acc[4];        // [py * 2 + u]
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[t][v] = 0.f;

  const int lane_off = (8 * hk + tq) * 64 + (cb + 4 * tp) * 2;
  const char* const dbase0 = Ds + coq * C::DSP + (2 * r0 * C::TW + 16 * ksh) * 64 + lane_off;
  const char* const xbase0 = Xs + ciq * C::XSP + (r0 * C::HWD + 16 * ksh + px + V) * 64 + lane_off;

  int cur = 0;
  if (split < a.ntiles) load_tile(split);
  store_tile(0, 0);
  if (split + a.P < a.ntiles) load_tile(split + a.P);
  __syncthreads();
  int seq = 0;
  bool negated = false;
  for (int tile = split; tile < a.ntiles; tile += a.P, ++seq) {
    if ((seq >= sq1 && seq < sq3) != negated) {
      negated = !negated;
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] = -acc[t];
    }
    if (tile + a.P < a.ntiles) {
      store_tile(cur ^ C::BUF, seq + 1);
      if (tile + 2 * a.P < a.ntiles) load_tile(tile + 2 * a.P);
    }
    const char* const dbase = dbase0 + cur;
    const char* const xbase = xbase0 + cur;
    cur ^= C::BUF;
#pragma unroll
    for (int hfi = 0; hfi < C::NHF; ++hfi) {
      // dy fragments: D0[j] = phase row py = 0 of tile row j (LDS row 2 j), D1[j] = py = 1 (LDS row 2 j + 1); at halo row rr the
      // taps (py, u) read D_py[rr - py - u]: D0[rr] and D1[rr - 1] are new, D0[rr - 1] and D1[rr - 2] come from the step before
      bf16x8 D0[2][PL], D1[2][PL];
#pragma unroll
      for (int rr = 0; rr < C::RW + 2; ++rr) {
        if (rr < C::RW) {
#pragma unroll
          for (int pl = 0; pl < PL; ++pl)
            D0[rr & 1][pl] = h2_tr_fragment(dbase + pl * C::DPLANE + ((2 * rr) * C::TW + 16 * C::KSH * hfi) * 64);
        }
        if (rr >= 1 && rr - 1 < C::RW) {
#pragma unroll
          for (int pl = 0; pl < PL; ++pl)
            D1[(rr - 1) & 1][pl] = h2_tr_fragment(dbase + pl * C::DPLANE + ((2 * (rr - 1) + 1) * C::TW + 16 * C::KSH * hfi) * 64);
        }
        bf16x8 B[PL];
#pragma unroll
        for (int pl = 0; pl < PL; ++pl) B[pl] = h2_tr_fragment(xbase + pl * C::XPLANE + (rr * C::HWD + 16 * C::KSH * hfi) * 64);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int py = t >> 1, u = t & 1;
          const int j = rr - py - u;           // tile row whose tap (py, u) reads halo row rr
          if (j >= 0 && j < C::RW) {
#pragma unroll
            for (int ij = 2; ij >= 0; --ij)
#pragma unroll
              for (int i = 0; i <= ij; ++i)
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(py ? D1[j & 1][i] : D0[j & 1][i], B[ij - i], acc[t], 0, 0, 0);
          }
        }
      }
    }
    __syncthreads();
  }
  if (negated) {
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = -acc[t];
  }
  // dW[co][ky][kx][ci] += T: the kernel rows Ky(py, u) x columns Kx(px, V) this phase tap stands for
  const int ci_g = cib * C::CIB + ciq * 32 + lr;
  const int kx0 = px == 0 ? (V ? 1 : 0) : (V ? 2 : 0), kx1 = px == 0 ? (V ? 2 : 0) : (V ? 2 : 1);
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int py = t >> 1, u = t & 1;
    const int ky0 = py == 0 ? (u ? 1 : 0) : (u ? 2 : 0), ky1 = py == 0 ? (u ? 2 : 0) : (u ? 2 : 1);
#pragma unroll
    for (int ky = ky0; ky <= ky1; ++ky)
      for (int kx = kx0; kx <= kx1; ++kx)
#pragma unroll
        for (int v = 0; v < 16; ++v) {
          const int co_g = cob * C::COB + coq * 32 + (v & 3) + 8 * (v >> 2) + 4 * lh;
          atomicAdd(a.dw + ((size_t)co_g * 9 + ky * 3 + kx) * a.ldw + ci_g, acc[t][v]);
        }
  }
}

template <int COQ, int CIQ, int TR, int TWK>
__global__ __launch_bounds__(512, 2) void conv_wgrad_up_kernel(const WgradUpArgs a) {
  using C = H2Up<COQ, CIQ, TR, TWK>;
  extern __shared__ __attribute__((aligned(16))) char h2smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  if (wave < 4) wgrad_up_role<C, 0>(a, h2smem, tid, lane, wave);
  else wgrad_up_role<C, 1>(a, h2smem, tid, lane, wave);
}

// 0: not served; 1 / 2: 64 x 64 channel blocks, 2 x 16 a-pixel tiles (a 1 x 32 tile form for wide images was measured and dropped: its
// three-row halo for one row of pixels triples the staged x bytes); 3: 32 produced x 64 gathered channels, 1 x 32 tiles
static int h2up_config(const udaseg_conv_desc* d, int up_ca) {
  if (!d || d->kh != 3 || d->kw != 3 || d->stride != 1 || d->pad != 1) return 0;
  if (d->n <= 0 || d->hi < 2 || d->wi < 2 || d->ho != d->hi || d->wo != d->wi || d->hi % 2 || d->wi % 2) return 0;
  if (up_ca <= 0 || up_ca > d->ci || up_ca % 64 != 0 || d->co % 32 != 0) return 0;
  const long long px = (long long)d->n * d->hi * d->wi;
  if (px * d->co * 4 >= (1LL << 31) || px / 4 * up_ca * 4 >= (1LL << 31)) return 0;
  const int wa = d->wi / 2;
  if (wa < 16) return 0;
  if (d->co % 64 != 0) return wa >= 32 ? 3 : 0;
  return wa >= 32 ? 1 : 2;
}

template <int COQ, int CIQ, int TR, int TWK>
static int launch_h2up_t(const udaseg_conv_desc* d, const float* a_, int up_ca, const float* dy, float* dw, hipStream_t s, int target) {
  using C = H2Up<COQ, CIQ, TR, TWK>;
  WgradUpArgs a = {};
  a.x = a_; a.dy = dy; a.dw = dw;
  a.n = d->n; a.h = d->hi / 2; a.w = d->wi / 2; a.ca = up_ca; a.co = d->co; a.ldw = d->ci;
  a.ntx = cdiv(a.w, C::TW); a.nty = cdiv(a.h, C::TR); a.ntiles = a.n * a.ntx * a.nty;
  a.ncib = up_ca / C::CIB; a.pairs = a.ncib * (d->co / C::COB);
  int P = target / (2 * a.pairs);
  if (P < 1) P = 1;
  if (P > a.ntiles) P = a.ntiles;
  a.P = P;
  const long long pa = (long long)a.n * a.h * a.w;
  a.x_bytes = (unsigned)(pa * up_ca * 4);
  a.dy_bytes = (unsigned)(4 * pa * d->co * 4);
  static KernelRec rec("hipFuncSetAttribute(conv_wgrad_up)", "conv_wgrad_up_kernel<%d, %d, %d, %d>", COQ, CIQ, TR, TWK);
  return launch_kernel(rec, conv_wgrad_up_kernel<COQ, CIQ, TR, TWK>, dim3((unsigned)(2 * a.pairs * P)), dim3(C::NT), C::LDS, C::LDS, s,
                       2.0 * (double)pa * d->co * 16.0 * up_ca, "conv_wgrad_up launch", a);
}

}  // namespace udaseg

using namespace udaseg;

extern "C" int udaseg_conv2d_wgrad_up_f32x3_ok(const udaseg_conv_desc* d, int up_ca) {
  return f32_halo_enabled() && h2up_config(d, up_ca) != 0 ? 1 : 0;
}

extern "C" int udaseg_wgrad_up_set_blocks(int blocks) {
  UDASEG_CHECK_ARG(blocks >= 0 && blocks <= 4096, "wgrad_up_set_blocks: 0 (default) .. 4096");
  return udaseg_set_option(UDASEG_OPT_WGRAD_UP_BLOCKS, blocks);
}

// dW[co][9][ci] (rows of d->ci channels, the first up_ca of them) += the weight gradient of conv3x3(nearest_x2(a)) in the phase form
extern "C" int udaseg_conv2d_wgrad_up_f32x3(const udaseg_conv_desc* d, const float* a, int up_ca, const float* dy, float* dw,
                                            void* stream) {
  UDASEG_CHECK_ARG(d && a && dy && dw, "conv2d_wgrad_up_f32x3: NULL pointer");
  const int cfg = f32_halo_enabled() ? h2up_config(d, up_ca) : 0;
  if (cfg == 0) {
    set_error("conv2d_wgrad_up_f32x3: geometry not supported (ask udaseg_conv2d_wgrad_up_f32x3_ok first)");
    return UDASEG_E_UNSUPPORTED;
  }
  // blocks per launch: few and long-lived like the nine-tap kernel.  Same-box sweep inside the overlapped step (images/s, phase weight
  // gradient off 983.7 / 996.7): 2 x 16 tiles at 64 / 128 / 256 blocks 995.2 / 990.1-994.4 / 969.7, 1 x 32 tiles at 128 / 256 blocks
  // 984.8 / 966.1 (profiles/r05_up_phase.txt) -- the 16-pixel tile everywhere, 96 blocks
  const int target = opt_get(UDASEG_OPT_WGRAD_UP_BLOCKS) > 0 ? opt_get(UDASEG_OPT_WGRAD_UP_BLOCKS) : 96;
  hipStream_t st = as_stream(stream);
  udaseg_conv_desc dd = *d;
  dd.ci = up_ca;
  const double flops = 2.0 * (double)d->n * (d->hi / 2) * (d->wi / 2) * d->co * 16.0 * up_ca;
  prof_begin(1, st);
  int rc;
  if (cfg == 1 || cfg == 2) rc = launch_h2up_t<2, 2, 2, 1>(d, a, up_ca, dy, dw, st, target);
  else rc = launch_h2up_t<1, 2, 1, 2>(d, a, up_ca, dy, dw, st, target);
  prof_end(1, st, flops, 2, &dd);
  return rc;
}
