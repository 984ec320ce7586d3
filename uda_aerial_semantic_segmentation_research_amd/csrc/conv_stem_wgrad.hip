// The stem's weight gradient with its BatchNorm backward in the staging: 7x7 / stride 2 / pad 3, 4 physical (3 live) input channels,
// 64 output channels, fp32 storage, v_mfma_f32_32x32x2_f32 (gfx950) -- autograd's weight gradient of torchvision ResNet.conv1 and
// the apply half of bn1's backward inside smp.Unet (reference src/models/train.py:343; trace fixture: the last
// aten::convolution_backward / aten::native_batch_norm_backward pair of a step).
//
// The stem has no data gradient, so dy = bn_bwd_apply(dz, y) had ONE reader, the weight gradient: a pass that read dz and y and wrote
// dy (3 x 134 MB at 8 x 512^2) to hand one operand to one kernel.  Here the loader forms dy from dz and y with bn_bwd_apply_kernel's
// fp32 arithmetic (norm_act.hip: same coefficients from the same sums and casts, same operation order) while it stages them, and dy
// never exists in memory.
//
// GEMM view:  dW[co][j] = sum_m dy[m][co] * X[m][j],  m over the output pixels, j over the 147 LIVE (ky, kx, c) triples padded to the
// MFMA granule: 5 column blocks of 32 = 160 columns (the generic split-K kernel multiplied 4 x 64 = 256, the padded channel among
// them, and re-read dy once per column block).  A block owns ALL columns of its pixel slab, so dz, y and x are read once per launch.
//   * slab: 8 x 32 output pixels.  dy of the slab sits in LDS as [pixel][64] (64 KB); the 21 x 69 input pixels under it are staged
//     once with the dead channel dropped, 3 floats per pixel: for kernel row ky the 21 columns (kx, c) of output pixel ox are then 21
//     CONTIGUOUS floats of input row 2 oy + ky - 3 starting at 6 ox (conv_stem_f32x3.hip's view of the forward), and a lane's B
//     operand is one ds_read_b32 at a per-lane column offset plus a compile-time step offset.
//   * 8 waves: wave w multiplies output-channel block w & 1 with all 5 column blocks (80 accumulator registers) over rows 2 (w >> 1)
//     and 2 (w >> 1) + 1 of the slab: 32 K-steps of 5 MFMAs per slab.
//   * persistent over the slabs with the next slab's dz / y / x in flight (registers) during the current slab's MFMAs; accumulators
//     stay in registers for the life of the block, the 4 row groups are folded through LDS at the end (fixed order) and ONE set of
//     64 x 147 fp32 atomics per block goes to the gradient arena.  The arena's fourth-channel entries receive nothing.
//   * every block derives the 64 channels' coefficients in a short preamble, block 0 writes dgamma / dbeta, as bn_bwd_apply_kernel does.
#include "common.h"
#include "launch.h"

namespace udaseg {

struct StemWgradArgs {
  const float* x;        // [n][hi][wi][4]
  const float* dz;       // [n][ho][wo][64] gradient of the activation
  const float* y;        // [n][ho][wo][64] the stem's raw convolution output
  const float *mean, *rstd, *gamma, *beta;
  const double* bsums;   // [R][2][64] sum(g), sum(g * xhat) (bn_bwd_reduce)
  float* dw;             // [64][7][7][4]
  float *dgamma, *dbeta;
  int n, hi, wi, ho, wo;
  int ntx, nty, nslabs;
  long long pixels;
  int act;
  float slope;
  int acc_param;
};

struct StemWgradCfg {
  static constexpr int NT = 512;
  static constexpr int TH = 8, TW = 32;                   // output pixels of a slab
  static constexpr int IR = 2 * TH + 5, IP = 2 * TW + 5;  // input rows / pixels of the band under it
  static constexpr int XS = 208;                          // floats of a band row (3 * IP = 207 used)
  static constexpr int NPIECE = IR * IP;
  static constexpr int NI = (NPIECE + NT - 1) / NT;
  static constexpr int NQ = TH * TW * 16 / NT;            // 16-byte vectors of dz (and of y) a thread stages per slab
  static constexpr int COLS = 147, NB = 5, LDC = 32 * NB; // live columns, column blocks, padded columns
  static constexpr int DY_FLOATS = TH * TW * 64, X_FLOATS = IR * XS, COEF_FLOATS = 6 * 64;
  static constexpr int LDS = (DY_FLOATS + X_FLOATS + COEF_FLOATS) * 4;
};

__global__ __launch_bounds__(512) void conv_small_ci_wgrad_kernel(const StemWgradArgs a) {
  using C = StemWgradCfg;
  static_assert(64 * C::LDC <= C::DY_FLOATS, "the end-of-block fold reuses the dy region");
  extern __shared__ __attribute__((aligned(16))) float swsm[];
  float* const dyl = swsm;
  float* const xl = swsm + C::DY_FLOATS;
  float* const coef = xl + C::X_FLOATS;                  // rows of 64: mean, rstd, scale, mean(g), mean(g * xhat), shift
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lp = lane & 31, lh = lane >> 5;
  const int mb = wave & 1, grp = wave >> 1;

  // the coefficients: bn_bwd_apply_kernel's preamble (fp32 storage, activation re-evaluated from y), one channel per thread
  if (tid < 64) {
    const int c = tid;
    const double inv = 1.0 / (double)a.pixels;
    double s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int r = 0; r < BN_REPLICAS; ++r) {
      s1 += a.bsums[(size_t)r * 2 * 64 + c];
      s2 += a.bsums[(size_t)r * 2 * 64 + 64 + c];
    }
    const float rs = a.rstd[c], mu = a.mean[c], gs = a.gamma[c] * rs;
    coef[c] = mu;
    coef[64 + c] = rs;
    coef[2 * 64 + c] = gs;
    coef[3 * 64 + c] = (float)(s1 * inv);
    coef[4 * 64 + c] = (float)(s2 * inv);
    coef[5 * 64 + c] = a.beta[c] - mu * gs;
    if (blockIdx.x == 0) {
      const float db = (float)s1, dg = (float)s2;
      if (a.dbeta) a.dbeta[c] = a.acc_param ? a.dbeta[c] + db : db;
      if (a.dgamma) a.dgamma[c] = a.acc_param ? a.dgamma[c] + dg : dg;
    }
  }

  // staging roles: dz / y vector i of this thread is channel quad q of slab pixel (row i, column prow); x piece i is input pixel
  // (band row, band pixel) = (piece / IP, piece % IP), piece = tid + i * NT
  const int q = tid & 15, prow = tid >> 4;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  f32x4 rdz[C::NQ], ry[C::NQ], rx[C::NI];
  unsigned vmask = 0, xmask = 0;                        // bit i: slab pixel (i, prow) is an output pixel / x piece i is inside the image
  // Every load is unconditional (a position outside the image reads element 0 of its tensor and is zeroed when it is stored to LDS):
  // a load under a branch is merged with its zero by register copies that wait for it, and the loads issued here must stay in flight
  // during the slab's MFMAs.
  auto load_slab = [&](int slab) {
    const int tx = slab % a.ntx, t2 = slab / a.ntx;
    const int ty = t2 % a.nty, img = t2 / a.nty;
    const int oy0 = ty * C::TH, ox0 = tx * C::TW;
    vmask = 0;
    xmask = 0;
#pragma unroll
    for (int i = 0; i < C::NQ; ++i) {
      const int oy = oy0 + i, ox = ox0 + prow;
      const bool ok = oy < a.ho && ox < a.wo;
      const size_t o = ok ? (((size_t)img * a.ho + oy) * a.wo + ox) * 64 + 4 * q : 0;
      rdz[i] = *reinterpret_cast<const f32x4*>(a.dz + o);
      ry[i] = *reinterpret_cast<const f32x4*>(a.y + o);
      vmask |= ok ? 1u << i : 0u;
    }
#pragma unroll
    for (int i = 0; i < C::NI; ++i) {
      const int piece = tid + i * C::NT;
      const int r = piece / C::IP, p = piece - r * C::IP;
      const int iy = 2 * oy0 - 3 + r, ix = 2 * ox0 - 3 + p;
      const bool ok = piece < C::NPIECE && (unsigned)iy < (unsigned)a.hi && (unsigned)ix < (unsigned)a.wi;
      rx[i] = *reinterpret_cast<const f32x4*>(a.x + (ok ? (((size_t)img * a.hi + iy) * a.wi + ix) * 4 : 0));
      xmask |= ok ? 1u << i : 0u;
    }
  };
  auto store_slab = [&]() {
    f32x4 mean, rstd, scale, mg, mgx, shift;
    mean = *reinterpret_cast<const f32x4*>(coef + 4 * q);
    rstd = *reinterpret_cast<const f32x4*>(coef + 64 + 4 * q);
    scale = *reinterpret_cast<const f32x4*>(coef + 2 * 64 + 4 * q);
    mg = *reinterpret_cast<const f32x4*>(coef + 3 * 64 + 4 * q);
    mgx = *reinterpret_cast<const f32x4*>(coef + 4 * 64 + 4 * q);
    shift = *reinterpret_cast<const f32x4*>(coef + 5 * 64 + 4 * q);
#pragma unroll
    for (int i = 0; i < C::NQ; ++i) {
      f32x4 out;
#pragma unroll
      for (int e = 0; e < 4; ++e) {                       // bn_bwd_apply_kernel's body, statement for statement
        const float zz = __builtin_fmaf(ry[i][e], scale[e], shift[e]);
        float gz = rdz[i][e];
        if (a.act != UDASEG_ACT_NONE) gz *= act_grad(zz, a.act, a.slope);
        const float xh = (ry[i][e] - mean[e]) * rstd[e];
        out[e] = scale[e] * (gz - mg[e] - xh * mgx[e]);
      }
      if (!((vmask >> i) & 1u)) out = zero4;              // outside the image: no pixel, no gradient
      *reinterpret_cast<f32x4*>(dyl + ((i * C::TW + prow) * 64 + 4 * q)) = out;
    }
#pragma unroll
    for (int i = 0; i < C::NI; ++i) {
      const int piece = tid + i * C::NT;
      if (i < C::NI - 1 || piece < C::NPIECE) {
        const int r = piece / C::IP, p = piece - r * C::IP;
        float* dst = xl + r * C::XS + 3 * p;
        const bool ok = (xmask >> i) & 1u;                // outside the image: zero padding
        // the dead fourth channel stays "used" until here: left dead, its register is handed to the MFMA loop's address arithmetic,
        // which then has to wait for the load that still owns it (s_waitcnt vmcnt(0) in front of the slab's MFMAs)
        asm volatile("" : : "v"(rx[i][3]));
        dst[0] = ok ? rx[i][0] : 0.f;
        dst[1] = ok ? rx[i][1] : 0.f;
        dst[2] = ok ? rx[i][2] : 0.f;
      }
    }
  };

  // column j = 32 nb + lp of this lane: (ky, t = 3 kx + c) = (j / 21, j % 21); the padded columns re-read column 0 and are dropped
  int colo[C::NB];
#pragma unroll
  for (int nb = 0; nb < C::NB; ++nb) {
    const int j = 32 * nb + lp;
    const int ky = j < C::COLS ? j / 21 : 0, t = j < C::COLS ? j - 21 * ky : 0;
    colo[nb] = ky * C::XS + t + 6 * lh;
  }
  f32x16 acc[C::NB];
#pragma unroll
  for (int nb = 0; nb < C::NB; ++nb)
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[nb][v] = 0.f;

  __syncthreads();                                       // the coefficients
  int slab = blockIdx.x;
  if (slab < a.nslabs) load_slab(slab);
  for (; slab < a.nslabs; slab += gridDim.x) {
    store_slab();
    __syncthreads();
    if (slab + (int)gridDim.x < a.nslabs) load_slab(slab + gridDim.x);
    // K-step s of this wave: output pixels (row 2 grp + (s >> 4), column 2 (s & 15) + lh) = slab pixel 64 grp + 2 s + lh
    const float* arow = dyl + (64 * grp + lh) * 64 + 32 * mb + lp;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const float* brow = xl + 2 * (2 * grp + half) * C::XS;
      const float* bcol[C::NB];
#pragma unroll
      for (int nb = 0; nb < C::NB; ++nb) bcol[nb] = brow + colo[nb];
#pragma unroll
      for (int ss = 0; ss < 16; ++ss) {
        const float av = arow[(16 * half + ss) * 128];
        float bv[C::NB];
#pragma unroll
        for (int nb = 0; nb < C::NB; ++nb) bv[nb] = bcol[nb][12 * ss];
#pragma unroll
        for (int nb = 0; nb < C::NB; ++nb) acc[nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv[nb], acc[nb], 0, 0, 0);
      }
    }
    __syncthreads();                                     // every wave is done with the slab before the next one overwrites it
  }

  // fold the four row groups in a fixed order: red[co][LDC] over the dy region (the slab loop ended with a barrier)
  float* const red = dyl;
  for (int g = 0; g < 4; ++g) {
    if (grp == g) {
#pragma unroll
      for (int nb = 0; nb < C::NB; ++nb)
#pragma unroll
        for (int v = 0; v < 16; ++v) {
          float* dst = red + (32 * mb + (v & 3) + 8 * (v >> 2) + 4 * lh) * C::LDC + 32 * nb + lp;
          *dst = g == 0 ? acc[nb][v] : *dst + acc[nb][v];
        }
    }
    __syncthreads();
  }
  for (int i = tid; i < 64 * C::COLS; i += C::NT) {
    const int co = i / C::COLS, j = i - co * C::COLS;
    const int ky = j / 21, t = j - 21 * ky;
    const int kx = t / 3, c = t - 3 * kx;
    atomicAdd(a.dw + ((co * 7 + ky) * 7 + kx) * 4 + c, red[co * C::LDC + j]);
  }
}

// dynamic LDS a block of the current device may opt in to (cached per device); 0 when there is no device
static int device_lds_optin() {
  static std::atomic<int> cache[16] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return 0;
  int v = cache[dev];
  if (v > 0) return v;
  int optin = 0, plain = 0;
  if (hipDeviceGetAttribute(&optin, hipDeviceAttributeSharedMemPerBlockOptin, dev) != hipSuccess) optin = 0;
  if (hipDeviceGetAttribute(&plain, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess) plain = 0;
  (void)hipGetLastError();
  v = optin > plain ? optin : plain;
  if (v > 0) cache[dev] = v;
  return v;
}

static bool stem_wgrad_geometry(const udaseg_conv_desc* d) {
  if (!d || d->kh != 7 || d->kw != 7 || d->stride != 2 || d->pad != 3 || d->ci != 4 || d->co != 64) return false;
  if (d->n <= 0 || d->hi < 1 || d->wi < 1 || d->ho != (d->hi - 1) / 2 + 1 || d->wo != (d->wi - 1) / 2 + 1) return false;
  const long long pin = (long long)d->n * d->hi * d->wi, pout = (long long)d->n * d->ho * d->wo;
  return pin * 16 < (1LL << 31) && pout * 256 < (1LL << 31);
}

}  // namespace udaseg

using namespace udaseg;

// 1: udaseg_conv2d_wgrad_stem_bn serves this layer on the current device (fp32 storage; ReLU / leaky layers without a residual input)
extern "C" int udaseg_conv_stem_wgrad_bn_ok(const udaseg_conv_desc* d) {
  if (opt_get(UDASEG_OPT_STEM_WGRAD_BN) == 0 || !stem_wgrad_geometry(d)) return 0;
  return device_lds_optin() >= StemWgradCfg::LDS ? 1 : 0;
}

extern "C" int udaseg_stem_wgrad_set_blocks(int blocks) {
  UDASEG_CHECK_ARG(blocks >= 0 && blocks <= 4096, "stem_wgrad_set_blocks: 0 (default) .. 4096");
  return udaseg_set_option(UDASEG_OPT_STEM_WGRAD_BLOCKS, blocks);
}

// dW[64][7][7][4] (+)= the weight gradient of the 7x7 / stride 2 / pad 3 stem from x and dy = bn_bwd_apply(dz, y), dy never stored;
// dgamma / dbeta as udaseg_bn_bwd_apply writes them.  accumulate = 0 zeroes the live entries of dW first; the fourth-channel entries
// are not touched either way.
extern "C" int udaseg_conv2d_wgrad_stem_bn(const udaseg_conv_desc* d, const float* x, const float* dz, const float* y,
                                           const float* save_mean, const float* save_rstd, const float* gamma, const float* beta,
                                           const double* bsums, int act, float slope, float* dw, float* dgamma, float* dbeta,
                                           int accumulate, int accumulate_param, void* stream) {
  UDASEG_CHECK_ARG(d && x && dz && y && save_mean && save_rstd && gamma && beta && bsums && dw, "conv2d_wgrad_stem_bn: NULL pointer");
  UDASEG_CHECK_ARG(act == UDASEG_ACT_LEAKY, "conv2d_wgrad_stem_bn: the layer's activation must be ReLU / leaky (got %d)", act);
  if (!udaseg_conv_stem_wgrad_bn_ok(d)) {
    set_error("conv2d_wgrad_stem_bn: not supported (7x7 / stride 2 / pad 3, 4 -> 64 channels, %d bytes of LDS per block; ask "
              "udaseg_conv_stem_wgrad_bn_ok first)", StemWgradCfg::LDS);
    return UDASEG_E_UNSUPPORTED;
  }
  using C = StemWgradCfg;
  StemWgradArgs a = {};
  a.x = x; a.dz = dz; a.y = y;
  a.mean = save_mean; a.rstd = save_rstd; a.gamma = gamma; a.beta = beta; a.bsums = bsums;
  a.dw = dw; a.dgamma = dgamma; a.dbeta = dbeta;
  a.n = d->n; a.hi = d->hi; a.wi = d->wi; a.ho = d->ho; a.wo = d->wo;
  a.ntx = cdiv(d->wo, C::TW);
  a.nty = cdiv(d->ho, C::TH);
  a.nslabs = d->n * a.nty * a.ntx;
  a.pixels = (long long)d->n * d->ho * d->wo;
  a.act = act; a.slope = slope; a.acc_param = accumulate_param;
  const int cus = device_cus();
  if (cus <= 0) return UDASEG_E_HIP;
  // One 8-wave block per CU, and never a block for fewer than MIN_SLABS slabs: a block's fixed part (the coefficient preamble, the
  // fold and its 64 x 147 atomics: ~7 us, the price of the second round of blocks in the block-count sweep) is half a slab's work,
  // so a small launch is shorter on few blocks.  It is also reproducible there: one block adds every element of dW once, and up to
  // two blocks add onto a zeroed gradient in either order with the same result -- a 2 x 32 x 32 step repeats bit for bit, as it did
  // on the split-K kernel, which took two K splits at that size.  UDASEG_OPT_STEM_WGRAD_BLOCKS (tests: a second trip through the slab
  // loop at a small shape; sweeps) sets the count itself.
  constexpr int MIN_SLABS = 4;
  const int forced = opt_get(UDASEG_OPT_STEM_WGRAD_BLOCKS);
  const int by_work = a.nslabs / MIN_SLABS > 1 ? a.nslabs / MIN_SLABS : 1;
  const int cap = forced > 0 ? forced : (by_work < cus ? by_work : cus);
  const int blocks = a.nslabs < cap ? a.nslabs : cap;
  hipStream_t st = as_stream(stream);
  if (!accumulate) {                    // before prof_begin: an early return must not leave the family's timing record open
    hipError_t e = hipMemset2DAsync(dw, 4 * sizeof(float), 0, 3 * sizeof(float), (size_t)64 * 49, st);
    if (e != hipSuccess) return hip_fail(e, "hipMemset2DAsync(dw)");
  }
  const double flops = 2.0 * (double)a.pixels * 64.0 * C::COLS;
  static KernelRec rec("hipFuncSetAttribute(conv_small_ci_wgrad)", "conv_small_ci_wgrad_kernel");
  prof_begin(1, st);
  const int rc = launch_kernel(rec, conv_small_ci_wgrad_kernel, dim3((unsigned)blocks), dim3(C::NT), C::LDS, C::LDS, st, flops,
                               "conv_small_ci_wgrad launch", a);
  prof_end(1, st, flops, 2, d);
  return rc;
}
