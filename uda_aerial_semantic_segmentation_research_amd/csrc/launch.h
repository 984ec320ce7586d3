// Host-side launch bookkeeping of the convolution kernels: the per-instantiation record (dynamic-LDS opt-in + timing id), the one
// function that launches through it, the CU count of the current device, and the tile-grid / statistics tail the halo-resident
// forward kernels share.  Host code only: nothing here is visible to a kernel.
#pragma once
#include "common.h"

namespace udaseg {

// One per kernel a launcher can start (a function-local static of the launcher template: plain, in-staging-transform and
// timeline instantiations each have their own).  The constructor formats the rocprofv3 symbol -- once per instantiation, under the
// language's guard for function-local statics -- so the string stands next to the template parameters it spells; the timing id is
// taken on the first launch.  Launches come from two host threads' streams: both flags are atomic, and a racing first launch sets
// the same attribute twice and registers the same name twice (kprof_id is serialised and returns the same id).
struct KernelRec {
  std::atomic<bool> lds_set{false};
  std::atomic<int> kid{-1};
  char name[160];
  const char* attr_what;      // hip_fail's text when the dynamic-LDS opt-in fails (nullptr: a kernel without dynamic LDS)
  __attribute__((format(printf, 3, 4))) KernelRec(const char* attr_what_, const char* name_fmt, ...) : attr_what(attr_what_) {
    va_list ap;
    va_start(ap, name_fmt);
    vsnprintf(name, sizeof(name), name_fmt, ap);
    va_end(ap);
  }
};

// Opt in to max_lds bytes of dynamic LDS (once per record; the 48 KB every kernel may use without asking needs no call), take
// the timing id, then kprof_begin / launch with lds bytes / kprof_end / check -- nothing that can fail stands between the two
// timing events.  flops: what kprof_end books (algorithmic bytes for the bandwidth-bound kernels); what: the launch check's text.
template <typename... P, typename... A>
static int launch_kernel(KernelRec& r, void (*kern)(P...), dim3 grid, dim3 block, int lds, int max_lds, hipStream_t s, double flops,
                         const char* what, A&&... args) {
  if (max_lds > 48 * 1024 && !r.lds_set) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, max_lds);
    if (e != hipSuccess) return hip_fail(e, r.attr_what);
    r.lds_set = true;
  }
  if (r.kid < 0) r.kid = kprof_id(r.name);
  hipEvent_t ev = kprof_begin(s);
  hipLaunchKernelGGL(kern, grid, block, lds, s, static_cast<A&&>(args)...);
  kprof_end(r.kid, ev, s, flops);
  UDASEG_LAUNCH_CHECK(what);
  return UDASEG_OK;
}

// RAII form for the bandwidth-bound kernels: `work` carries their ALGORITHMIC BYTES (bench.py reports TB/s for symbols that do
// not start with "conv").  Costs one atomic-int test per call when profiling is off.
struct KTimer {
  KernelRec& r;
  hipStream_t s;
  hipEvent_t ev;
  double work;
  KTimer(KernelRec& rec, hipStream_t st, double w) : r(rec), s(st), work(w) {
    if (r.kid < 0) r.kid = kprof_id(r.name);
    ev = kprof_begin(s);
  }
  ~KTimer() { kprof_end(r.kid, ev, s, work); }
};

// CU count of the CURRENT device for the persistent-grid launchers (cached per device); 0 after hip_fail has set the error text:
//   const int cus = device_cus();  if (cus <= 0) return UDASEG_E_HIP;
int device_cus();

// f64 partial-sum scratch of launches with more than 1024 blocks (udaseg_set_stats_scratch): the current device's, when it holds
// HALO_SCR_REPLICAS x 2 x co doubles, else nullptr; and the launch that folds it into the [R][2][co] accumulators
// One scratch per device, used by ONE stream: the first stream that asks owns it until the scratch is re-bound
// (udaseg_set_stats_scratch); a launch on any other stream gets nullptr and adds into the 16 replicas directly (correct, slower)
// instead of mixing its partial sums with the owner's in-flight launch (the contract was only written down before round 5).
double* halo_stats_scratch(int co, hipStream_t s);
void launch_halo_stats_fold(double* sscr, int co, double* stats, hipStream_t s);

// The tile grid of a halo-resident forward / data-gradient launch (HaloArgs, F3Args, UpArgs: the same field names): th x tw pixel
// tiles x blocks of cb produced channels; fills ntx / nty / ncb / nk16 and, for a launch with statistics and more than 1024 blocks,
// sscr.  Returns the block count (x classes: the parity classes of the 2 x 2-window data gradient).
template <typename Args>
static long long tile_launch_shape(Args& a, int th, int tw, int cb, hipStream_t s, int classes = 1) {
  a.ntx = cdiv(a.w, tw);
  a.nty = cdiv(a.h, th);
  a.ncb = cdiv(a.co, cb);
  a.nk16 = (a.ci + 15) / 16;
  const long long blocks = (long long)a.n * a.nty * a.ntx * a.ncb * classes;
  a.sscr = nullptr;
  if (a.stats != nullptr && blocks > 1024) a.sscr = halo_stats_scratch(a.co, s);
  return blocks;
}
// ... and its tail: rc of the launch, then the fold of the scratch the launch summed into
template <typename Args>
static int fold_stats(int rc, const Args& a, hipStream_t s) {
  if (rc != UDASEG_OK || a.sscr == nullptr) return rc;
  launch_halo_stats_fold(a.sscr, a.co, a.stats, s);
  UDASEG_LAUNCH_CHECK("halo_stats_fold launch");
  return UDASEG_OK;
}

}  // namespace udaseg
