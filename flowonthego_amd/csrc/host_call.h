// host_call.h -- the host-side scaffold every C-ABI file (fotg_<feature>.hip) shares: run on the context's device, report a HIP
// failure, read a context's coarse flow in a fused entry point, refuse aliasing arguments (spans.h), own the stream-ordered memory
// of one call, opt a kernel in to more dynamic LDS than the default limit.  An entry point decides FOTG_ERR_ARG first, from its
// arguments alone, and only then takes a DevGuard.
#pragma once
#include <map>
#include <mutex>
#include <utility>
#include "common.h"
#include "flowsrc.hip.h"
#include "spans.h"

// run on `dev`, leave the caller's current device as it was
struct DevGuard {
  int prev = -1;
  bool ok = false;
  hipError_t err = hipSuccess;       // what the failing hipGetDevice / hipSetDevice returned
  explicit DevGuard(int dev)
  {
    int cur = -1;
    if ((err = hipGetDevice(&cur)) != hipSuccess) return;
    if (cur == dev) { ok = true; return; }
    if ((err = hipSetDevice(dev)) != hipSuccess) return;
    prev = cur; ok = true;
  }
  ~DevGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

namespace fotg {
namespace {                          // (internal to each file, as the pasted copies were)

int hip_fail(hipError_t e)
{
  set_last_hip_error((int)e);
  return FOTG_ERR_HIP;
}

// The start of a fused (fotg_upsample_crop_*) entry point: the context's final-scale geometry, and n of its coarse flows at
// `flow`.  false = FOTG_ERR_ARG.  (An entry point with another batch rule -- temporal's n K, interp's bidir -- spells its own.)
bool fused_geom(const fotg_ctx *ctx, int n, const float *flow, CtxUpsampleGeom *g)
{
  if (!ctx || !flow || ctx_upsample_geom(ctx, g) != FOTG_OK) return false;
  return n >= 1 && n <= g->max_batch && g->nch == 2;
}

UpsampleSrc upsample_src(const CtxUpsampleGeom &g, const float *flow)
{
  return UpsampleSrc{flow, (long)g.wl * g.hl * 2, g.wl, g.hl, g.sc_l, g.x0, g.y0};
}

// The stream-ordered memory of one call.  get() allocates on the stream, unless an earlier get() failed (`err` keeps the first
// failure); finish(e) frees what was obtained, latest first, and turns e -- the call's error so far -- into its return value: a
// failing free surfaces only when nothing failed before it.
struct Scratch {
  hipStream_t stream;
  hipError_t err = hipSuccess;
  void *mem[5];                      // (flowfilter takes five; a sixth get() fails rather than leaks)
  int n = 0;
  explicit Scratch(hipStream_t s) : stream(s) {}
  template <class T>
  bool get(T **p, size_t bytes)
  {
    if (err != hipSuccess) return false;
    err = n < 5 ? hipMallocAsync((void **)p, bytes, stream) : hipErrorInvalidValue;
    if (err == hipSuccess) mem[n++] = *p;
    return err == hipSuccess;
  }
  int finish(hipError_t e)
  {
    while (n > 0) {
      const hipError_t ef = hipFreeAsync(mem[--n], stream);
      if (e == hipSuccess) e = ef;
    }
    return e == hipSuccess ? FOTG_OK : hip_fail(e);
  }
};

// hipFuncAttributeMaxDynamicSharedMemorySize is a per-device property of a kernel: opt kernel fn in to lds bytes once per (kernel,
// device), on the current device.  Contexts / pipes / calls driven from different host threads share the file's cache.
std::mutex g_lds_mu;
std::map<std::pair<const void *, int>, int> g_lds_set;
template <typename... A>
hipError_t lds_opt_in(void (*fn)(A...), int lds)
{
  std::lock_guard<std::mutex> lock(g_lds_mu);
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  int &have = g_lds_set[{reinterpret_cast<const void *>(fn), dev}];
  if (lds <= have) return hipSuccess;
  e = hipFuncSetAttribute(reinterpret_cast<const void *>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  if (e == hipSuccess) have = lds;
  return e;
}

}  // namespace
}  // namespace fotg
