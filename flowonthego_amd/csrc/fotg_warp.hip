// fotg_warp.hip -- C-ABI of the frame warp (include/fotg.h fotg_warp / fotg_upsample_crop_warp and their 8-bit forms), kernels in
// warp.hip.h.  Per call: one launch over every image of the batch and, when statistics are asked for, a second small launch that
// folds the per-workgroup partials (stream-ordered memory of the call) into them.  Asynchronous on the caller's stream; no host
// synchronisation.
#include "common.h"
#define FOTG_WARP_FOLD_KERNEL
#include "warp.hip.h"

using namespace fotg;

hipError_t fotg::warp_fold(const WarpPartial *part, int blocks, int n, double *stats, hipStream_t stream)
{
  warp_fold_kernel<<<dim3((unsigned)n), WARP_THREADS, 0, stream>>>(part, blocks, stats);
  return hipGetLastError();
}

namespace {

struct DevGuard {                    // run on `dev`, leave the caller's current device as it was
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

int hip_fail(hipError_t e)
{
  set_last_hip_error((int)e);
  return FOTG_ERR_HIP;
}

template <class Src, class T>
int warp_batch(int device, int n, const Src &flow, const T *src, int w, int h, int channels, const T *ref, const unsigned char *occ,
               int fill_mode, float fill, T *dst, unsigned char *code, double *stats, void *stream_)
{
  if (n < 1 || !src || w <= 0 || h <= 0 || (channels != 1 && channels != 3) || (fill_mode != 0 && fill_mode != 1)) return FOTG_ERR_ARG;
  if (!dst && !code && !stats) return FOTG_ERR_ARG;
  const long hw = (long)w * h;
  const long blocks = ((hw + 3) / 4 + WARP_THREADS - 1) / WARP_THREADS;
  if (blocks > 0x7fffffffL || n > 65535) return FOTG_ERR_ARG;
  if (dst) {                         // the taps of a pixel are read after other pixels have been written: no warp in place
    const size_t bytes = (size_t)n * hw * channels * sizeof(T);
    const char *a = reinterpret_cast<const char *>(src), *b = reinterpret_cast<const char *>(dst);
    if (a < b + bytes && b < a + bytes) return FOTG_ERR_ARG;
  }
  DevGuard guard(device);
  if (!guard.ok) return hip_fail(guard.err);
  hipStream_t stream = (hipStream_t)stream_;
  WarpPartial *part = nullptr;
  if (stats) {
    const hipError_t e = hipMallocAsync((void **)&part, (size_t)n * blocks * sizeof(WarpPartial), stream);
    if (e != hipSuccess) return hip_fail(e);
  }
  const dim3 grid((unsigned)blocks, (unsigned)n);
  if (channels == 1)
    warp_kernel<Src, T, 1><<<grid, WARP_THREADS, 0, stream>>>(flow, src, ref, occ, w, h, fill_mode, fill, dst, code, part);
  else
    warp_kernel<Src, T, 3><<<grid, WARP_THREADS, 0, stream>>>(flow, src, ref, occ, w, h, fill_mode, fill, dst, code, part);
  hipError_t e = hipGetLastError();
  if (stats) {
    if (e == hipSuccess) {
      e = warp_fold(part, (int)blocks, n, stats, stream);
    }
    const hipError_t ef = hipFreeAsync(part, stream);
    if (e == hipSuccess) e = ef;
  }
  return e == hipSuccess ? FOTG_OK : hip_fail(e);
}

template <class T>
int warp_fused(fotg_ctx *ctx, int n, const float *flow, const T *src, int channels, const T *ref, const unsigned char *occ,
               int fill_mode, float fill, T *dst, unsigned char *code, double *stats, void *stream)
{
  CtxUpsampleGeom g;
  if (!ctx || !flow || ctx_upsample_geom(ctx, &g) != FOTG_OK) return FOTG_ERR_ARG;
  if (n < 1 || n > g.max_batch || g.nch != 2) return FOTG_ERR_ARG;
  const UpsampleSrc f{flow, (long)g.wl * g.hl * 2, g.wl, g.hl, g.sc_l, g.x0, g.y0};
  return warp_batch(g.device, n, f, src, g.w_org, g.h_org, channels, ref, occ, fill_mode, fill, dst, code, stats, stream);
}

}  // namespace

extern "C" {

int fotg_warp(int device, int n, const float *src, const float *flow, int w, int h, int channels, const float *ref,
              const unsigned char *occ, int fill_mode, float fill, float *dst, unsigned char *code, double *stats, void *stream)
{
  if (!flow) return FOTG_ERR_ARG;
  return warp_batch(device, n, DenseSrc{flow}, src, w, h, channels, ref, occ, fill_mode, fill, dst, code, stats, stream);
}

int fotg_warp_u8(int device, int n, const unsigned char *src, const float *flow, int w, int h, int channels, const unsigned char *ref,
                 const unsigned char *occ, int fill_mode, float fill, unsigned char *dst, unsigned char *code, double *stats, void *stream)
{
  if (!flow) return FOTG_ERR_ARG;
  return warp_batch(device, n, DenseSrc{flow}, src, w, h, channels, ref, occ, fill_mode, fill, dst, code, stats, stream);
}

int fotg_upsample_crop_warp(fotg_ctx *ctx, int n, const float *coarse_flow, const float *src, int channels, const float *ref,
                            const unsigned char *occ, int fill_mode, float fill, float *dst, unsigned char *code, double *stats,
                            void *stream)
{
  return warp_fused(ctx, n, coarse_flow, src, channels, ref, occ, fill_mode, fill, dst, code, stats, stream);
}

int fotg_upsample_crop_warp_u8(fotg_ctx *ctx, int n, const float *coarse_flow, const unsigned char *src, int channels,
                               const unsigned char *ref, const unsigned char *occ, int fill_mode, float fill, unsigned char *dst,
                               unsigned char *code, double *stats, void *stream)
{
  return warp_fused(ctx, n, coarse_flow, src, channels, ref, occ, fill_mode, fill, dst, code, stats, stream);
}

}  // extern "C"
