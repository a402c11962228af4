// fotg_warp.hip -- C-ABI of the frame warp (include/fotg.h fotg_warp / fotg_upsample_crop_warp and their 8-bit forms), kernels in
// warp.hip.h.  Per call: one launch over every image of the batch and, when statistics are asked for, a second small launch that
// folds the per-workgroup partials (stream-ordered memory of the call) into them.  Asynchronous on the caller's stream; no host
// synchronisation.
#include "host_call.h"
#define FOTG_WARP_FOLD_KERNEL
#include "warp.hip.h"

using namespace fotg;

hipError_t fotg::warp_fold(const WarpPartial *part, int blocks, int n, double *stats, hipStream_t stream)
{
  warp_fold_kernel<<<dim3((unsigned)n), WARP_THREADS, 0, stream>>>(part, blocks, stats);
  return hipGetLastError();
}

namespace {

template <class Src, class T>
int warp_batch(int device, int n, const Src &flow, const T *src, int w, int h, int channels, const T *ref, const unsigned char *occ,
               int fill_mode, float fill, T *dst, unsigned char *code, double *stats, void *stream_)
{
  if (n < 1 || !src || w <= 0 || h <= 0 || (channels != 1 && channels != 3) || (fill_mode != 0 && fill_mode != 1)) return FOTG_ERR_ARG;
  if (!dst && !code && !stats) return FOTG_ERR_ARG;
  const long hw = (long)w * h;
  const long blocks = ((hw + 3) / 4 + WARP_THREADS - 1) / WARP_THREADS;
  if (blocks > 0x7fffffffL || n > 65535) return FOTG_ERR_ARG;
  const size_t bytes = (size_t)n * hw * channels * sizeof(T);
  // the taps of a pixel are read after other pixels have been written: no warp in place
  if (overlap(Span{src, bytes}, Span{dst, bytes})) return FOTG_ERR_ARG;
  DevGuard guard(device);
  if (!guard.ok) return hip_fail(guard.err);
  hipStream_t stream = (hipStream_t)stream_;
  WarpPartial *part = nullptr;
  Scratch mem(stream);
  if (stats && !mem.get(&part, (size_t)n * blocks * sizeof(WarpPartial))) return mem.finish(mem.err);
  const dim3 grid((unsigned)blocks, (unsigned)n);
  if (channels == 1)
    warp_kernel<Src, T, 1><<<grid, WARP_THREADS, 0, stream>>>(flow, src, ref, occ, w, h, fill_mode, fill, dst, code, part);
  else
    warp_kernel<Src, T, 3><<<grid, WARP_THREADS, 0, stream>>>(flow, src, ref, occ, w, h, fill_mode, fill, dst, code, part);
  hipError_t e = hipGetLastError();
  if (stats && e == hipSuccess) e = warp_fold(part, (int)blocks, n, stats, stream);
  return mem.finish(e);
}

template <class T>
int warp_fused(fotg_ctx *ctx, int n, const float *flow, const T *src, int channels, const T *ref, const unsigned char *occ,
               int fill_mode, float fill, T *dst, unsigned char *code, double *stats, void *stream)
{
  CtxUpsampleGeom g;
  if (!fused_geom(ctx, n, flow, &g)) return FOTG_ERR_ARG;
  return warp_batch(g.device, n, upsample_src(g, flow), src, g.w_org, g.h_org, channels, ref, occ, fill_mode, fill, dst, code, stats,
                    stream);
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
