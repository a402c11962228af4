// fotg_temporal.hip -- C-ABI of the motion-compensated temporal filter (include/fotg.h fotg_temporal_filter /
// fotg_upsample_crop_temporal_filter and their 8-bit forms), kernels in temporal.hip.h.  Per call: the validated frame indices
// copied into stream-ordered memory of the call, one launch over every output image and, when statistics are asked for, a second
// small launch that folds the per-workgroup partials.  The gains travel by value in the kernel arguments.  Everything is enqueued
// on the caller's stream; the host arrays are consumed before the call returns.
#include <cmath>
#include <vector>
#include "host_call.h"
#include "temporal.hip.h"

using namespace fotg;

namespace {

template <class Src, class T>
int temporal_batch(int device, int n, int K, int nframes, const Src &flow, const T *frames, int w, int h, int channels,
                   const int *center, const int *neighbors, const unsigned char *masks, float tau, const float *gains, const T *ref,
                   T *dst, unsigned char *used, double *stats, void *stream_)
{
  if (n < 1 || K < 1 || K > TEMPORAL_MAXK || nframes < 1 || w <= 0 || h <= 0 || (channels != 1 && channels != 3)) return FOTG_ERR_ARG;
  if (!frames || !center || !neighbors || !(tau > 0.f) || !std::isfinite(tau)) return FOTG_ERR_ARG;
  if (!dst && !used && !stats) return FOTG_ERR_ARG;
  TemporalGains gn;
  for (int k = 0; k < TEMPORAL_MAXK; ++k) {
    gn.g[k] = k < K && gains ? gains[k] : (k < K ? 1.0f : 0.0f);
    if (!std::isfinite(gn.g[k]) || gn.g[k] < 0.f) return FOTG_ERR_ARG;
  }
  std::vector<int> ix((size_t)n * (K + 1));
  for (int i = 0; i < n; ++i) {
    if (center[i] < 0 || center[i] >= nframes) return FOTG_ERR_ARG;
    ix[(size_t)i * (K + 1)] = center[i];
    for (int k = 0; k < K; ++k) {
      const int b = neighbors[(size_t)i * K + k];
      if (b < -1 || b >= nframes) return FOTG_ERR_ARG;
      ix[(size_t)i * (K + 1) + 1 + k] = b;
    }
  }
  const long hw = (long)w * h;
  const long tiles_x = ((long)w + TEMPORAL_TW - 1) / TEMPORAL_TW, tiles_y = ((long)h + TEMPORAL_TH - 1) / TEMPORAL_TH;
  const long blocks = tiles_x * tiles_y;
  if (blocks > 0x7fffffffL || tiles_y > 65535 || n > 65535) return FOTG_ERR_ARG;
  // the taps of a frame are read after pixels of dst have been written: no filtering in place
  const size_t img = (size_t)hw * channels * sizeof(T);
  if (overlap(Span{frames, nframes * img}, Span{dst, n * img})) return FOTG_ERR_ARG;
  const float scale = 1.0f / (tau * (float)(9 * channels));
  DevGuard guard(device);
  if (!guard.ok) return hip_fail(guard.err);
  hipStream_t stream = (hipStream_t)stream_;
  int *dix = nullptr;
  WarpPartial *part = nullptr;
  Scratch mem(stream);
  mem.get(&dix, ix.size() * sizeof(int));
  if (stats) mem.get(&part, (size_t)n * blocks * sizeof(WarpPartial));
  if (mem.err != hipSuccess) return mem.finish(mem.err);
  hipError_t e = hipMemcpyAsync(dix, ix.data(), ix.size() * sizeof(int), hipMemcpyHostToDevice, stream);   // pageable: consumed on return
  if (e == hipSuccess) {
    const dim3 grid((unsigned)tiles_x, (unsigned)tiles_y, (unsigned)n);
    if (channels == 1)
      temporal_kernel<Src, T, 1><<<grid, WARP_THREADS, 0, stream>>>(flow, frames, ref, masks, dix, K, w, h, scale, gn, dst, used, part);
    else
      temporal_kernel<Src, T, 3><<<grid, WARP_THREADS, 0, stream>>>(flow, frames, ref, masks, dix, K, w, h, scale, gn, dst, used, part);
    e = hipGetLastError();
  }
  if (stats && e == hipSuccess) {
    temporal_fold_kernel<<<dim3((unsigned)n), WARP_THREADS, 0, stream>>>(part, (int)blocks, stats);
    e = hipGetLastError();
  }
  return mem.finish(e);
}

template <class T>
int temporal_fused(fotg_ctx *ctx, int n, int K, int nframes, const float *flows, const T *frames, int channels, const int *center,
                   const int *neighbors, const unsigned char *masks, float tau, const float *gains, const T *ref, T *dst,
                   unsigned char *used, double *stats, void *stream)
{
  CtxUpsampleGeom g;
  if (!ctx || !flows || ctx_upsample_geom(ctx, &g) != FOTG_OK) return FOTG_ERR_ARG;
  if (n < 1 || K < 1 || K > TEMPORAL_MAXK || (long)n * K > g.max_batch || g.nch != 2) return FOTG_ERR_ARG;
  return temporal_batch(g.device, n, K, nframes, upsample_src(g, flows), frames, g.w_org, g.h_org, channels, center, neighbors, masks,
                        tau, gains, ref, dst, used, stats, stream);
}

}  // namespace

extern "C" {

int fotg_temporal_filter(int device, int n, int K, int T, const float *frames, int w, int h, int channels, const int *center,
                         const int *neighbors, const float *flows, const unsigned char *masks, float tau, const float *gains,
                         const float *ref, float *dst, unsigned char *used, double *stats, void *stream)
{
  if (!flows) return FOTG_ERR_ARG;
  return temporal_batch(device, n, K, T, DenseSrc{flows}, frames, w, h, channels, center, neighbors, masks, tau, gains, ref, dst,
                        used, stats, stream);
}

int fotg_temporal_filter_u8(int device, int n, int K, int T, const unsigned char *frames, int w, int h, int channels,
                            const int *center, const int *neighbors, const float *flows, const unsigned char *masks, float tau,
                            const float *gains, const unsigned char *ref, unsigned char *dst, unsigned char *used, double *stats,
                            void *stream)
{
  if (!flows) return FOTG_ERR_ARG;
  return temporal_batch(device, n, K, T, DenseSrc{flows}, frames, w, h, channels, center, neighbors, masks, tau, gains, ref, dst,
                        used, stats, stream);
}

int fotg_upsample_crop_temporal_filter(fotg_ctx *ctx, int n, int K, int T, const float *coarse_flows, const float *frames,
                                       int channels, const int *center, const int *neighbors, const unsigned char *masks, float tau,
                                       const float *gains, const float *ref, float *dst, unsigned char *used, double *stats,
                                       void *stream)
{
  return temporal_fused(ctx, n, K, T, coarse_flows, frames, channels, center, neighbors, masks, tau, gains, ref, dst, used, stats,
                        stream);
}

int fotg_upsample_crop_temporal_filter_u8(fotg_ctx *ctx, int n, int K, int T, const float *coarse_flows,
                                          const unsigned char *frames, int channels, const int *center, const int *neighbors,
                                          const unsigned char *masks, float tau, const float *gains, const unsigned char *ref,
                                          unsigned char *dst, unsigned char *used, double *stats, void *stream)
{
  return temporal_fused(ctx, n, K, T, coarse_flows, frames, channels, center, neighbors, masks, tau, gains, ref, dst, used, stats,
                        stream);
}

}  // extern "C"
