// fotg_flowfilter.hip -- C-ABI of the edge- and occlusion-aware flow filter (include/fotg.h fotg_flow_filter /
// fotg_upsample_crop_flow_filter and their 8-bit-guide forms), kernels in flowfilter.hip.h.  Per call: one launch per pass and,
// when statistics are asked for, a second small launch that folds the per-workgroup partials of the last pass.  Between passes the
// vectors ping-pong between `out` and stream-ordered memory of the call, the pass codes between two byte planes of that memory.
// The spatial table travels by value in the kernel arguments.  Everything is enqueued on the caller's stream; the host array is
// consumed before the call returns.
#include <cmath>
#include "host_call.h"
#include "flowfilter.hip.h"

using namespace fotg;

namespace {

template <class Src, class T, int NOC>
hipError_t launch_pass(const dim3 &grid, hipStream_t stream, const Src &flow, const float *prev, const T *guide,
                       const unsigned char *mask, int mask_mode, int w, int h, int R, float scale, const FlowFilterSpatial &sp,
                       float *out, unsigned char *code, int code_mode, WarpPartial *part)
{
  flowfilter_kernel<Src, T, NOC><<<grid, WARP_THREADS, flowfilter_lds_bytes<T, NOC>(R), stream>>>(
      flow, prev, guide, mask, mask_mode, w, h, R, scale, sp, out, code, code_mode, part);
  return hipGetLastError();
}

// flow_bytes: the extent of the memory behind `flow`, which `out` may not overlap
template <class Src, class T>
int filter_batch(int device, int n, const Src &flow, const void *flow_mem, size_t flow_bytes, const T *guide, int w, int h,
                 int channels, const unsigned char *mask, int R, const float *spatial, float tau, int iters, float *out,
                 unsigned char *code, double *stats, void *stream_)
{
  if (n < 1 || w <= 0 || h <= 0 || (channels != 1 && channels != 3)) return FOTG_ERR_ARG;
  if (R < 1 || R > FLOWFILTER_MAXR || iters < 1 || iters > FLOWFILTER_MAXITERS) return FOTG_ERR_ARG;
  if (!flow_mem || !guide || !(tau > 0.f) || !std::isfinite(tau)) return FOTG_ERR_ARG;
  if (!out && !code && !stats) return FOTG_ERR_ARG;
  FlowFilterSpatial sp;
  for (int i = 0; i <= FLOWFILTER_MAXR; ++i) {
    sp.s[i] = i <= R ? (spatial ? spatial[i] : 1.0f) : 0.0f;
    if (!std::isfinite(sp.s[i]) || sp.s[i] < 0.f || sp.s[i] > 1.f) return FOTG_ERR_ARG;
  }
  if (!(sp.s[0] > 0.f)) return FOTG_ERR_ARG;
  const long hw = (long)w * h;
  const long tiles_x = ((long)w + FLOWFILTER_TW - 1) / FLOWFILTER_TW, tiles_y = ((long)h + FLOWFILTER_TH - 1) / FLOWFILTER_TH;
  const long blocks = tiles_x * tiles_y;
  if (blocks > 0x7fffffffL || tiles_y > 65535 || n > 65535) return FOTG_ERR_ARG;
  const size_t vbytes = (size_t)n * hw * 2 * sizeof(float);
  if (overlap(Span{flow_mem, flow_bytes}, Span{out, vbytes})) return FOTG_ERR_ARG;  // a window reads what a neighbour's thread writes
  const float scale = 1.0f / (tau * (float)channels);
  DevGuard guard(device);
  if (!guard.ok) return hip_fail(guard.err);
  hipStream_t stream = (hipStream_t)stream_;

  // memory of the call: the vectors between the passes (one buffer beside `out`; two without it, from three passes on), the pass
  // codes (two byte planes) and the partial sums
  float *tmp[2] = {nullptr, nullptr};
  unsigned char *pc[2] = {nullptr, nullptr};
  WarpPartial *part = nullptr;
  Scratch mem(stream);
  if (iters > 1) {
    mem.get(&tmp[0], vbytes);
    if (!out && iters > 2) mem.get(&tmp[1], vbytes);
    mem.get(&pc[0], (size_t)n * hw);
    if (iters > 2) mem.get(&pc[1], (size_t)n * hw);
  }
  if (stats) mem.get(&part, (size_t)n * blocks * sizeof(WarpPartial));
  hipError_t e = mem.err;

  const dim3 grid((unsigned)tiles_x, (unsigned)tiles_y, (unsigned)n);
  const float *prev = nullptr;
  const unsigned char *prev_code = nullptr;
  for (int k = 1; k <= iters && e == hipSuccess; ++k) {
    const bool last = k == iters;
    // the last pass writes `out`; the passes before it alternate so that pass k never writes what it reads
    float *dstv = last ? out : (((iters - k) & 1) ? tmp[0] : (out ? out : tmp[1]));
    unsigned char *dstc = last ? code : pc[(k - 1) & 1];
    const unsigned char *m = k == 1 ? mask : prev_code;
    const int mm = k == 1 ? FLOWFILTER_MASK_USER : FLOWFILTER_MASK_PASS, cm = last ? FLOWFILTER_CODE_FINAL : FLOWFILTER_CODE_PASS;
    WarpPartial *pp = last ? part : nullptr;
    if (channels == 1)
      e = launch_pass<Src, T, 1>(grid, stream, flow, prev, guide, m, mm, w, h, R, scale, sp, dstv, dstc, cm, pp);
    else
      e = launch_pass<Src, T, 3>(grid, stream, flow, prev, guide, m, mm, w, h, R, scale, sp, dstv, dstc, cm, pp);
    prev = dstv; prev_code = dstc;
  }
  if (stats && e == hipSuccess) {
    flowfilter_fold_kernel<<<dim3((unsigned)n), WARP_THREADS, 0, stream>>>(part, (int)blocks, stats);
    e = hipGetLastError();
  }
  return mem.finish(e);
}

template <class T>
int filter_dense(int device, int n, const float *flow, const T *guide, int w, int h, int channels, const unsigned char *mask, int R,
                 const float *spatial, float tau, int iters, float *out, unsigned char *code, double *stats, void *stream)
{
  const size_t fbytes = n > 0 && w > 0 && h > 0 ? (size_t)n * w * h * 2 * sizeof(float) : 0;
  return filter_batch(device, n, DenseSrc{flow}, flow, fbytes, guide, w, h, channels, mask, R, spatial, tau, iters, out, code, stats,
                      stream);
}

template <class T>
int filter_fused(fotg_ctx *ctx, int n, const float *coarse, const T *guide, int channels, const unsigned char *mask, int R,
                 const float *spatial, float tau, int iters, float *out, unsigned char *code, double *stats, void *stream)
{
  CtxUpsampleGeom g;
  if (!fused_geom(ctx, n, coarse, &g)) return FOTG_ERR_ARG;
  return filter_batch(g.device, n, upsample_src(g, coarse), coarse, (size_t)n * g.wl * g.hl * 2 * sizeof(float), guide, g.w_org,
                      g.h_org, channels, mask, R, spatial, tau, iters, out, code, stats, stream);
}

}  // namespace

extern "C" {

int fotg_flow_filter(int device, int n, const float *flow, const float *guide, int w, int h, int channels, const unsigned char *mask,
                     int radius, const float *spatial, float tau, int iters, float *out, unsigned char *code, double *stats,
                     void *stream)
{
  return filter_dense(device, n, flow, guide, w, h, channels, mask, radius, spatial, tau, iters, out, code, stats, stream);
}

int fotg_flow_filter_u8(int device, int n, const float *flow, const unsigned char *guide, int w, int h, int channels,
                        const unsigned char *mask, int radius, const float *spatial, float tau, int iters, float *out,
                        unsigned char *code, double *stats, void *stream)
{
  return filter_dense(device, n, flow, guide, w, h, channels, mask, radius, spatial, tau, iters, out, code, stats, stream);
}

int fotg_upsample_crop_flow_filter(fotg_ctx *ctx, int n, const float *coarse_flow, const float *guide, int channels,
                                   const unsigned char *mask, int radius, const float *spatial, float tau, int iters, float *out,
                                   unsigned char *code, double *stats, void *stream)
{
  return filter_fused(ctx, n, coarse_flow, guide, channels, mask, radius, spatial, tau, iters, out, code, stats, stream);
}

int fotg_upsample_crop_flow_filter_u8(fotg_ctx *ctx, int n, const float *coarse_flow, const unsigned char *guide, int channels,
                                      const unsigned char *mask, int radius, const float *spatial, float tau, int iters, float *out,
                                      unsigned char *code, double *stats, void *stream)
{
  return filter_fused(ctx, n, coarse_flow, guide, channels, mask, radius, spatial, tau, iters, out, code, stats, stream);
}

}  // extern "C"
