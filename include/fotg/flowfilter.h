// include/fotg/flowfilter.h -- edge- and occlusion-aware filtering of a flow over the C-ABI of libfotg.so (fotg_flow_filter /
// fotg_upsample_crop_flow_filter and their 8-bit-guide forms): a joint bilateral filter of the vectors guided by the frame the flow
// belongs to; vectors a consistency mask rejects stay out of the means and are filled from their neighbours.  flow, guide, mask and
// the outputs are device pointers; spatial is a HOST array, consumed before the call returns.  Asynchronous on `stream` (a
// hipStream_t, 0 = the null stream); each call returns a FOTG_* status.  The definition is in include/fotg.h.
// Stream-ordered memory: a second call on a stream whose earlier call is still pending may wait on the host (include/fotg.h,
// STREAM-ORDERED MEMORY); the first returns at once.
#ifndef FOTG_FLOWFILTER_HEADER
#define FOTG_FLOWFILTER_HEADER
#include <cmath>
#include "../fotg.h"

namespace OFC {

enum { FLOWFILTER_MAX_RADIUS = 7, FLOWFILTER_MAX_ITERS = 4 };
// code: per pixel
enum FlowFilterCode { FLOWFILTER_FILTERED = 0, FLOWFILTER_FILLED = 1, FLOWFILTER_UNSUPPORTED = 3 };
// stats: per image four doubles
enum FlowFilterStat { FLOWFILTER_N_FILTERED = 0, FLOWFILTER_N_FILLED = 1, FLOWFILTER_N_UNSUPPORTED = 2, FLOWFILTER_SUM_ABS_CHANGE = 3 };

// the Gaussian table s[i] = exp(-i^2 / (2 sigma^2)), i = 0 .. radius, evaluated in double and rounded to float; s holds radius + 1
inline void FlowFilterSpatialTable(int radius, double sigma, float *s)
{
  for (int i = 0; i <= radius; ++i) s[i] = (float)std::exp(-(double)(i * i) / (2.0 * sigma * sigma));
}

// flow: n x height x width x 2 float32; guide: n x height x width x channels float32 or 8-bit, channels 1 or 3; out: the filtered
// flow (not overlapping flow).  code (n x height x width uint8), stats (n x 4 double), mask (n x height x width uint8, a mask of
// FbCheck) and spatial (radius + 1 floats in [0, 1], the first > 0; NULL = all 1) may be NULL.
inline int FlowFilter(const float *flow, const float *guide, int width, int height, int channels, int n, float *out,
                      unsigned char *code = nullptr, double *stats = nullptr, const unsigned char *mask = nullptr, int radius = 3,
                      const float *spatial = nullptr, float tau = 20.f, int iters = 1, int device = 0, void *stream = nullptr)
{
  return fotg_flow_filter(device, n, flow, guide, width, height, channels, mask, radius, spatial, tau, iters, out, code, stats,
                          stream);
}
inline int FlowFilter(const float *flow, const unsigned char *guide, int width, int height, int channels, int n, float *out,
                      unsigned char *code = nullptr, double *stats = nullptr, const unsigned char *mask = nullptr, int radius = 3,
                      const float *spatial = nullptr, float tau = 20.f, int iters = 1, int device = 0, void *stream = nullptr)
{
  return fotg_flow_filter_u8(device, n, flow, guide, width, height, channels, mask, radius, spatial, tau, iters, out, code, stats,
                             stream);
}

// the same on a context's coarse flow (n of fotg_out_size, n <= max_batch), upsampled and cropped on the fly: guide, mask and the
// outputs at the original frame size; the unfiltered full-resolution flow is never written
inline int UpsampleCropFlowFilter(fotg_ctx *ctx, const float *coarse_flow, const float *guide, int channels, int n, float *out,
                                  unsigned char *code = nullptr, double *stats = nullptr, const unsigned char *mask = nullptr,
                                  int radius = 3, const float *spatial = nullptr, float tau = 20.f, int iters = 1,
                                  void *stream = nullptr)
{
  return fotg_upsample_crop_flow_filter(ctx, n, coarse_flow, guide, channels, mask, radius, spatial, tau, iters, out, code, stats,
                                        stream);
}
inline int UpsampleCropFlowFilter(fotg_ctx *ctx, const float *coarse_flow, const unsigned char *guide, int channels, int n,
                                  float *out, unsigned char *code = nullptr, double *stats = nullptr,
                                  const unsigned char *mask = nullptr, int radius = 3, const float *spatial = nullptr,
                                  float tau = 20.f, int iters = 1, void *stream = nullptr)
{
  return fotg_upsample_crop_flow_filter_u8(ctx, n, coarse_flow, guide, channels, mask, radius, spatial, tau, iters, out, code, stats,
                                           stream);
}

}  // namespace OFC
#endif
