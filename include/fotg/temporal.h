// include/fotg/temporal.h -- motion-compensated temporal filtering over the C-ABI of libfotg.so (fotg_temporal_filter /
// fotg_upsample_crop_temporal_filter and their 8-bit forms): the neighbours of a centre frame pulled onto it along their flows and
// averaged with it, each with a per-pixel weight that falls with the photometric difference in a 3 x 3 window.  frames, flows,
// masks, ref and the outputs are device pointers; center, neighbors and gains are HOST arrays, consumed before the call returns.
// Asynchronous on `stream` (a hipStream_t, 0 = the null stream); each call returns a FOTG_* status.  The definition is in
// include/fotg.h.
// Stream-ordered memory: a second call on a stream whose earlier call is still pending may wait on the host (include/fotg.h,
// STREAM-ORDERED MEMORY); the first returns at once.
#ifndef FOTG_TEMPORAL_HEADER
#define FOTG_TEMPORAL_HEADER
#include "../fotg.h"

namespace OFC {

enum { TEMPORAL_MAX_NEIGHBORS = 8 };
// stats: per output image four doubles
enum TemporalStat { TEMPORAL_SUM_USED = 0, TEMPORAL_UNFILTERED = 1, TEMPORAL_SUM_ABS_FILTERED = 2, TEMPORAL_SUM_ABS_CENTER = 3 };

// frames: T x height x width x channels float32 or 8-bit, channels 1 or 3; center: n frame indices; neighbors: n x K frame indices
// (-1 = absent), 1 <= K <= 8; flows: n x K x height x width x 2 float32, centre -> neighbour.  dst: n images of the frames' layout.
// used (n x height x width uint8), stats (n x 4 double), masks (n x K x height x width uint8, masks of FbCheck), gains (K floats
// >= 0; NULL = all 1) and ref (n clean images, for the residual sums) may be NULL.
inline int TemporalFilter(const float *frames, int T, int width, int height, int channels, const int *center, const int *neighbors,
                          int n, int K, const float *flows, float *dst, unsigned char *used = nullptr, double *stats = nullptr,
                          float tau = 30.f, const float *gains = nullptr, const unsigned char *masks = nullptr,
                          const float *ref = nullptr, int device = 0, void *stream = nullptr)
{
  return fotg_temporal_filter(device, n, K, T, frames, width, height, channels, center, neighbors, flows, masks, tau, gains, ref,
                              dst, used, stats, stream);
}
inline int TemporalFilter(const unsigned char *frames, int T, int width, int height, int channels, const int *center,
                          const int *neighbors, int n, int K, const float *flows, unsigned char *dst, unsigned char *used = nullptr,
                          double *stats = nullptr, float tau = 30.f, const float *gains = nullptr,
                          const unsigned char *masks = nullptr, const unsigned char *ref = nullptr, int device = 0,
                          void *stream = nullptr)
{
  return fotg_temporal_filter_u8(device, n, K, T, frames, width, height, channels, center, neighbors, flows, masks, tau, gains, ref,
                                 dst, used, stats, stream);
}

// the same along a context's coarse flows (n K of fotg_out_size, the outflow of one fotg_calc_batch of the pairs (centre,
// neighbour), image-major), upsampled and cropped on the fly: frames at the original frame size, n K <= max_batch
inline int UpsampleCropTemporalFilter(fotg_ctx *ctx, const float *coarse_flows, const float *frames, int T, int channels,
                                      const int *center, const int *neighbors, int n, int K, float *dst,
                                      unsigned char *used = nullptr, double *stats = nullptr, float tau = 30.f,
                                      const float *gains = nullptr, const unsigned char *masks = nullptr, const float *ref = nullptr,
                                      void *stream = nullptr)
{
  return fotg_upsample_crop_temporal_filter(ctx, n, K, T, coarse_flows, frames, channels, center, neighbors, masks, tau, gains, ref,
                                            dst, used, stats, stream);
}
inline int UpsampleCropTemporalFilter(fotg_ctx *ctx, const float *coarse_flows, const unsigned char *frames, int T, int channels,
                                      const int *center, const int *neighbors, int n, int K, unsigned char *dst,
                                      unsigned char *used = nullptr, double *stats = nullptr, float tau = 30.f,
                                      const float *gains = nullptr, const unsigned char *masks = nullptr,
                                      const unsigned char *ref = nullptr, void *stream = nullptr)
{
  return fotg_upsample_crop_temporal_filter_u8(ctx, n, K, T, coarse_flows, frames, channels, center, neighbors, masks, tau, gains,
                                               ref, dst, used, stats, stream);
}

}  // namespace OFC
#endif
