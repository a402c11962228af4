// include/fotg/warp.h -- warp an image along a flow over the C-ABI of libfotg.so (fotg_warp / fotg_upsample_crop_warp and their
// 8-bit forms): the reference's image_warp with per-pixel codes (0 valid, 1 occluded, 2 the vector leaves the frame, 3 unknown:
// the alphabet of include/fotg/fbcheck.h) and photometric residuals.  Device pointers throughout, asynchronous on `stream` (a
// hipStream_t, 0 = the null stream); each call returns a FOTG_* status.  The definition is in include/fotg.h.
// Stream-ordered memory: a second call on a stream whose earlier call is still pending may wait on the host (include/fotg.h,
// STREAM-ORDERED MEMORY); the first returns at once.
#ifndef FOTG_WARP_HEADER
#define FOTG_WARP_HEADER
#include "../fotg.h"

namespace OFC {

enum WarpFill { WARP_FILL_REFERENCE = 0, WARP_FILL_INVALID = 1 };
// stats: per image six doubles
enum WarpStat { WARP_VALID = 0, WARP_OCCLUDED = 1, WARP_OUTSIDE = 2, WARP_UNKNOWN = 3, WARP_SUM_ABS_WARPED = 4, WARP_SUM_ABS_UNWARPED = 5 };

// src (the image to pull back: frame 1 for a forward flow), dst: n x height x width x channels float32 or 8-bit, channels 1 or 3;
// flow: n x height x width x 2 float32.  ref (frame 0, for the residual sums), occ (a mask of FbCheck), code (n x height x width
// uint8) and stats (n x 6 double) may be NULL.  fill_mode WARP_FILL_INVALID writes `fill` wherever the code is not 0.
inline int Warp(const float *src, const float *flow, int width, int height, int channels, float *dst, unsigned char *code = nullptr,
                double *stats = nullptr, const float *ref = nullptr, const unsigned char *occ = nullptr,
                int fill_mode = WARP_FILL_REFERENCE, float fill = 0.f, int n = 1, int device = 0, void *stream = nullptr)
{
  return fotg_warp(device, n, src, flow, width, height, channels, ref, occ, fill_mode, fill, dst, code, stats, stream);
}
inline int Warp(const unsigned char *src, const float *flow, int width, int height, int channels, unsigned char *dst,
                unsigned char *code = nullptr, double *stats = nullptr, const unsigned char *ref = nullptr,
                const unsigned char *occ = nullptr, int fill_mode = WARP_FILL_REFERENCE, float fill = 0.f, int n = 1, int device = 0,
                void *stream = nullptr)
{
  return fotg_warp_u8(device, n, src, flow, width, height, channels, ref, occ, fill_mode, fill, dst, code, stats, stream);
}

// the same along a context's coarse flow (fotg_out_size), upsampled and cropped on the fly: images at the original frame size
inline int UpsampleCropWarp(fotg_ctx *ctx, const float *coarse_flow, const float *src, int channels, float *dst,
                            unsigned char *code = nullptr, double *stats = nullptr, const float *ref = nullptr,
                            const unsigned char *occ = nullptr, int fill_mode = WARP_FILL_REFERENCE, float fill = 0.f, int n = 1,
                            void *stream = nullptr)
{
  return fotg_upsample_crop_warp(ctx, n, coarse_flow, src, channels, ref, occ, fill_mode, fill, dst, code, stats, stream);
}
inline int UpsampleCropWarp(fotg_ctx *ctx, const float *coarse_flow, const unsigned char *src, int channels, unsigned char *dst,
                            unsigned char *code = nullptr, double *stats = nullptr, const unsigned char *ref = nullptr,
                            const unsigned char *occ = nullptr, int fill_mode = WARP_FILL_REFERENCE, float fill = 0.f, int n = 1,
                            void *stream = nullptr)
{
  return fotg_upsample_crop_warp_u8(ctx, n, coarse_flow, src, channels, ref, occ, fill_mode, fill, dst, code, stats, stream);
}

}  // namespace OFC
#endif
