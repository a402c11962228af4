// include/fotg/blur.h -- motion blur along a flow over the C-ABI of libfotg.so (fotg_motion_blur, fotg_upsample_crop_motion_blur):
// a shutter simulated per frame by the tile-max / neighbour-max reconstruction filter, for float32 and 8-bit frames of 1 or 3
// channels.  Device pointers throughout, asynchronous on `stream` (a hipStream_t, 0 = the null stream); every call returns a
// FOTG_* status.  The definition is in include/fotg.h.
// Stream-ordered memory: a second call on a stream whose earlier call is still pending may wait on the host (include/fotg.h,
// STREAM-ORDERED MEMORY); the first returns at once.
#ifndef FOTG_BLUR_HEADER
#define FOTG_BLUR_HEADER
#include "../fotg.h"

namespace OFC {

// code: per pixel
enum BlurCode { BLUR_UNTOUCHED = 0, BLUR_BLURRED = 1, BLUR_CLAMPED = 2, BLUR_UNKNOWN = 3 };
// stats: per image eight 64-bit integers
enum BlurStat { BLUR_N_UNTOUCHED = 0, BLUR_N_BLURRED = 1, BLUR_N_CLAMPED = 2, BLUR_N_UNKNOWN = 3, BLUR_TAPS = 4, BLUR_COPY_TILES = 5,
                BLUR_MAX_LEN = 6, BLUR_STATS = 8 };
enum { BLUR_TILE = 32, BLUR_MAX = 32, BLUR_SHUTTER_180 = 128 };      // shutter256 = round(256 shutter): 128 = half the frame interval

// src, dst: n x height x width x channels float32 or 8-bit, channels 1 or 3; flow: n x height x width x 2 float32, the flow of src's
// frame.  mask (n x height x width uint8, a mask of FbCheck), code (n x height x width uint8), vectors (n x height x width x 2 int16,
// the half-vectors in 1/16 pixel) and stats (n x 8 int64) may be NULL.
inline int MotionBlur(const float *src, const float *flow, int width, int height, int channels, float *dst, int shutter256 = BLUR_SHUTTER_180,
                      int max_blur = BLUR_MAX, const unsigned char *mask = nullptr, unsigned char *code = nullptr, short *vectors = nullptr,
                      long long *stats = nullptr, int n = 1, int device = 0, void *stream = nullptr)
{
  return fotg_motion_blur(device, n, src, FOTG_BLUR_F32, channels, flow, width, height, mask, shutter256, max_blur, dst, code, vectors, stats,
                          stream);
}
inline int MotionBlur(const unsigned char *src, const float *flow, int width, int height, int channels, unsigned char *dst,
                      int shutter256 = BLUR_SHUTTER_180, int max_blur = BLUR_MAX, const unsigned char *mask = nullptr,
                      unsigned char *code = nullptr, short *vectors = nullptr, long long *stats = nullptr, int n = 1, int device = 0,
                      void *stream = nullptr)
{
  return fotg_motion_blur(device, n, src, FOTG_BLUR_U8, channels, flow, width, height, mask, shutter256, max_blur, dst, code, vectors, stats,
                          stream);
}

// the same along a context's coarse flow (fotg_out_size), upsampled and cropped on the fly: frames at the original frame size
inline int UpsampleCropMotionBlur(fotg_ctx *ctx, const float *coarse_flow, const float *src, int channels, float *dst,
                                  int shutter256 = BLUR_SHUTTER_180, int max_blur = BLUR_MAX, const unsigned char *mask = nullptr,
                                  unsigned char *code = nullptr, short *vectors = nullptr, long long *stats = nullptr, int n = 1,
                                  void *stream = nullptr)
{
  return fotg_upsample_crop_motion_blur(ctx, n, src, FOTG_BLUR_F32, channels, coarse_flow, mask, shutter256, max_blur, dst, code, vectors,
                                        stats, stream);
}
inline int UpsampleCropMotionBlur(fotg_ctx *ctx, const float *coarse_flow, const unsigned char *src, int channels, unsigned char *dst,
                                  int shutter256 = BLUR_SHUTTER_180, int max_blur = BLUR_MAX, const unsigned char *mask = nullptr,
                                  unsigned char *code = nullptr, short *vectors = nullptr, long long *stats = nullptr, int n = 1,
                                  void *stream = nullptr)
{
  return fotg_upsample_crop_motion_blur(ctx, n, src, FOTG_BLUR_U8, channels, coarse_flow, mask, shutter256, max_blur, dst, code, vectors,
                                        stats, stream);
}

}  // namespace OFC
#endif
