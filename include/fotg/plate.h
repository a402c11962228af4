// include/fotg/plate.h -- background plates and mosaics over the C-ABI of libfotg.so (fotg_plate / fotg_plate_motion /
// fotg_upsample_crop_plate and their 8-bit forms): the frames of a shot pulled into one coordinate system along their motion and
// reduced per pixel by a median (or a mean) over the frames that see the pixel.  frames, the source of the vectors, occ, exclude,
// ref and the outputs are device pointers; index is a HOST array, consumed before the call returns.  Asynchronous on `stream` (a
// hipStream_t, 0 = the null stream); each call returns a FOTG_* status.  The definition is in include/fotg.h.
// Stream-ordered memory: a second call on a stream whose earlier call is still pending may wait on the host (include/fotg.h,
// STREAM-ORDERED MEMORY); the first returns at once.
#ifndef FOTG_PLATE_HEADER
#define FOTG_PLATE_HEADER
#include "../fotg.h"

namespace OFC {

enum { PLATE_MAX_FRAMES = 32, PLATE_MAX_DIM = 16384 };
enum PlateMode { PLATE_MEDIAN = 0, PLATE_MEAN = 1 };
// code: per canvas pixel
enum PlateCode { PLATE_ESTIMATED = 0, PLATE_HIDDEN = 1, PLATE_UNCOVERED = 2 };
// stats: per plate six doubles
enum PlateStat { PLATE_N_ESTIMATED = 0, PLATE_N_HIDDEN = 1, PLATE_N_UNCOVERED = 2, PLATE_SUM_COUNT = 3, PLATE_SUM_ABS_PLATE = 4,
                 PLATE_SUM_ABS_FIRST = 5, PLATE_STATS = 6 };

// The canvas of n plates: W x H pixels, pixel (X, Y) the reference coordinate (X - ox, Y - oy).
struct PlateCanvas { int W, H, ox, oy; };
// What may be left out: occ (n x K x H x W uint8), exclude (T x height x width uint8), ref (n x H x W x channels) and the outputs
// count, code (n x H x W uint8) and stats (n x 6 double).
template <class P> struct PlateOptions {
  const unsigned char *occ = nullptr, *exclude = nullptr;
  const P *ref = nullptr;
  unsigned char *count = nullptr, *code = nullptr;
  double *stats = nullptr;
  int mode = PLATE_MEDIAN, min_count = 1;
  float fill = 0.f;
};

// frames: T x height x width x channels float32 or 8-bit, channels 1 or 3; index: n x K frame indices (-1 = absent), 1 <= K <= 32;
// flows: n x K x H x W x 2 float32 on the canvas, reference -> frame.  dst: n x H x W x channels of the frames' type.
inline int BackgroundPlate(const float *frames, int T, int width, int height, int channels, const int *index, int n, int K,
                           const float *flows, const PlateCanvas &c, float *dst, const PlateOptions<float> &o = PlateOptions<float>(),
                           int device = 0, void *stream = nullptr)
{
  return fotg_plate(device, n, K, T, frames, width, height, channels, index, flows, c.W, c.H, c.ox, c.oy, o.occ, o.exclude, o.mode,
                    o.min_count, o.fill, o.ref, dst, o.count, o.code, o.stats, stream);
}
inline int BackgroundPlate(const unsigned char *frames, int T, int width, int height, int channels, const int *index, int n, int K,
                           const float *flows, const PlateCanvas &c, unsigned char *dst,
                           const PlateOptions<unsigned char> &o = PlateOptions<unsigned char>(), int device = 0, void *stream = nullptr)
{
  return fotg_plate_u8(device, n, K, T, frames, width, height, channels, index, flows, c.W, c.H, c.ox, c.oy, o.occ, o.exclude, o.mode,
                       o.min_count, o.fill, o.ref, dst, o.count, o.code, o.stats, stream);
}

// the same from camera motions: params n x K x 6 double, the maps reference -> frame in fit_motion's pixel-frame convention
inline int BackgroundPlateMotion(const float *frames, int T, int width, int height, int channels, const int *index, int n, int K,
                                 const double *params, const PlateCanvas &c, float *dst,
                                 const PlateOptions<float> &o = PlateOptions<float>(), int device = 0, void *stream = nullptr)
{
  return fotg_plate_motion(device, n, K, T, frames, width, height, channels, index, params, c.W, c.H, c.ox, c.oy, o.occ, o.exclude, o.mode,
                           o.min_count, o.fill, o.ref, dst, o.count, o.code, o.stats, stream);
}
inline int BackgroundPlateMotion(const unsigned char *frames, int T, int width, int height, int channels, const int *index, int n, int K,
                                 const double *params, const PlateCanvas &c, unsigned char *dst,
                                 const PlateOptions<unsigned char> &o = PlateOptions<unsigned char>(), int device = 0,
                                 void *stream = nullptr)
{
  return fotg_plate_motion_u8(device, n, K, T, frames, width, height, channels, index, params, c.W, c.H, c.ox, c.oy, o.occ, o.exclude,
                              o.mode, o.min_count, o.fill, o.ref, dst, o.count, o.code, o.stats, stream);
}

// the same along a context's coarse flows (n K of fotg_out_size, the outflow of one fotg_calc_batch of the pairs (reference, frame),
// plate-major), upsampled and cropped on the fly: the canvas is the frame grid, n K <= max_batch
inline int UpsampleCropBackgroundPlate(fotg_ctx *ctx, const float *coarse_flows, const float *frames, int T, int channels,
                                       const int *index, int n, int K, float *dst, const PlateOptions<float> &o = PlateOptions<float>(),
                                       void *stream = nullptr)
{
  return fotg_upsample_crop_plate(ctx, n, K, T, coarse_flows, frames, channels, index, o.occ, o.exclude, o.mode, o.min_count, o.fill, o.ref,
                                  dst, o.count, o.code, o.stats, stream);
}
inline int UpsampleCropBackgroundPlate(fotg_ctx *ctx, const float *coarse_flows, const unsigned char *frames, int T, int channels,
                                       const int *index, int n, int K, unsigned char *dst,
                                       const PlateOptions<unsigned char> &o = PlateOptions<unsigned char>(), void *stream = nullptr)
{
  return fotg_upsample_crop_plate_u8(ctx, n, K, T, coarse_flows, frames, channels, index, o.occ, o.exclude, o.mode, o.min_count, o.fill,
                                     o.ref, dst, o.count, o.code, o.stats, stream);
}

}  // namespace OFC
#endif
