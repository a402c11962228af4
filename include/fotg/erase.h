// include/fotg/erase.h -- object removal over the C-ABI of libfotg.so (fotg_erase / fotg_erase_motion / fotg_upsample_crop_erase and
// their 8-bit forms): a mask grown by a disc, feathered at its rim and filled from the plate sampled into the frame's own grid.
// frames, plate, the source of the vectors, plate_code, mask, remove and the outputs are device pointers; index is a HOST array,
// consumed before the call returns.  Asynchronous on `stream` (a hipStream_t, 0 = the null stream); each call returns a FOTG_*
// status.  The definition is in include/fotg.h.
// Stream-ordered memory: a second call on a stream whose earlier call is still pending may wait on the host (include/fotg.h,
// STREAM-ORDERED MEMORY); the first returns at once.
#ifndef FOTG_ERASE_HEADER
#define FOTG_ERASE_HEADER
#include "../fotg.h"

namespace OFC {

enum { ERASE_MAX_DIM = 16384, ERASE_MAX_GROW = 8, ERASE_MAX_FEATHER = 8, ERASE_FULL = 256 };
// code: per frame pixel
enum EraseCode { ERASE_UNTOUCHED = 0, ERASE_REPLACED = 1, ERASE_NO_PLATE = 2, ERASE_UNKNOWN = 3, ERASE_BLENDED = 4 };
// stats: per frame eight 64-bit integers
enum EraseStat { ERASE_N_UNTOUCHED = 0, ERASE_N_REPLACED = 1, ERASE_N_NO_PLATE = 2, ERASE_N_UNKNOWN = 3, ERASE_N_BLENDED = 4,
                 ERASE_N_HOLES = 5, ERASE_N_REMOVE = 6, ERASE_SUM_ALPHA = 7, ERASE_STATS = 8 };

// P plates of W x H x channels on a canvas whose pixel (X, Y) is the reference coordinate (X - ox, Y - oy); code: P x H x W uint8
// (fotg_plate's code, non-zero = nothing known there) or null; index: the plate of every frame (host), null = plate 0 for P == 1,
// plate i for P == n
template <class P_> struct ErasePlate {
  const P_ *plate = nullptr;
  int P = 1, W = 0, H = 0, ox = 0, oy = 0;
  const unsigned char *code = nullptr;
  const int *index = nullptr;
};
// What may be left out: mask (n x height x width uint8, non-zero = the vector is unknown) and the outputs dst (the frames' type and
// shape), code (n x height x width uint8), alpha (int16) and stats (n x 8 long long) -- not all four.  grow: the radius of the
// disc the mask is grown by, feather: the width of the ramp beyond it, both 0 .. 8 pixels.
template <class P_> struct EraseOptions {
  const unsigned char *mask = nullptr;
  int grow = 2, feather = 3;
  P_ *dst = nullptr;
  unsigned char *code = nullptr;
  short *alpha = nullptr;
  long long *stats = nullptr;
};

// frames: n x height x width x channels float32 or 8-bit, channels 1 or 3; remove: n x height x width uint8, non-zero = take this
// pixel out; flows: n x height x width x 2 float32, frame -> reference
inline int RemoveObjects(const float *frames, int n, int width, int height, int channels, const ErasePlate<float> &p,
                         const unsigned char *remove, const float *flows, const EraseOptions<float> &o, int device = 0, void *stream = nullptr)
{
  return fotg_erase(device, n, frames, width, height, channels, p.P, p.plate, p.W, p.H, p.ox, p.oy, p.index, flows, p.code, o.mask, remove,
                    o.grow, o.feather, o.dst, o.code, o.alpha, o.stats, stream);
}
inline int RemoveObjects(const unsigned char *frames, int n, int width, int height, int channels, const ErasePlate<unsigned char> &p,
                         const unsigned char *remove, const float *flows, const EraseOptions<unsigned char> &o, int device = 0,
                         void *stream = nullptr)
{
  return fotg_erase_u8(device, n, frames, width, height, channels, p.P, p.plate, p.W, p.H, p.ox, p.oy, p.index, flows, p.code, o.mask, remove,
                       o.grow, o.feather, o.dst, o.code, o.alpha, o.stats, stream);
}

// the same from camera motions: params n x 6 double, the maps frame -> reference in fit_motion's pixel-frame convention
inline int RemoveObjectsMotion(const float *frames, int n, int width, int height, int channels, const ErasePlate<float> &p,
                               const unsigned char *remove, const double *params, const EraseOptions<float> &o, int device = 0,
                               void *stream = nullptr)
{
  return fotg_erase_motion(device, n, frames, width, height, channels, p.P, p.plate, p.W, p.H, p.ox, p.oy, p.index, params, p.code, o.mask,
                           remove, o.grow, o.feather, o.dst, o.code, o.alpha, o.stats, stream);
}
inline int RemoveObjectsMotion(const unsigned char *frames, int n, int width, int height, int channels, const ErasePlate<unsigned char> &p,
                               const unsigned char *remove, const double *params, const EraseOptions<unsigned char> &o, int device = 0,
                               void *stream = nullptr)
{
  return fotg_erase_motion_u8(device, n, frames, width, height, channels, p.P, p.plate, p.W, p.H, p.ox, p.oy, p.index, params, p.code, o.mask,
                              remove, o.grow, o.feather, o.dst, o.code, o.alpha, o.stats, stream);
}

// the same along a context's coarse flows (n <= max_batch of fotg_out_size, the outflow of one fotg_calc_batch of the pairs
// (frame, reference)), upsampled and cropped on the fly; the frames have the context's original size
inline int UpsampleCropRemoveObjects(fotg_ctx *ctx, const float *coarse_flows, const float *frames, int n, int channels,
                                     const ErasePlate<float> &p, const unsigned char *remove, const EraseOptions<float> &o,
                                     void *stream = nullptr)
{
  return fotg_upsample_crop_erase(ctx, n, coarse_flows, frames, channels, p.P, p.plate, p.W, p.H, p.ox, p.oy, p.index, p.code, o.mask, remove,
                                  o.grow, o.feather, o.dst, o.code, o.alpha, o.stats, stream);
}
inline int UpsampleCropRemoveObjects(fotg_ctx *ctx, const float *coarse_flows, const unsigned char *frames, int n, int channels,
                                     const ErasePlate<unsigned char> &p, const unsigned char *remove, const EraseOptions<unsigned char> &o,
                                     void *stream = nullptr)
{
  return fotg_upsample_crop_erase_u8(ctx, n, coarse_flows, frames, channels, p.P, p.plate, p.W, p.H, p.ox, p.oy, p.index, p.code, o.mask,
                                     remove, o.grow, o.feather, o.dst, o.code, o.alpha, o.stats, stream);
}

// the dilation of remove (n x height x width uint8) by the disc of radius grow as alpha == ERASE_FULL: a pass with alpha as its
// only output, which reads nothing but remove
inline int GrowMaskAlpha(const unsigned char *remove, int n, int width, int height, int grow, short *alpha, int device = 0,
                         void *stream = nullptr)
{
  return fotg_erase(device, n, nullptr, width, height, 1, 1, nullptr, 1, 1, 0, 0, nullptr, nullptr, nullptr, nullptr, remove, grow, 0, nullptr,
                    nullptr, alpha, nullptr, stream);
}

}  // namespace OFC
#endif
