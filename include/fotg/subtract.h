// include/fotg/subtract.h -- background subtraction against a plate over the C-ABI of libfotg.so (fotg_subtract /
// fotg_subtract_motion / fotg_upsample_crop_subtract and their 8-bit forms): every frame compared with the plate sampled into the
// frame's own grid, the difference averaged over a small window and classified by a low and a high threshold.  frames, plate, the
// source of the vectors, plate_code, mask and the outputs are device pointers; index is a HOST array, consumed before the call
// returns.  Asynchronous on `stream` (a hipStream_t, 0 = the null stream); each call returns a FOTG_* status.  The definition is
// in include/fotg.h.
// Stream-ordered memory: a second call on a stream whose earlier call is still pending may wait on the host (include/fotg.h,
// STREAM-ORDERED MEMORY); the first returns at once.
#ifndef FOTG_SUBTRACT_HEADER
#define FOTG_SUBTRACT_HEADER
#include "../fotg.h"

namespace OFC {

enum { SUBTRACT_MAX_DIM = 16384, SUBTRACT_MAX_WINDOW = 2 };
// code: per frame pixel; fotg_label_components with the foreground set SUBTRACT_FG_SET takes the map as it is
enum SubtractCode { SUBTRACT_BACKGROUND = 0, SUBTRACT_FOREGROUND = 1, SUBTRACT_NO_PLATE = 2, SUBTRACT_UNKNOWN = 3, SUBTRACT_STRONG = 4 };
enum { SUBTRACT_FG_SET = (1 << SUBTRACT_FOREGROUND) | (1 << SUBTRACT_STRONG) };
// stats: per frame seven 64-bit integers
enum SubtractStat { SUBTRACT_N_BACKGROUND = 0, SUBTRACT_N_FOREGROUND = 1, SUBTRACT_N_NO_PLATE = 2, SUBTRACT_N_UNKNOWN = 3,
                    SUBTRACT_N_STRONG = 4, SUBTRACT_SUM_DIFF = 5, SUBTRACT_SUM_DIFF_FOREGROUND = 6, SUBTRACT_STATS = 7 };

// P plates of W x H x channels on a canvas whose pixel (X, Y) is the reference coordinate (X - ox, Y - oy); code: P x H x W uint8
// (fotg_plate's code, non-zero = nothing known there) or null; index: the plate of every frame (host), null = plate 0 for P == 1,
// plate i for P == n
template <class P_> struct SubtractPlate {
  const P_ *plate = nullptr;
  int P = 1, W = 0, H = 0, ox = 0, oy = 0;
  const unsigned char *code = nullptr;
  const int *index = nullptr;
};
// What may be left out: mask (n x height x width uint8, non-zero = the vector is unknown) and the outputs code (n x height x width
// uint8), diff (int16), evidence (n x height x width x 2 float) and stats (n x 7 long long) -- not all four.  low, high: the
// thresholds in grey levels; window: 0, 1 or 2.
struct SubtractOptions {
  const unsigned char *mask = nullptr;
  float low = 8.f, high = 24.f;
  int window = 1;
  unsigned char *code = nullptr;
  short *diff = nullptr;
  float *evidence = nullptr;
  long long *stats = nullptr;
};

// frames: n x height x width x channels float32 or 8-bit, channels 1 or 3; flows: n x height x width x 2 float32, frame -> reference
inline int SubtractBackground(const float *frames, int n, int width, int height, int channels, const SubtractPlate<float> &p,
                              const float *flows, const SubtractOptions &o, int device = 0, void *stream = nullptr)
{
  return fotg_subtract(device, n, frames, width, height, channels, p.P, p.plate, p.W, p.H, p.ox, p.oy, p.index, flows, p.code, o.mask, o.low,
                       o.high, o.window, o.code, o.diff, o.evidence, o.stats, stream);
}
inline int SubtractBackground(const unsigned char *frames, int n, int width, int height, int channels,
                              const SubtractPlate<unsigned char> &p, const float *flows, const SubtractOptions &o, int device = 0,
                              void *stream = nullptr)
{
  return fotg_subtract_u8(device, n, frames, width, height, channels, p.P, p.plate, p.W, p.H, p.ox, p.oy, p.index, flows, p.code, o.mask,
                          o.low, o.high, o.window, o.code, o.diff, o.evidence, o.stats, stream);
}

// the same from camera motions: params n x 6 double, the maps frame -> reference in fit_motion's pixel-frame convention
inline int SubtractBackgroundMotion(const float *frames, int n, int width, int height, int channels, const SubtractPlate<float> &p,
                                    const double *params, const SubtractOptions &o, int device = 0, void *stream = nullptr)
{
  return fotg_subtract_motion(device, n, frames, width, height, channels, p.P, p.plate, p.W, p.H, p.ox, p.oy, p.index, params, p.code,
                              o.mask, o.low, o.high, o.window, o.code, o.diff, o.evidence, o.stats, stream);
}
inline int SubtractBackgroundMotion(const unsigned char *frames, int n, int width, int height, int channels,
                                    const SubtractPlate<unsigned char> &p, const double *params, const SubtractOptions &o, int device = 0,
                                    void *stream = nullptr)
{
  return fotg_subtract_motion_u8(device, n, frames, width, height, channels, p.P, p.plate, p.W, p.H, p.ox, p.oy, p.index, params, p.code,
                                 o.mask, o.low, o.high, o.window, o.code, o.diff, o.evidence, o.stats, stream);
}

// the same along a context's coarse flows (n <= max_batch of fotg_out_size, the outflow of one fotg_calc_batch of the pairs
// (frame, reference)), upsampled and cropped on the fly; the frames have the context's original size
inline int UpsampleCropSubtractBackground(fotg_ctx *ctx, const float *coarse_flows, const float *frames, int n, int channels,
                                          const SubtractPlate<float> &p, const SubtractOptions &o, void *stream = nullptr)
{
  return fotg_upsample_crop_subtract(ctx, n, coarse_flows, frames, channels, p.P, p.plate, p.W, p.H, p.ox, p.oy, p.index, p.code, o.mask,
                                     o.low, o.high, o.window, o.code, o.diff, o.evidence, o.stats, stream);
}
inline int UpsampleCropSubtractBackground(fotg_ctx *ctx, const float *coarse_flows, const unsigned char *frames, int n, int channels,
                                          const SubtractPlate<unsigned char> &p, const SubtractOptions &o, void *stream = nullptr)
{
  return fotg_upsample_crop_subtract_u8(ctx, n, coarse_flows, frames, channels, p.P, p.plate, p.W, p.H, p.ox, p.oy, p.index, p.code, o.mask,
                                        o.low, o.high, o.window, o.code, o.diff, o.evidence, o.stats, stream);
}

}  // namespace OFC
#endif
