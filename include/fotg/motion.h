// include/fotg/motion.h -- the global-motion fit over the C-ABI of libfotg.so (fotg_fit_motion / fotg_upsample_crop_fit_motion /
// fotg_motion_flow): the one camera motion (translation, similarity, affine) that explains a flow, a code per pixel (0 follows it,
// 1 moves on its own, 2 excluded by the mask, 3 unknown) and the motion as a flow for the warp.  Device pointers throughout,
// asynchronous on `stream` (a hipStream_t, 0 = the null stream); each call returns a FOTG_* status.  The definition is in
// include/fotg.h.
// Stream-ordered memory: a second call on a stream whose earlier call is still pending may wait on the host (include/fotg.h,
// STREAM-ORDERED MEMORY); the first returns at once.
#ifndef FOTG_MOTION_HEADER
#define FOTG_MOTION_HEADER
#include "../fotg.h"

namespace OFC {

enum MotionModel { MOTION_TRANSLATION = 0, MOTION_SIMILARITY = 1, MOTION_AFFINE = 2 };
// params: per image six doubles
enum MotionParam { MOTION_A00 = 0, MOTION_A01 = 1, MOTION_TX = 2, MOTION_A10 = 3, MOTION_A11 = 4, MOTION_TY = 5 };
// stats: per image six 64-bit integers
enum MotionStat { MOTION_FOLLOWS = 0, MOTION_INDEPENDENT = 1, MOTION_MASKED = 2, MOTION_UNKNOWN = 3, MOTION_IN_FIT = 4, MOTION_FITTED = 5 };

// flow n x height x width x 2 float32; mask n x height x width uint8 or nullptr (0 = the pixel takes part); params n x 6 doubles.
// code n x height x width uint8, residual n x height x width x 2 float32, stats n x 6, sums n x 12: each may be nullptr.
inline int FitMotion(const float *flow, const unsigned char *mask, int width, int height, double *params, int model = MOTION_AFFINE,
                     unsigned char *code = nullptr, float *residual = nullptr, long long *stats = nullptr, long long *sums = nullptr,
                     int iters = 3, float thresh = 1.0f, int n = 1, int device = 0, void *stream = nullptr)
{
  return fotg_fit_motion(device, n, flow, mask, width, height, model, iters, thresh, params, code, residual, stats, sums, stream);
}

// the same on n coarse flows of a context (the outflow of fotg_calc_batch / fotg_calc_sequence), upsampled and cropped on the fly
inline int UpsampleCropFitMotion(fotg_ctx *ctx, int n, const float *coarse_flow, const unsigned char *mask, double *params,
                                 int model = MOTION_AFFINE, unsigned char *code = nullptr, float *residual = nullptr,
                                 long long *stats = nullptr, long long *sums = nullptr, int iters = 3, float thresh = 1.0f,
                                 void *stream = nullptr)
{
  return fotg_upsample_crop_fit_motion(ctx, n, coarse_flow, mask, model, iters, thresh, params, code, residual, stats, sums, stream);
}

// params n x 6 doubles -> flow n x height x width x 2 float32: what fotg_warp applies
inline int MotionFlow(const double *params, int width, int height, float *flow, int n = 1, int device = 0, void *stream = nullptr)
{
  return fotg_motion_flow(device, n, params, width, height, flow, stream);
}

}  // namespace OFC
#endif
