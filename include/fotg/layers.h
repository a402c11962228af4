// include/fotg/layers.h -- motion layers over the C-ABI of libfotg.so (fotg_motion_layers / fotg_upsample_crop_motion_layers): up to
// eight motions of one model (translation, similarity, affine) fitted to one flow, a label per pixel (the layer; 253 unassigned,
// 254 excluded by the mask, 255 unknown), a record per layer.  Device pointers throughout, asynchronous on `stream` (a hipStream_t,
// 0 = the null stream); each call returns a FOTG_* status.  The definition is in include/fotg.h.
// Stream-ordered memory: a second call on a stream whose earlier call is still pending may wait on the host (include/fotg.h,
// STREAM-ORDERED MEMORY); the first returns at once.
#ifndef FOTG_LAYERS_HEADER
#define FOTG_LAYERS_HEADER
#include "motion.h"

namespace OFC {

enum { LAYERS_MAX = 8 };
enum LayerLabel { LAYER_UNASSIGNED = 253, LAYER_MASKED = 254, LAYER_UNKNOWN = 255 };
// records: per layer eight 64-bit integers
enum LayerRecord { LAYER_REC_LABELLED = 0, LAYER_REC_IN_FIT = 1, LAYER_REC_LIVE = 2, LAYER_REC_FITTED = 3, LAYER_REC_SEED = 4,
                   LAYER_REC_SUM_X = 5, LAYER_REC_SUM_Y = 6, LAYER_REC_SUM_U = 7 };
// stats: per image four 64-bit integers
enum LayerStat { LAYER_STAT_UNASSIGNED = 0, LAYER_STAT_MASKED = 1, LAYER_STAT_UNKNOWN = 2, LAYER_STAT_LIVE = 3 };

// flow n x height x width x 2 float32; mask n x height x width uint8 or nullptr (0 = the pixel takes part); params n x layers x 6
// doubles (MotionParam per layer).  init n x layers x 6 doubles (the layers to start from instead of seeding), labels n x height x
// width uint8, residual n x height x width x 2 float32, records n x layers x 8, stats n x 4, sums n x layers x 12: each may be nullptr.
inline int MotionLayers(const float *flow, const unsigned char *mask, int width, int height, int layers, double *params,
                        int model = MOTION_AFFINE, unsigned char *labels = nullptr, float *residual = nullptr, long long *records = nullptr,
                        long long *stats = nullptr, long long *sums = nullptr, const double *init = nullptr, int iters = 3, int rounds = 3,
                        float thresh = 1.0f, int n = 1, int device = 0, void *stream = nullptr)
{
  return fotg_motion_layers(device, n, flow, mask, width, height, layers, model, iters, rounds, thresh, init, params, labels, residual,
                            records, stats, sums, stream);
}

// the same on n coarse flows of a context (the outflow of fotg_calc_batch / fotg_calc_sequence), upsampled and cropped on the fly
inline int UpsampleCropMotionLayers(fotg_ctx *ctx, int n, const float *coarse_flow, const unsigned char *mask, int layers, double *params,
                                    int model = MOTION_AFFINE, unsigned char *labels = nullptr, float *residual = nullptr,
                                    long long *records = nullptr, long long *stats = nullptr, long long *sums = nullptr,
                                    const double *init = nullptr, int iters = 3, int rounds = 3, float thresh = 1.0f, void *stream = nullptr)
{
  return fotg_upsample_crop_motion_layers(ctx, n, coarse_flow, mask, layers, model, iters, rounds, thresh, init, params, labels, residual,
                                          records, stats, sums, stream);
}

}  // namespace OFC
#endif
