// include/fotg/histograms.h -- motion histograms over the C-ABI of libfotg.so (fotg_motion_histograms,
// fotg_upsample_crop_motion_histograms): the histogram of optical flow (HOF) and the motion-boundary histograms (MBHx, MBHy) of a
// flow, per cell of a regular grid and/or per object of the ids of LabelComponents (fotg/objects.h), with the camera motion of
// FitMotion (fotg/motion.h) subtracted first.  Device pointers throughout, asynchronous on `stream` (a hipStream_t, 0 = the null
// stream); every call returns a FOTG_* status.  The definition is in include/fotg.h.
#ifndef FOTG_HISTOGRAMS_HEADER
#define FOTG_HISTOGRAMS_HEADER
#include "../fotg.h"

namespace OFC {

// a record: 32 64-bit integers
enum HistField { HIST_HOF = 0, HIST_ZERO = 8, HIST_MBHX = 9, HIST_MBHY = 17, HIST_N = 25, HIST_N_MBH = 26, HIST_N_BAD = 27, HIST_SUM_M = 28,
                 HIST_SUM_U = 29, HIST_SUM_V = 30, HIST_FIELDS = 32 };
enum { HIST_BINS = 8, HIST_THRESH256 = 102 };       // 102 = rint(0.4 x 256): vectors shorter than 0.4 pixel count in the zero bin

inline int HistCells(int size, int cell) { return (size + cell - 1) / cell; }

// flow n x height x width x 2 float32; cells n x HistCells(height, cell) x HistCells(width, cell) x 32 or nullptr; ids n x height x width
// int32 with objects n x rows x 32, or both nullptr; mask n x height x width uint8 or nullptr; params n x 6 doubles or nullptr.
inline int MotionHistograms(const float *flow, int width, int height, long long *cells, int cell = 16, const int *ids = nullptr,
                            long long *objects = nullptr, int rows = 256, const unsigned char *mask = nullptr, const double *params = nullptr,
                            int thresh256 = HIST_THRESH256, int n = 1, int device = 0, void *stream = nullptr)
{
  return fotg_motion_histograms(device, n, flow, width, height, mask, params, cell, thresh256, cells, ids, rows, objects, stream);
}

// the same along the coarse flow of a context, upsampled and cropped on the fly
inline int MotionHistograms(fotg_ctx *ctx, const float *coarse_flow, long long *cells, int cell = 16, const int *ids = nullptr,
                            long long *objects = nullptr, int rows = 256, const unsigned char *mask = nullptr, const double *params = nullptr,
                            int thresh256 = HIST_THRESH256, int n = 1, void *stream = nullptr)
{
  return fotg_upsample_crop_motion_histograms(ctx, n, coarse_flow, mask, params, cell, thresh256, cells, ids, rows, objects, stream);
}

}  // namespace OFC
#endif
