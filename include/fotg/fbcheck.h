// include/fotg/fbcheck.h -- forward-backward consistency check over the C-ABI of libfotg.so (fotg_fb_check /
// fotg_upsample_crop_fb_check): per pixel 0 consistent, 1 occluded or inconsistent, 2 the vector leaves the frame, 3 unknown.
// Device pointers throughout, asynchronous on `stream` (a hipStream_t, 0 = the null stream); each call returns a FOTG_* status.
#ifndef FOTG_FBCHECK_HEADER
#define FOTG_FBCHECK_HEADER
#include "../fotg.h"

namespace OFC {

enum FbCode { FB_CONSISTENT = 0, FB_OCCLUDED = 1, FB_OUTSIDE = 2, FB_UNKNOWN = 3 };

// flow (frame 0 -> 1), flow_bw (frame 1 -> 0): n x height x width x 2 float32.  mask (frame 0) / mask_bw (frame 1): n x height x
// width uint8, either may be NULL.  counts: NULL or n x 2 x 4 uint32, per image and direction the pixels of each code.
inline int FbCheck(const float *flow, const float *flow_bw, int width, int height, unsigned char *mask, unsigned char *mask_bw = nullptr,
                   unsigned *counts = nullptr, float alpha1 = 0.01f, float alpha2 = 0.5f, int n = 1, int device = 0, void *stream = nullptr)
{
  return fotg_fb_check(device, n, flow, flow_bw, width, height, alpha1, alpha2, mask, mask_bw, counts, stream);
}

// the same from a context's coarse flows (fotg_out_size each), upsampled and cropped on the fly: masks at the original frame size
inline int UpsampleCropFbCheck(fotg_ctx *ctx, const float *flow, const float *flow_bw, unsigned char *mask, unsigned char *mask_bw = nullptr,
                               unsigned *counts = nullptr, float alpha1 = 0.01f, float alpha2 = 0.5f, int n = 1, void *stream = nullptr)
{
  return fotg_upsample_crop_fb_check(ctx, n, flow, flow_bw, alpha1, alpha2, mask, mask_bw, counts, stream);
}

}  // namespace OFC
#endif
