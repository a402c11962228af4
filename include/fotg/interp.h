// include/fotg/interp.h -- the frame at time t between two frames over the C-ABI of libfotg.so (fotg_interp /
// fotg_upsample_crop_interp and their 8-bit forms): forward projection of the bidirectional flow to t with collisions resolved by
// photo-consistency, holes filled from the other direction, both frames sampled and blended with occlusion reasoning (Baker et
// al., "A Database and Evaluation Methodology for Optical Flow", section 3.3).  Device pointers throughout, asynchronous on
// `stream` (a hipStream_t, 0 = the null stream); each call returns a FOTG_* status.  The definition is in include/fotg.h.
// Stream-ordered memory: a second call on a stream whose earlier call is still pending may wait on the host (include/fotg.h,
// STREAM-ORDERED MEMORY); the first returns at once.
#ifndef FOTG_INTERP_HEADER
#define FOTG_INTERP_HEADER
#include "../fotg.h"

namespace OFC {

// code byte: the origin of the pixel's vector, plus INTERP_ONLY_FRAME0 / INTERP_ONLY_FRAME1 where one frame alone was used
enum InterpCode { INTERP_FROM_FORWARD = 0, INTERP_FROM_BACKWARD = 1, INTERP_HOLE = 2, INTERP_ONLY_FRAME0 = 4, INTERP_ONLY_FRAME1 = 8 };
// stats: per image six doubles
enum InterpStat { INTERP_N_FORWARD = 0, INTERP_N_BACKWARD = 1, INTERP_N_HOLES = 2, INTERP_N_ONE_SIDED = 3, INTERP_SUM_ABS = 4,
                  INTERP_SUM_ABS_BLEND = 5 };

// I0, I1, dst: n x height x width x channels float32 or 8-bit, channels 1 or 3; flow_fw (0 -> 1), flow_bw (1 -> 0): n x height x
// width x 2 float32; 0 < t < 1.  mask_fw / mask_bw (FbCheck's masks; both NULL: the call runs the check itself with alpha1, alpha2),
// ref (the true frame at t, for the residual sums), code (n x height x width uint8) and stats (n x 6 double) may be NULL.
inline int Interpolate(const float *I0, const float *I1, const float *flow_fw, const float *flow_bw, int width, int height, int channels,
                       float t, float *dst, unsigned char *code = nullptr, double *stats = nullptr, const float *ref = nullptr,
                       const unsigned char *mask_fw = nullptr, const unsigned char *mask_bw = nullptr, float alpha1 = 0.01f,
                       float alpha2 = 0.5f, int n = 1, int device = 0, void *stream = nullptr)
{
  return fotg_interp(device, n, I0, I1, flow_fw, flow_bw, width, height, channels, t, mask_fw, mask_bw, alpha1, alpha2, ref, dst, code,
                     stats, stream);
}
inline int Interpolate(const unsigned char *I0, const unsigned char *I1, const float *flow_fw, const float *flow_bw, int width, int height,
                       int channels, float t, unsigned char *dst, unsigned char *code = nullptr, double *stats = nullptr,
                       const unsigned char *ref = nullptr, const unsigned char *mask_fw = nullptr, const unsigned char *mask_bw = nullptr,
                       float alpha1 = 0.01f, float alpha2 = 0.5f, int n = 1, int device = 0, void *stream = nullptr)
{
  return fotg_interp_u8(device, n, I0, I1, flow_fw, flow_bw, width, height, channels, t, mask_fw, mask_bw, alpha1, alpha2, ref, dst,
                        code, stats, stream);
}

// the same from the coarse flows of a bidirectional context (the outflows of fotg_calc_bidir), upsampled and cropped on the fly:
// frames at the original size.  FOTG_ERR_UNSUPPORTED for a context created without fotg_params::bidir.
inline int UpsampleCropInterpolate(fotg_ctx *ctx, const float *coarse_fw, const float *coarse_bw, const float *I0, const float *I1,
                                   int channels, float t, float *dst, unsigned char *code = nullptr, double *stats = nullptr,
                                   const float *ref = nullptr, const unsigned char *mask_fw = nullptr,
                                   const unsigned char *mask_bw = nullptr, float alpha1 = 0.01f, float alpha2 = 0.5f, int n = 1,
                                   void *stream = nullptr)
{
  return fotg_upsample_crop_interp(ctx, n, coarse_fw, coarse_bw, I0, I1, channels, t, mask_fw, mask_bw, alpha1, alpha2, ref, dst, code,
                                   stats, stream);
}
inline int UpsampleCropInterpolate(fotg_ctx *ctx, const float *coarse_fw, const float *coarse_bw, const unsigned char *I0,
                                   const unsigned char *I1, int channels, float t, unsigned char *dst, unsigned char *code = nullptr,
                                   double *stats = nullptr, const unsigned char *ref = nullptr, const unsigned char *mask_fw = nullptr,
                                   const unsigned char *mask_bw = nullptr, float alpha1 = 0.01f, float alpha2 = 0.5f, int n = 1,
                                   void *stream = nullptr)
{
  return fotg_upsample_crop_interp_u8(ctx, n, coarse_fw, coarse_bw, I0, I1, channels, t, mask_fw, mask_bw, alpha1, alpha2, ref, dst,
                                      code, stats, stream);
}

}  // namespace OFC
#endif
