// fotg_fbcheck.hip -- C-ABI of the forward-backward consistency check (include/fotg.h fotg_fb_check /
// fotg_upsample_crop_fb_check), kernel in fbcheck.hip.h.  Per call: zero the counts (when asked for), one launch for both
// directions of every pair.  Asynchronous on the caller's stream; no host synchronisation.
#include "host_call.h"
#include "fbcheck.hip.h"

using namespace fotg;

namespace {

template <class Src>
int fb_batch(int device, int n, const Src &fw, const Src &bw, int w, int h, float alpha1, float alpha2, unsigned char *mask,
             unsigned char *mask_bw, unsigned *counts, void *stream_)
{
  const long hw = (long)w * h;
  const long blocks = ((hw + 3) / 4 + 255) / 256;
  if (blocks > 0x7fffffffL || n > 65535) return FOTG_ERR_ARG;
  if (!mask && !mask_bw && !counts) return FOTG_OK;
  DevGuard guard(device);
  if (!guard.ok) return hip_fail(guard.err);
  hipStream_t stream = (hipStream_t)stream_;
  if (counts) {
    const hipError_t e = hipMemsetAsync(counts, 0, (size_t)n * 2 * FB_NCODE * sizeof(unsigned), stream);
    if (e != hipSuccess) return hip_fail(e);
  }
  fb_check_kernel<Src><<<dim3((unsigned)blocks, (unsigned)n, 2), 256, 0, stream>>>(fw, bw, w, h, alpha1, alpha2, mask, mask_bw, counts);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? FOTG_OK : hip_fail(e);
}

}  // namespace

extern "C" {

int fotg_fb_check(int device, int n, const float *flow, const float *flow_bw, int w, int h, float alpha1, float alpha2,
                  unsigned char *mask, unsigned char *mask_bw, unsigned *counts, void *stream)
{
  if (n < 1 || !flow || !flow_bw || w <= 0 || h <= 0) return FOTG_ERR_ARG;
  return fb_batch(device, n, DenseSrc{flow}, DenseSrc{flow_bw}, w, h, alpha1, alpha2, mask, mask_bw, counts, stream);
}

int fotg_upsample_crop_fb_check(fotg_ctx *ctx, int n, const float *flow, const float *flow_bw, float alpha1, float alpha2,
                                unsigned char *mask, unsigned char *mask_bw, unsigned *counts, void *stream)
{
  CtxUpsampleGeom g;
  if (!flow_bw || !fused_geom(ctx, n, flow, &g)) return FOTG_ERR_ARG;
  return fb_batch(g.device, n, upsample_src(g, flow), upsample_src(g, flow_bw), g.w_org, g.h_org, alpha1, alpha2, mask, mask_bw, counts,
                  stream);
}

}  // extern "C"
