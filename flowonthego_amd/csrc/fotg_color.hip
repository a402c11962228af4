// fotg_color.hip -- C-ABI of the Middlebury flow colour code (include/fotg.h fotg_flow_color / fotg_upsample_crop_color), kernels in
// flowcolor.hip.h.  Per batch: zero the per-image keys, range pass, colour pass, and (when the caller asked for them) the keys
// turned into the printed statistics in place.  Asynchronous on the caller's stream; no host synchronisation.
#include "host_call.h"
#include "flowcolor.hip.h"

using namespace fotg;

namespace {

// range + colour launches over a batch of n images of w x h pixels, whatever Src reads them from
template <class Src>
int color_batch(int device, int n, const Src &src, int w, int h, float maxmotion, unsigned char *rgb, float *stats, void *stream_)
{
  const long hw = (long)w * h, npix = hw * n;
  const long color_blocks = ((npix + 3) / 4 + 255) / 256;
  if (color_blocks > 0x7fffffffL) return FOTG_ERR_ARG;
  DevGuard guard(device);
  if (!guard.ok) return hip_fail(hipGetLastError());
  hipStream_t stream = (hipStream_t)stream_;
  // per-image keys: the caller's stats buffer (decoded in place at the end), or stream-ordered memory of our own
  unsigned *keys = reinterpret_cast<unsigned *>(stats);
  Scratch mem(stream);
  if (!keys && !mem.get(&keys, (size_t)n * FC_NSTAT * sizeof(unsigned))) return mem.finish(mem.err);
  hipError_t e = hipMemsetAsync(keys, 0, (size_t)n * FC_NSTAT * sizeof(unsigned), stream);
  if (e == hipSuccess) {
    // range pass: at least 4 pixels per thread, about 4096 workgroups for the batch (16 per CU)
    const long need = (hw + 1023) / 1024, cap = 4096 / n > 8 ? 4096 / n : 8;
    const int per_img = (int)(need < cap ? need : cap);
    flow_range_kernel<Src><<<dim3((unsigned)((long)per_img * n)), 256, 0, stream>>>(src, w, h, per_img, keys);
    flow_color_kernel<Src><<<dim3((unsigned)color_blocks), 256, 0, stream>>>(src, w, h, npix, keys, maxmotion, rgb);
    if (stats) flow_stats_kernel<<<dim3((unsigned)((n + 255) / 256)), 256, 0, stream>>>(n, keys);
    e = hipGetLastError();
  }
  return mem.finish(e);
}

}  // namespace

extern "C" {

int fotg_flow_color(int device, int n, const float *flow, int w, int h, float maxmotion, unsigned char *rgb, float *stats, void *stream)
{
  if (n < 1 || !flow || !rgb || w <= 0 || h <= 0) return FOTG_ERR_ARG;
  return color_batch(device, n, DenseSrc{flow}, w, h, maxmotion, rgb, stats, stream);
}

int fotg_upsample_crop_color(fotg_ctx *ctx, int n, const float *flow, float maxmotion, unsigned char *rgb, float *stats, void *stream)
{
  CtxUpsampleGeom g;
  if (!rgb || !fused_geom(ctx, n, flow, &g)) return FOTG_ERR_ARG;
  return color_batch(g.device, n, upsample_src(g, flow), g.w_org, g.h_org, maxmotion, rgb, stats, stream);
}

}  // extern "C"
