// fotg_histograms.hip -- C-ABI of the motion histograms (include/fotg.h fotg_motion_histograms /
// fotg_upsample_crop_motion_histograms), kernel in histograms.hip.h.  Per call: the clearing of the object rows, which are
// accumulated into, and one launch; the cells are written whole by the launch.  Everything is enqueued on the caller's stream.
#include "host_call.h"
#include "histograms.hip.h"

using namespace fotg;

namespace {

bool aligned(const void *p, size_t a) { return (reinterpret_cast<size_t>(p) & (a - 1)) == 0; }

// flow_mem: the flow's memory, flow_bytes long; dense: the kernel reads it with 16-byte loads
template <class Src>
int histogram_batch(int device, int n, const Src &flow, const void *flow_mem, size_t flow_bytes, bool dense, int w, int h,
                    const unsigned char *mask, const double *params, int cell, int thresh256, long long *cells, const int *ids, int rows,
                    long long *objects, void *stream_)
{
  if (n < 1 || n > 65535 || w < 1 || h < 1 || w > MH_MAX_DIM || h > MH_MAX_DIM || !flow_mem) return FOTG_ERR_ARG;
  if ((cell != 8 && cell != 16 && cell != 32) || thresh256 < 0) return FOTG_ERR_ARG;
  if ((!cells && !objects) || (objects && !ids)) return FOTG_ERR_ARG;
  if (objects && (rows < 1 || rows > MH_MAX_ROWS)) return FOTG_ERR_ARG;
  const size_t px = (size_t)n * w * h, gw = (size_t)(w + cell - 1) / cell, gh = (size_t)(h + cell - 1) / cell;
  const Span out[2] = {{cells, (size_t)n * gh * gw * MH_NREC * sizeof(long long)},
                       {objects, objects ? (size_t)n * rows * MH_NREC * sizeof(long long) : 0}};
  const Span in[4] = {{flow_mem, flow_bytes}, {mask, px}, {params, (size_t)n * 6 * sizeof(double)}, {ids, px * sizeof(int)}};
  if (overlap_any(out, in) || overlap_among(out)) return FOTG_ERR_ARG;
  DevGuard guard(device);
  if (!guard.ok) return hip_fail(guard.err);
  hipStream_t stream = (hipStream_t)stream_;
  hipError_t e = objects ? hipMemsetAsync(objects, 0, out[1].bytes, stream) : hipSuccess;
  if (e == hipSuccess) {
    const int vec = (dense && aligned(flow_mem, 16) ? 1 : 0) | (mask && aligned(mask, 4) ? 2 : 0) | (objects && aligned(ids, 16) ? 4 : 0);
    const dim3 grid((unsigned)((w + MH_TW - 1) / MH_TW), (unsigned)((h + MH_TH - 1) / MH_TH), (unsigned)n);
    mh_kernel<Src><<<grid, MH_THREADS, 0, stream>>>(flow, mask, params, objects ? ids : nullptr, w, h, cell, thresh256, objects ? rows : 1, vec,
                                                    cells, objects);
    e = hipGetLastError();
  }
  return e == hipSuccess ? FOTG_OK : hip_fail(e);
}

}  // namespace

extern "C" {

int fotg_motion_histograms(int device, int n, const float *flow, int w, int h, const unsigned char *mask, const double *params, int cell,
                           int thresh256, long long *cells, const int *ids, int rows, long long *objects, void *stream)
{
  const size_t fbytes = (n > 0 && w > 0 && h > 0) ? (size_t)n * w * h * 2 * sizeof(float) : 0;
  return histogram_batch(device, n, DenseSrc{flow}, flow, fbytes, true, w, h, mask, params, cell, thresh256, cells, ids, rows, objects, stream);
}

int fotg_upsample_crop_motion_histograms(fotg_ctx *ctx, int n, const float *coarse_flow, const unsigned char *mask, const double *params,
                                         int cell, int thresh256, long long *cells, const int *ids, int rows, long long *objects, void *stream)
{
  CtxUpsampleGeom g;
  if (!fused_geom(ctx, n, coarse_flow, &g)) return FOTG_ERR_ARG;
  return histogram_batch(g.device, n, upsample_src(g, coarse_flow), coarse_flow, (size_t)n * g.wl * g.hl * 2 * sizeof(float), false,
                         g.w_org, g.h_org, mask, params, cell, thresh256, cells, ids, rows, objects, stream);
}

}  // extern "C"
