// fotg_objtracks.hip -- C-ABI of the object tracks (include/fotg.h fotg_object_overlap / fotg_upsample_crop_object_overlap /
// fotg_object_links / fotg_object_tracks), kernels in objtracks.hip.h.  Per call: the clearing of the outputs that are accumulated
// into, and one launch.  Everything is enqueued on the caller's stream.
#include "host_call.h"
#include "objtracks.hip.h"

using namespace fotg;

namespace {

bool aligned(const void *p, size_t a) { return (reinterpret_cast<size_t>(p) & (a - 1)) == 0; }

// flow_mem: the flow's memory, flow_bytes long; dense: the kernel reads it with 16-byte loads
template <class Src>
int overlap_batch(int device, int n, const Src &flow, const void *flow_mem, size_t flow_bytes, bool dense, const int *ids_a,
                  const int *ids_b, int w, int h, const unsigned char *mask, int ka, int kb, int *votes, long long *sent, void *stream_)
{
  if (n < 1 || n > 65535 || w < 1 || h < 1 || w > OT_MAX_DIM || h > OT_MAX_DIM) return FOTG_ERR_ARG;
  if (ka < 1 || ka > OT_MAX_K || kb < 1 || kb > OT_MAX_K) return FOTG_ERR_ARG;
  if (!flow_mem || !ids_a || !ids_b || !votes || !sent) return FOTG_ERR_ARG;
  const size_t px = (size_t)n * w * h;
  const Span out[2] = {{votes, (size_t)n * ka * kb * sizeof(int)}, {sent, (size_t)n * ka * OT_NSENT * sizeof(long long)}};
  const Span in[4] = {{ids_a, px * sizeof(int)}, {ids_b, px * sizeof(int)}, {flow_mem, flow_bytes}, {mask, px}};
  if (overlap_any(out, in) || overlap_among(out)) return FOTG_ERR_ARG;
  DevGuard guard(device);
  if (!guard.ok) return hip_fail(guard.err);
  hipStream_t stream = (hipStream_t)stream_;
  hipError_t e = hipMemsetAsync(votes, 0, out[0].bytes, stream);
  if (e == hipSuccess) e = hipMemsetAsync(sent, 0, out[1].bytes, stream);
  if (e == hipSuccess) {
    const int vec = aligned(ids_a, 16) && (!dense || aligned(flow_mem, 16)) && (!mask || aligned(mask, 4));
    const dim3 grid((unsigned)((w + 3 + OT_STRIP - 1) / OT_STRIP), (unsigned)((h + OT_WAVES * OT_ROWS - 1) / (OT_WAVES * OT_ROWS)), (unsigned)n);
    objvote_kernel<Src><<<grid, OT_THREADS, 0, stream>>>(flow, ids_a, ids_b, mask, w, h, ka, kb, vec, votes, sent);
    e = hipGetLastError();
  }
  return e == hipSuccess ? FOTG_OK : hip_fail(e);
}

}  // namespace

extern "C" {

int fotg_object_overlap(int device, int n, const int *ids_a, const int *ids_b, int w, int h, const float *flow,
                        const unsigned char *mask, int ka, int kb, int *votes, long long *sent, void *stream)
{
  const size_t fbytes = (n > 0 && w > 0 && h > 0) ? (size_t)n * w * h * 2 * sizeof(float) : 0;
  return overlap_batch(device, n, DenseSrc{flow}, flow, fbytes, true, ids_a, ids_b, w, h, mask, ka, kb, votes, sent, stream);
}

int fotg_upsample_crop_object_overlap(fotg_ctx *ctx, int n, const float *coarse_flow, const int *ids_a, const int *ids_b,
                                      const unsigned char *mask, int ka, int kb, int *votes, long long *sent, void *stream)
{
  CtxUpsampleGeom g;
  if (!fused_geom(ctx, n, coarse_flow, &g)) return FOTG_ERR_ARG;
  return overlap_batch(g.device, n, upsample_src(g, coarse_flow), coarse_flow, (size_t)n * g.wl * g.hl * 2 * sizeof(float), false,
                       ids_a, ids_b, g.w_org, g.h_org, mask, ka, kb, votes, sent, stream);
}

int fotg_object_links(int device, int n, const int *votes, const long long *objects_a, const long long *objects_b, int ka, int kb,
                      int min_votes, int min_frac256, int *link_ab, int *link_ba, void *stream_)
{
  if (n < 1 || n > 65535 || ka < 1 || ka > OT_MAX_K || kb < 1 || kb > OT_MAX_K) return FOTG_ERR_ARG;
  if (min_votes < 1 || min_frac256 < 0 || min_frac256 > 256) return FOTG_ERR_ARG;
  if (!votes || !objects_a || !objects_b || !link_ab || !link_ba) return FOTG_ERR_ARG;
  const Span out[2] = {{link_ab, (size_t)n * ka * OT_NLINK * sizeof(int)}, {link_ba, (size_t)n * kb * OT_NLINK * sizeof(int)}};
  const Span in[3] = {{votes, (size_t)n * ka * kb * sizeof(int)}, {objects_a, (size_t)n * ka * OT_NREC * sizeof(long long)},
                      {objects_b, (size_t)n * kb * OT_NREC * sizeof(long long)}};
  if (overlap_any(out, in) || overlap_among(out)) return FOTG_ERR_ARG;
  DevGuard guard(device);
  if (!guard.ok) return hip_fail(guard.err);
  objlink_kernel<<<dim3((unsigned)n), OT_THREADS, 0, (hipStream_t)stream_>>>(votes, objects_a, objects_b, ka, kb, min_votes, min_frac256,
                                                                             link_ab, link_ba);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? FOTG_OK : hip_fail(e);
}

int fotg_object_tracks(int device, int T, int K, const long long *objects, const int *link_ab, const int *link_ba, int max_tracks,
                       int *track, long long *tracks, long long *stats, void *stream_)
{
  if (T < 1 || T > 65535 || K < 1 || K > OT_MAX_K || max_tracks < 1 || max_tracks > OT_MAX_TRACKS) return FOTG_ERR_ARG;
  if (!objects || !link_ab || !link_ba || !track || !tracks) return FOTG_ERR_ARG;
  const Span out[3] = {{track, (size_t)(T + 1) * K * sizeof(int)}, {tracks, (size_t)max_tracks * OT_NTRACK * sizeof(long long)},
                       {stats, OT_NSTAT * sizeof(long long)}};
  const Span in[3] = {{objects, (size_t)(T + 1) * K * OT_NREC * sizeof(long long)}, {link_ab, (size_t)T * K * OT_NLINK * sizeof(int)},
                      {link_ba, (size_t)T * K * OT_NLINK * sizeof(int)}};
  if (overlap_any(out, in) || overlap_among(out)) return FOTG_ERR_ARG;
  DevGuard guard(device);
  if (!guard.ok) return hip_fail(guard.err);
  hipStream_t stream = (hipStream_t)stream_;
  hipError_t e = hipMemsetAsync(tracks, 0, out[1].bytes, stream);
  if (e == hipSuccess) {
    objtrack_kernel<<<dim3(1), (unsigned)((K + FOTG_WAVE - 1) / FOTG_WAVE * FOTG_WAVE), 0, stream>>>(objects, link_ab, link_ba, T, K, max_tracks,
                                                                                                      track, tracks, stats);
    e = hipGetLastError();
  }
  return e == hipSuccess ? FOTG_OK : hip_fail(e);
}

}  // extern "C"
