// fotg_chain.hip -- C-ABI of flow chaining (include/fotg.h fotg_flow_chain / fotg_track_points and their fused forms), kernels in
// chain.hip.h.  Per call: zero the statistics (when asked for), one launch that walks all T steps of every chain.  Asynchronous on
// the caller's stream; no host synchronisation.
#include "host_call.h"
#include "chain.hip.h"

using namespace fotg;

namespace {

// the size checks every form shares
bool chain_args_ok(int n_seq, int T, int w, int h)
{
  if (n_seq < 1 || n_seq > 65535 || T < 1 || w < 1 || h < 1) return false;
  if ((long)n_seq * T > 0x7fffffffL) return false;                                      // the plane index s T + k is an int
  // the dense grid's x dimension: w h can reach 2^62, a quarter of it over 256 threads 2^52 workgroups
  return (((long)w * h + 3) / 4 + CHAIN_THREADS - 1) / CHAIN_THREADS <= 0x7fffffffL;
}

template <class Src>
int chain_dense(int device, int n_seq, int T, const Src &fw, const Src &bw, bool has_bw, size_t in_bytes, int w, int h, float alpha1,
                float alpha2, float *total, unsigned char *code, int *steps, unsigned long long *stats, void *stream_)
{
  if (!chain_args_ok(n_seq, T, w, h) || (!total && !code && !steps && !stats)) return FOTG_ERR_ARG;
  const size_t hw = (size_t)w * h, np = (size_t)n_seq * hw;
  const Span out[4] = {{total, np * 8}, {code, np}, {steps, np * 4}, {stats, (size_t)n_seq * CHAIN_NSTAT * 8}};
  const Span in[2] = {{fw.flow, in_bytes}, {has_bw ? bw.flow : nullptr, in_bytes}};
  if (overlap_any(out, in)) return FOTG_ERR_ARG;              // (outputs against inputs only)
  DevGuard guard(device);
  if (!guard.ok) return hip_fail(guard.err);
  hipStream_t stream = (hipStream_t)stream_;
  if (stats) {
    const hipError_t e = hipMemsetAsync(stats, 0, out[3].bytes, stream);
    if (e != hipSuccess) return hip_fail(e);
  }
  const dim3 grid((unsigned)(((hw + 3) / 4 + CHAIN_THREADS - 1) / CHAIN_THREADS), (unsigned)n_seq);
  if (has_bw)
    chain_dense_kernel<Src, true><<<grid, CHAIN_THREADS, 0, stream>>>(fw, bw, T, w, h, alpha1, alpha2, total, code, steps, stats);
  else
    chain_dense_kernel<Src, false><<<grid, CHAIN_THREADS, 0, stream>>>(fw, fw, T, w, h, alpha1, alpha2, total, code, steps, stats);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? FOTG_OK : hip_fail(e);
}

template <class Src>
int chain_points(int device, int n_seq, int T, const Src &fw, const Src &bw, bool has_bw, size_t in_bytes, int w, int h, float alpha1,
                 float alpha2, int P, const float *pts, float *traj, unsigned char *code, int *steps, unsigned long long *stats,
                 void *stream_)
{
  if (!chain_args_ok(n_seq, T, w, h) || P < 1 || !pts || (!traj && !code && !steps && !stats)) return FOTG_ERR_ARG;
  const size_t np = (size_t)n_seq * P;
  const Span out[4] = {{traj, np * ((size_t)T + 1) * 8}, {code, np}, {steps, np * 4}, {stats, (size_t)n_seq * CHAIN_NSTAT * 8}};
  const Span in[3] = {{fw.flow, in_bytes}, {has_bw ? bw.flow : nullptr, in_bytes}, {pts, np * 8}};
  if (overlap_any(out, in)) return FOTG_ERR_ARG;
  DevGuard guard(device);
  if (!guard.ok) return hip_fail(guard.err);
  hipStream_t stream = (hipStream_t)stream_;
  if (stats) {
    const hipError_t e = hipMemsetAsync(stats, 0, out[3].bytes, stream);
    if (e != hipSuccess) return hip_fail(e);
  }
  const dim3 grid((unsigned)(((size_t)P + CHAIN_THREADS - 1) / CHAIN_THREADS), (unsigned)n_seq);
  if (has_bw)
    chain_points_kernel<Src, true><<<grid, CHAIN_THREADS, 0, stream>>>(fw, bw, T, w, h, alpha1, alpha2, P, pts, traj, code, steps, stats);
  else
    chain_points_kernel<Src, false><<<grid, CHAIN_THREADS, 0, stream>>>(fw, fw, T, w, h, alpha1, alpha2, P, pts, traj, code, steps, stats);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? FOTG_OK : hip_fail(e);
}

}  // namespace

extern "C" {

int fotg_flow_chain(int device, int n_seq, int T, const float *flows, const float *flows_bw, int w, int h, float alpha1, float alpha2,
                    float *total, unsigned char *code, int *steps, unsigned long long *stats, void *stream)
{
  if (!flows || !chain_args_ok(n_seq, T, w, h)) return FOTG_ERR_ARG;
  const size_t in_bytes = (size_t)n_seq * T * w * h * 2 * sizeof(float);
  return chain_dense(device, n_seq, T, DenseSrc{flows}, DenseSrc{flows_bw}, flows_bw != nullptr, in_bytes, w, h, alpha1, alpha2, total,
                     code, steps, stats, stream);
}

int fotg_track_points(int device, int n_seq, int T, const float *flows, const float *flows_bw, int w, int h, float alpha1,
                      float alpha2, int P, const float *pts, float *traj, unsigned char *code, int *steps, unsigned long long *stats,
                      void *stream)
{
  if (!flows || !chain_args_ok(n_seq, T, w, h)) return FOTG_ERR_ARG;
  const size_t in_bytes = (size_t)n_seq * T * w * h * 2 * sizeof(float);
  return chain_points(device, n_seq, T, DenseSrc{flows}, DenseSrc{flows_bw}, flows_bw != nullptr, in_bytes, w, h, alpha1, alpha2, P, pts,
                      traj, code, steps, stats, stream);
}

int fotg_upsample_crop_flow_chain(fotg_ctx *ctx, int T, const float *coarse_flows, const float *coarse_bw, float alpha1, float alpha2,
                                  float *total, unsigned char *code, int *steps, unsigned long long *stats, void *stream)
{
  CtxUpsampleGeom g;                 // a chain of T of the context's coarse flows: one sequence, the batch index is the step
  if (!fused_geom(ctx, T, coarse_flows, &g)) return FOTG_ERR_ARG;
  const size_t in_bytes = (size_t)T * g.wl * g.hl * 2 * sizeof(float);
  return chain_dense(g.device, 1, T, upsample_src(g, coarse_flows), upsample_src(g, coarse_bw), coarse_bw != nullptr, in_bytes, g.w_org,
                     g.h_org, alpha1, alpha2, total, code, steps, stats, stream);
}

int fotg_upsample_crop_track_points(fotg_ctx *ctx, int T, const float *coarse_flows, const float *coarse_bw, float alpha1,
                                    float alpha2, int P, const float *pts, float *traj, unsigned char *code, int *steps,
                                    unsigned long long *stats, void *stream)
{
  CtxUpsampleGeom g;
  if (!fused_geom(ctx, T, coarse_flows, &g)) return FOTG_ERR_ARG;
  const size_t in_bytes = (size_t)T * g.wl * g.hl * 2 * sizeof(float);
  return chain_points(g.device, 1, T, upsample_src(g, coarse_flows), upsample_src(g, coarse_bw), coarse_bw != nullptr, in_bytes, g.w_org,
                      g.h_org, alpha1, alpha2, P, pts, traj, code, steps, stats, stream);
}

}  // extern "C"
