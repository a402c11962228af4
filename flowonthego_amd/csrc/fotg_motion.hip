// fotg_motion.hip -- C-ABI of the global-motion fit (include/fotg.h fotg_fit_motion / fotg_upsample_crop_fit_motion /
// fotg_motion_flow), kernels in motion.hip.h.  Per call: iters + 1 rounds of (one pass over every image of the batch, the solve),
// then the final pass where codes, residuals or counts are asked for.  The accumulators and the parameters stay on the device;
// everything is asynchronous on the caller's stream, nothing synchronises with the host.
#include <atomic>
#include "host_call.h"
#include "motion.hip.h"

using namespace fotg;

namespace {

// how a pass's sums reach the image's accumulators: 0 one 64-bit atomic per workgroup and sum, 1 per-workgroup partials and
// motion_fold_kernel.  Same bits either way (integer sums); the default is the one that measured faster, in every form, by
// 0.06 .. 0.09 ms per pass over 64 x 1080p: the fold.
std::atomic<int> g_ending{1};

template <class Src, int PASS>
void launch_pass(dim3 grid, hipStream_t stream, const Src &flow, const unsigned char *mask, int w, int h, const double *params,
                 float thresh2, long long *acc, int acc_stride, long long *part, unsigned char *code, float *residual)
{
  motion_pass_kernel<Src, PASS><<<grid, MOTION_THREADS, 0, stream>>>(flow, mask, w, h, params, thresh2, acc, acc_stride, part, code, residual);
}

template <class Src>
int fit_batch(int device, int n, const Src &flow, size_t in_bytes, const unsigned char *mask, int w, int h, int model, int iters,
              float thresh, double *params, unsigned char *code, float *residual, long long *stats, long long *sums, void *stream_)
{
  if (n < 1 || n > 65535 || w < 1 || h < 1 || w > MOTION_MAX_DIM || h > MOTION_MAX_DIM) return FOTG_ERR_ARG;
  if (model < 0 || model > 2 || iters < 0 || iters > MOTION_MAX_ITERS || !(thresh >= 0.f) || !params) return FOTG_ERR_ARG;
  const size_t hw = (size_t)w * h;
  const Span out[5] = {{params, (size_t)n * 6 * 8}, {code, n * hw}, {residual, n * hw * 8}, {stats, (size_t)n * MOTION_NSTAT * 8},
                       {sums, (size_t)n * MOTION_NSUM * 8}};
  const Span in[2] = {{flow.flow, in_bytes}, {mask, n * hw}};
  if (overlap_any(out, in) || overlap_among(out)) return FOTG_ERR_ARG;
  DevGuard guard(device);
  if (!guard.ok) return hip_fail(guard.err);
  hipStream_t stream = (hipStream_t)stream_;
  const int blocks = (int)(((hw + 3) / 4 + MOTION_THREADS - 1) / MOTION_THREADS);       // <= 2^18 for 16384 x 16384
  const bool fold = g_ending.load() == 1;
  const bool final_pass = code || residual || stats;
  // the call's memory: n x 12 accumulators, n `bad` flags, then (fold ending) the per-workgroup partials
  const size_t head = (size_t)n * (MOTION_NSUM + 1);
  long long *ws = nullptr;
  Scratch mem(stream);
  if (!mem.get(&ws, (head + (fold ? (size_t)n * blocks * MOTION_NSUM : 0)) * sizeof(long long))) return mem.finish(mem.err);
  long long *acc = ws, *bad = ws + (size_t)n * MOTION_NSUM, *part = fold ? ws + head : nullptr;
  hipError_t e = hipMemsetAsync(ws, 0, head * sizeof(long long), stream);
  if (e == hipSuccess) e = hipMemsetAsync(params, 0, out[0].bytes, stream);
  if (e == hipSuccess && stats) e = hipMemsetAsync(stats, 0, out[3].bytes, stream);
  const float thresh2 = thresh * thresh;
  const dim3 grid((unsigned)blocks, (unsigned)n);
  for (int r = 0; r <= iters && e == hipSuccess; ++r) {
    if (r == 0)
      launch_pass<Src, MOTION_ROUND0>(grid, stream, flow, mask, w, h, params, thresh2, fold ? nullptr : acc, MOTION_NSUM, part, nullptr, nullptr);
    else
      launch_pass<Src, MOTION_ROUND>(grid, stream, flow, mask, w, h, params, thresh2, fold ? nullptr : acc, MOTION_NSUM, part, nullptr, nullptr);
    if (fold) motion_fold_kernel<MOTION_NSUM><<<dim3((unsigned)n), MOTION_THREADS, 0, stream>>>(part, blocks, acc, MOTION_NSUM);
    const bool last = r == iters;
    motion_solve_kernel<<<dim3((unsigned)((n + 63) / 64)), 64, 0, stream>>>(acc, n, model, w, h, params, bad, last ? sums : nullptr,
                                                                           last ? stats : nullptr);
    e = hipGetLastError();
  }
  if (final_pass && e == hipSuccess) {
    launch_pass<Src, MOTION_FINAL>(grid, stream, flow, mask, w, h, params, thresh2, fold ? nullptr : stats, MOTION_NSTAT,
                                   stats ? part : nullptr, code, residual);
    if (fold && stats) motion_fold_kernel<4><<<dim3((unsigned)n), MOTION_THREADS, 0, stream>>>(part, blocks, stats, MOTION_NSTAT);
    e = hipGetLastError();
  }
  return mem.finish(e);
}

}  // namespace

extern "C" {

int fotg_fit_motion(int device, int n, const float *flow, const unsigned char *mask, int w, int h, int model, int iters, float thresh,
                    double *params, unsigned char *code, float *residual, long long *stats, long long *sums, void *stream)
{
  if (!flow || n < 1 || w < 1 || h < 1) return FOTG_ERR_ARG;
  return fit_batch(device, n, DenseSrc{flow}, (size_t)n * w * h * 2 * sizeof(float), mask, w, h, model, iters, thresh, params, code,
                   residual, stats, sums, stream);
}

int fotg_upsample_crop_fit_motion(fotg_ctx *ctx, int n, const float *coarse_flow, const unsigned char *mask, int model, int iters,
                                  float thresh, double *params, unsigned char *code, float *residual, long long *stats, long long *sums,
                                  void *stream)
{
  CtxUpsampleGeom g;
  if (!fused_geom(ctx, n, coarse_flow, &g)) return FOTG_ERR_ARG;
  return fit_batch(g.device, n, upsample_src(g, coarse_flow), (size_t)n * g.wl * g.hl * 2 * sizeof(float), mask, g.w_org, g.h_org,
                   model, iters, thresh, params, code, residual, stats, sums, stream);
}

int fotg_motion_flow(int device, int n, const double *params, int w, int h, float *flow, void *stream)
{
  if (n < 1 || n > 65535 || w < 1 || h < 1 || !params || !flow) return FOTG_ERR_ARG;
  const size_t hw = (size_t)w * h;
  const size_t blocks = ((hw + 3) / 4 + MOTION_THREADS - 1) / MOTION_THREADS;
  if (blocks > 0x7fffffffUL) return FOTG_ERR_ARG;
  if (overlap(Span{params, (size_t)n * 6 * 8}, Span{flow, n * hw * 8})) return FOTG_ERR_ARG;
  DevGuard guard(device);
  if (!guard.ok) return hip_fail(guard.err);
  motion_flow_kernel<<<dim3((unsigned)blocks, (unsigned)n), MOTION_THREADS, 0, (hipStream_t)stream>>>(params, w, h, flow);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? FOTG_OK : hip_fail(e);
}

int fotg_motion_ending(int ending)
{
  if (ending == 0 || ending == 1) return g_ending.exchange(ending);
  return g_ending.load();
}

}  // extern "C"
