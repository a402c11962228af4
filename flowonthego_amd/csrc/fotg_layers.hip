// fotg_layers.hip -- C-ABI of the motion layers (include/fotg.h fotg_motion_layers / fotg_upsample_crop_motion_layers), kernels in
// layers.hip.h.  Per call: the seeding layer by layer (a tile pass and the selection, then iters + 1 rounds of pass, fold, solve),
// `rounds` refinement rounds (assign pass, fold, solve of every layer), then the final pass where labels, residuals, records or
// stats are asked for.  The parameters, the layers' flags and every sum stay on the device; everything is asynchronous on the
// caller's stream, nothing synchronises with the host.
#include "host_call.h"
#include "layers.hip.h"

using namespace fotg;

namespace {

template <class Src>
int layers_batch(int device, int n, const Src &flow, size_t in_bytes, const unsigned char *mask, int w, int h, int K, int model, int iters,
                 int rounds, float thresh, const double *init, double *params, unsigned char *labels, float *residual, long long *records,
                 long long *stats, long long *sums, void *stream_)
{
  if (n < 1 || n > 65535 || w < 1 || h < 1 || w > MOTION_MAX_DIM || h > MOTION_MAX_DIM || K < 1 || K > LAYERS_MAX) return FOTG_ERR_ARG;
  if (model < 0 || model > 2 || iters < 0 || iters > MOTION_MAX_ITERS || rounds < 0 || rounds > LAYERS_MAX_ROUNDS || !(thresh >= 0.f) || !params)
    return FOTG_ERR_ARG;
  const size_t hw = (size_t)w * h, nk = (size_t)n * K;
  const Span out[6] = {{params, nk * 6 * 8}, {labels, n * hw}, {residual, n * hw * 8}, {records, nk * LAYERS_NREC * 8},
                       {stats, (size_t)n * LAYERS_NSTAT * 8}, {sums, nk * MOTION_NSUM * 8}};
  const Span in[3] = {{flow.flow, in_bytes}, {mask, n * hw}, {init, nk * 6 * 8}};
  if (overlap_any(out, in) || overlap_among(out)) return FOTG_ERR_ARG;
  DevGuard guard(device);
  if (!guard.ok) return hip_fail(guard.err);
  hipStream_t stream = (hipStream_t)stream_;
  const int blocks = (int)(((hw + 3) / 4 + MOTION_THREADS - 1) / MOTION_THREADS);       // <= 2^18 for 16384 x 16384
  const int tx = (w + LAYERS_TILE - 1) / LAYERS_TILE, tiles = tx * ((h + LAYERS_TILE - 1) / LAYERS_TILE);   // <= 2^18
  const bool final_pass = labels || residual || records || stats;
  // the call's memory: the layers' state, the folded sums (K + 1 rows of 12 per image), the tile sums, the workgroups' partials
  const size_t n_st = nk * LAYERS_NST, n_acc = (size_t)n * (K + 1) * MOTION_NSUM, n_tile = init || K == 1 ? 0 : (size_t)n * tiles * 3;
  const size_t n_part = (size_t)n * blocks * K * MOTION_NSUM;                           // >= (K + 1) x 4 of the final pass
  long long *ws = nullptr;
  Scratch mem(stream);
  if (!mem.get(&ws, (n_st + n_acc + n_tile + n_part) * sizeof(long long))) return mem.finish(mem.err);
  long long *st = ws, *acc = st + n_st, *tile_sums = acc + n_acc, *part = tile_sums + n_tile;
  hipError_t e = hipSuccess;
  if (sums) e = hipMemsetAsync(sums, 0, out[5].bytes, stream);
  const float thresh2 = thresh * thresh;
  const dim3 grid((unsigned)blocks, (unsigned)n);
  const int acc_stride = (K + 1) * MOTION_NSUM;
  const auto solve = [&](int k0, int k1, int close) {
    const int total = n * (k1 - k0);
    layers_solve_kernel<<<dim3((unsigned)((total + 63) / 64)), 64, 0, stream>>>(acc, n, K, k0, k1, close, model, w, h, params, st, sums);
  };
  if (e == hipSuccess) {
    layers_init_kernel<<<dim3((unsigned)((nk + 63) / 64)), 64, 0, stream>>>((int)nk, init, params, st, K);
    e = hipGetLastError();
  }
  for (int k = 0; k < K && !init && e == hipSuccess; ++k) {
    if (k > 0) {
      layers_tile_kernel<Src><<<dim3((unsigned)tiles, (unsigned)n), MOTION_THREADS, 0, stream>>>(flow, mask, w, h, tx, params, st, K, k, thresh2,
                                                                                              tile_sums);
      layers_select_kernel<<<dim3((unsigned)n), MOTION_THREADS, 0, stream>>>(tile_sums, tiles, w, h, K, k, params, st);
    }
    for (int r = 0; r <= iters; ++r) {
      layers_pass_kernel<Src, LAYERS_ROUND><<<grid, MOTION_THREADS, 0, stream>>>(flow, mask, w, h, params, st, K, k, k == 0 && r == 0, thresh2,
                                                                                 part, nullptr, nullptr);
      layers_fold_kernel<MOTION_NSUM><<<dim3(1, (unsigned)n), MOTION_THREADS, 0, stream>>>(part, blocks, acc, acc_stride, k);
      solve(k, k + 1, r == iters);
    }
    e = hipGetLastError();
  }
  for (int r = 0; r < rounds && e == hipSuccess; ++r) {
    layers_pass_kernel<Src, LAYERS_ASSIGN><<<grid, MOTION_THREADS, 0, stream>>>(flow, mask, w, h, params, st, K, 0, 0, thresh2, part, nullptr,
                                                                                nullptr);
    layers_fold_kernel<MOTION_NSUM><<<dim3((unsigned)K, (unsigned)n), MOTION_THREADS, 0, stream>>>(part, blocks, acc, acc_stride, 0);
    solve(0, K, 0);
    e = hipGetLastError();
  }
  if (final_pass && e == hipSuccess) {
    layers_pass_kernel<Src, LAYERS_FINAL><<<grid, MOTION_THREADS, 0, stream>>>(flow, mask, w, h, params, st, K, 0, 0, thresh2, part, labels,
                                                                               residual);
    layers_fold_kernel<4><<<dim3((unsigned)(K + 1), (unsigned)n), MOTION_THREADS, 0, stream>>>(part, blocks, acc, (K + 1) * 4, 0);
    layers_records_kernel<<<dim3((unsigned)((nk + 63) / 64)), 64, 0, stream>>>(acc, st, n, K, records, stats);
    e = hipGetLastError();
  }
  return mem.finish(e);
}

}  // namespace

extern "C" {

int fotg_motion_layers(int device, int n, const float *flow, const unsigned char *mask, int w, int h, int layers, int model, int iters,
                       int rounds, float thresh, const double *init, double *params, unsigned char *labels, float *residual,
                       long long *records, long long *stats, long long *sums, void *stream)
{
  if (!flow || n < 1 || w < 1 || h < 1) return FOTG_ERR_ARG;
  return layers_batch(device, n, DenseSrc{flow}, (size_t)n * w * h * 2 * sizeof(float), mask, w, h, layers, model, iters, rounds, thresh,
                      init, params, labels, residual, records, stats, sums, stream);
}

int fotg_upsample_crop_motion_layers(fotg_ctx *ctx, int n, const float *coarse_flow, const unsigned char *mask, int layers, int model,
                                     int iters, int rounds, float thresh, const double *init, double *params, unsigned char *labels,
                                     float *residual, long long *records, long long *stats, long long *sums, void *stream)
{
  CtxUpsampleGeom g;
  if (!fused_geom(ctx, n, coarse_flow, &g)) return FOTG_ERR_ARG;
  return layers_batch(g.device, n, upsample_src(g, coarse_flow), (size_t)n * g.wl * g.hl * 2 * sizeof(float), mask, g.w_org, g.h_org, layers,
                      model, iters, rounds, thresh, init, params, labels, residual, records, stats, sums, stream);
}

}  // extern "C"
