// fotg_plate.hip -- C-ABI of the background plate (include/fotg.h fotg_plate / fotg_plate_motion / fotg_upsample_crop_plate and
// their 8-bit forms), kernel in plate.hip.h.  Per call: the validated frame indices copied into stream-ordered memory of the call,
// one launch over every plate and, when statistics are asked for, warp_fold_kernel over the per-wave partials.  The dynamic LDS
// of the launch is sized by K; above the default limit the kernel is opted in through lds_opt_in.  Everything is enqueued on the
// caller's stream; the host array is consumed before the call returns.
#include <atomic>
#include <vector>
#include "host_call.h"
#include "plate.hip.h"

using namespace fotg;

namespace {

// canvas rows per workgroup (64 rows threads): the same bits for every value; the default is the one that measured faster
// 
std::atomic<int> g_rows{1};

template <class Src, class T, int NOC>
hipError_t launch(const dim3 &grid, int threads, int K, hipStream_t stream, const Src &flow, const T *frames, const T *ref,
                  const unsigned char *occ, const unsigned char *exclude, const int *dix, int w, int h, int W, int H, int ox, int oy,
                  int mode, int min_count, float fill, T *dst, unsigned char *count, unsigned char *code, WarpPartial *part)
{
  const size_t lds = plate_lds_bytes(K, NOC, threads);
  if (lds > 64 * 1024) {
    const hipError_t e = lds_opt_in(plate_kernel<Src, T, NOC>, (int)lds);
    if (e != hipSuccess) return e;
  }
  plate_kernel<Src, T, NOC><<<grid, threads, lds, stream>>>(flow, frames, ref, occ, exclude, dix, K, w, h, W, H, ox, oy, mode, min_count,
                                                           fill, dst, count, code, part);
  return hipGetLastError();
}

// src_mem / src_bytes: the extent of the memory behind `flow`
template <class Src, class T>
int plate_batch(int device, int n, int K, int nframes, const Src &flow, const void *src_mem, size_t src_bytes, const T *frames, int w,
                int h, int channels, const int *index, int W, int H, int ox, int oy, const unsigned char *occ,
                const unsigned char *exclude, int mode, int min_count, float fill, const T *ref, T *dst, unsigned char *count,
                unsigned char *code, double *stats, void *stream_)
{
  if (n < 1 || n > 65535 || K < 1 || K > PLATE_MAXK || nframes < 1) return FOTG_ERR_ARG;
  if (w < 1 || h < 1 || w > PLATE_MAX_DIM || h > PLATE_MAX_DIM || W < 1 || H < 1 || W > PLATE_MAX_DIM || H > PLATE_MAX_DIM) return FOTG_ERR_ARG;
  if (ox < -PLATE_MAX_ORIGIN || ox > PLATE_MAX_ORIGIN || oy < -PLATE_MAX_ORIGIN || oy > PLATE_MAX_ORIGIN) return FOTG_ERR_ARG;
  if ((channels != 1 && channels != 3) || (mode != 0 && mode != 1) || min_count < 1 || min_count > K) return FOTG_ERR_ARG;
  if (!frames || !src_mem || !index) return FOTG_ERR_ARG;
  if (!dst && !count && !code && !stats) return FOTG_ERR_ARG;
  std::vector<int> ix((size_t)n * K);
  for (size_t j = 0; j < ix.size(); ++j) {
    if (index[j] < -1 || index[j] >= nframes) return FOTG_ERR_ARG;
    ix[j] = index[j];
  }
  const size_t HW = (size_t)W * H, hw = (size_t)w * h;
  const size_t img = HW * channels * sizeof(T);
  const Span out[4] = {{dst, n * img}, {count, n * HW}, {code, n * HW}, {stats, (size_t)n * WARP_NSTAT * sizeof(double)}};
  const Span in[5] = {{frames, nframes * hw * channels * sizeof(T)}, {src_mem, src_bytes}, {occ, (size_t)n * K * HW},
                      {exclude, nframes * hw}, {ref, n * img}};
  if (overlap_any(out, in) || overlap_among(out)) return FOTG_ERR_ARG;
  const int rows = g_rows.load();
  const unsigned tiles_x = (unsigned)((W + PLATE_TW - 1) / PLATE_TW), tiles_y = (unsigned)((H + rows - 1) / rows);
  const int blocks = (int)(tiles_x * (unsigned)H);               // partials per plate: one per wave, <= 2^22
  DevGuard guard(device);
  if (!guard.ok) return hip_fail(guard.err);
  hipStream_t stream = (hipStream_t)stream_;
  int *dix = nullptr;
  WarpPartial *part = nullptr;
  Scratch mem(stream);
  mem.get(&dix, ix.size() * sizeof(int));
  if (stats) mem.get(&part, (size_t)n * blocks * sizeof(WarpPartial));
  if (mem.err != hipSuccess) return mem.finish(mem.err);
  hipError_t e = hipMemcpyAsync(dix, ix.data(), ix.size() * sizeof(int), hipMemcpyHostToDevice, stream);   // pageable: consumed on return
  if (e == hipSuccess) {
    const dim3 grid(tiles_x, tiles_y, (unsigned)n);
    const int threads = PLATE_TW * rows;
    if (channels == 1)
      e = launch<Src, T, 1>(grid, threads, K, stream, flow, frames, ref, occ, exclude, dix, w, h, W, H, ox, oy, mode, min_count, fill, dst,
                            count, code, part);
    else
      e = launch<Src, T, 3>(grid, threads, K, stream, flow, frames, ref, occ, exclude, dix, w, h, W, H, ox, oy, mode, min_count, fill, dst,
                            count, code, part);
  }
  if (stats && e == hipSuccess) e = warp_fold(part, blocks, n, stats, stream);
  return mem.finish(e);
}

template <class T>
int plate_dense(int device, int n, int K, int nframes, const T *frames, int w, int h, int channels, const int *index, const float *flows,
                int W, int H, int ox, int oy, const unsigned char *occ, const unsigned char *exclude, int mode, int min_count, float fill,
                const T *ref, T *dst, unsigned char *count, unsigned char *code, double *stats, void *stream)
{
  const size_t bytes = n > 0 && K > 0 && W > 0 && H > 0 ? (size_t)n * K * W * H * 2 * sizeof(float) : 0;
  return plate_batch(device, n, K, nframes, DenseSrc{flows}, flows, bytes, frames, w, h, channels, index, W, H, ox, oy, occ, exclude, mode,
                     min_count, fill, ref, dst, count, code, stats, stream);
}

template <class T>
int plate_motion(int device, int n, int K, int nframes, const T *frames, int w, int h, int channels, const int *index,
                 const double *params, int W, int H, int ox, int oy, const unsigned char *occ, const unsigned char *exclude, int mode,
                 int min_count, float fill, const T *ref, T *dst, unsigned char *count, unsigned char *code, double *stats, void *stream)
{
  const size_t bytes = n > 0 && K > 0 ? (size_t)n * K * 6 * sizeof(double) : 0;
  return plate_batch(device, n, K, nframes, MotionSrc{params, w, h}, params, bytes, frames, w, h, channels, index, W, H, ox, oy, occ,
                     exclude, mode, min_count, fill, ref, dst, count, code, stats, stream);
}

template <class T>
int plate_fused(fotg_ctx *ctx, int n, int K, int nframes, const float *coarse, const T *frames, int channels, const int *index,
                const unsigned char *occ, const unsigned char *exclude, int mode, int min_count, float fill, const T *ref, T *dst,
                unsigned char *count, unsigned char *code, double *stats, void *stream)
{
  CtxUpsampleGeom g;
  if (!ctx || !coarse || ctx_upsample_geom(ctx, &g) != FOTG_OK) return FOTG_ERR_ARG;
  if (n < 1 || K < 1 || K > PLATE_MAXK || (long)n * K > g.max_batch || g.nch != 2) return FOTG_ERR_ARG;
  return plate_batch(g.device, n, K, nframes, upsample_src(g, coarse), coarse, (size_t)n * K * g.wl * g.hl * 2 * sizeof(float), frames,
                     g.w_org, g.h_org, channels, index, g.w_org, g.h_org, 0, 0, occ, exclude, mode, min_count, fill, ref, dst, count, code,
                     stats, stream);
}

}  // namespace

extern "C" {

int fotg_plate(int device, int n, int K, int T, const float *frames, int w, int h, int channels, const int *index, const float *flows,
               int W, int H, int ox, int oy, const unsigned char *occ, const unsigned char *exclude, int mode, int min_count, float fill,
               const float *ref, float *dst, unsigned char *count, unsigned char *code, double *stats, void *stream)
{
  return plate_dense(device, n, K, T, frames, w, h, channels, index, flows, W, H, ox, oy, occ, exclude, mode, min_count, fill, ref, dst,
                     count, code, stats, stream);
}

int fotg_plate_u8(int device, int n, int K, int T, const unsigned char *frames, int w, int h, int channels, const int *index,
                  const float *flows, int W, int H, int ox, int oy, const unsigned char *occ, const unsigned char *exclude, int mode,
                  int min_count, float fill, const unsigned char *ref, unsigned char *dst, unsigned char *count, unsigned char *code,
                  double *stats, void *stream)
{
  return plate_dense(device, n, K, T, frames, w, h, channels, index, flows, W, H, ox, oy, occ, exclude, mode, min_count, fill, ref, dst,
                     count, code, stats, stream);
}

int fotg_plate_motion(int device, int n, int K, int T, const float *frames, int w, int h, int channels, const int *index,
                      const double *params, int W, int H, int ox, int oy, const unsigned char *occ, const unsigned char *exclude, int mode,
                      int min_count, float fill, const float *ref, float *dst, unsigned char *count, unsigned char *code, double *stats,
                      void *stream)
{
  return plate_motion(device, n, K, T, frames, w, h, channels, index, params, W, H, ox, oy, occ, exclude, mode, min_count, fill, ref, dst,
                      count, code, stats, stream);
}

int fotg_plate_motion_u8(int device, int n, int K, int T, const unsigned char *frames, int w, int h, int channels, const int *index,
                         const double *params, int W, int H, int ox, int oy, const unsigned char *occ, const unsigned char *exclude,
                         int mode, int min_count, float fill, const unsigned char *ref, unsigned char *dst, unsigned char *count,
                         unsigned char *code, double *stats, void *stream)
{
  return plate_motion(device, n, K, T, frames, w, h, channels, index, params, W, H, ox, oy, occ, exclude, mode, min_count, fill, ref, dst,
                      count, code, stats, stream);
}

int fotg_upsample_crop_plate(fotg_ctx *ctx, int n, int K, int T, const float *coarse_flows, const float *frames, int channels,
                             const int *index, const unsigned char *occ, const unsigned char *exclude, int mode, int min_count, float fill,
                             const float *ref, float *dst, unsigned char *count, unsigned char *code, double *stats, void *stream)
{
  return plate_fused(ctx, n, K, T, coarse_flows, frames, channels, index, occ, exclude, mode, min_count, fill, ref, dst, count, code, stats,
                     stream);
}

int fotg_upsample_crop_plate_u8(fotg_ctx *ctx, int n, int K, int T, const float *coarse_flows, const unsigned char *frames, int channels,
                                const int *index, const unsigned char *occ, const unsigned char *exclude, int mode, int min_count,
                                float fill, const unsigned char *ref, unsigned char *dst, unsigned char *count, unsigned char *code,
                                double *stats, void *stream)
{
  return plate_fused(ctx, n, K, T, coarse_flows, frames, channels, index, occ, exclude, mode, min_count, fill, ref, dst, count, code, stats,
                     stream);
}

int fotg_plate_rows(int rows)
{
  if (rows == 1 || rows == 2 || rows == PLATE_MAX_ROWS) return g_rows.exchange(rows);
  return g_rows.load();
}

}  // extern "C"
