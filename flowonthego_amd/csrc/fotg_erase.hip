// fotg_erase.hip -- C-ABI of the object removal (include/fotg.h fotg_erase / fotg_erase_motion / fotg_upsample_crop_erase and their
// 8-bit forms), kernel in erase.hip.h.  Per call: the validated plate indices, when given, copied into stream-ordered memory of the
// call, a stream-ordered memset of stats, and one launch over every frame.  Everything is enqueued on the caller's stream; the host
// array is consumed before the call returns; nothing synchronises.
#include <vector>
#include "host_call.h"
#include "erase.hip.h"

using namespace fotg;

namespace {

// src_mem / src_bytes: the extent of the memory behind `flow`
template <class Src, class T>
int erase_batch(int device, int n, const Src &flow, const void *src_mem, size_t src_bytes, const T *frames, int w, int h, int channels,
                int P, const T *plate, int W, int H, int ox, int oy, const int *index, const unsigned char *plate_code,
                const unsigned char *mask, const unsigned char *remove, int grow, int feather, T *dst, unsigned char *code, short *alpha,
                long long *stats, void *stream_)
{
  if (n < 1 || n > 65535 || P < 1 || P > 65535) return FOTG_ERR_ARG;
  if (w < 1 || h < 1 || w > ER_MAX_DIM || h > ER_MAX_DIM || W < 1 || H < 1 || W > ER_MAX_DIM || H > ER_MAX_DIM) return FOTG_ERR_ARG;
  if (ox < -ER_MAX_ORIGIN || ox > ER_MAX_ORIGIN || oy < -ER_MAX_ORIGIN || oy > ER_MAX_ORIGIN) return FOTG_ERR_ARG;
  if ((channels != 1 && channels != 3) || grow < 0 || grow > ER_MAXG || feather < 0 || feather > ER_MAXF) return FOTG_ERR_ARG;
  if (!remove || (!dst && !code && !alpha && !stats)) return FOTG_ERR_ARG;
  const bool sampled = dst || code || stats;                      // alpha alone reads nothing but remove
  if (sampled && (!frames || !plate || !src_mem)) return FOTG_ERR_ARG;
  if (!index && P != 1 && P != n) return FOTG_ERR_ARG;
  std::vector<int> ix;
  if (index) {
    ix.assign(index, index + n);
    for (int v : ix)
      if (v < 0 || v >= P) return FOTG_ERR_ARG;
  }
  const size_t hw = (size_t)w * h, HW = (size_t)W * H;
  const Span out[4] = {{dst, n * hw * channels * sizeof(T)}, {code, n * hw}, {alpha, n * hw * sizeof(short)},
                       {stats, (size_t)n * ER_NSTAT * sizeof(long long)}};
  const Span in[6] = {{frames, n * hw * channels * sizeof(T)}, {plate, P * HW * channels * sizeof(T)}, {src_mem, src_bytes},
                      {plate_code, P * HW}, {mask, n * hw}, {remove, n * hw}};
  if (overlap_any(out, in) || overlap_among(out)) return FOTG_ERR_ARG;
  DevGuard guard(device);
  if (!guard.ok) return hip_fail(guard.err);
  hipStream_t stream = (hipStream_t)stream_;
  int *dix = nullptr;
  Scratch mem(stream);
  hipError_t e = hipSuccess;
  if (index && sampled) {
    mem.get(&dix, ix.size() * sizeof(int));
    if (mem.err != hipSuccess) return mem.finish(mem.err);
    e = hipMemcpyAsync(dix, ix.data(), ix.size() * sizeof(int), hipMemcpyHostToDevice, stream);           // pageable: consumed on return
  }
  if (stats && e == hipSuccess) e = hipMemsetAsync(stats, 0, (size_t)n * ER_NSTAT * sizeof(long long), stream);
  if (e == hipSuccess) {
    const dim3 grid((unsigned)((w + ER_TW - 1) / ER_TW), (unsigned)((h + ER_TH - 1) / ER_TH), (unsigned)n);
    unsigned long long *st = reinterpret_cast<unsigned long long *>(stats);
    if (channels == 1)
      erase_kernel<Src, T, 1><<<grid, ER_THREADS, 0, stream>>>(flow, frames, plate, dix, P, plate_code, mask, remove, w, h, W, H, ox, oy, grow,
                                                               feather, dst, code, alpha, st);
    else
      erase_kernel<Src, T, 3><<<grid, ER_THREADS, 0, stream>>>(flow, frames, plate, dix, P, plate_code, mask, remove, w, h, W, H, ox, oy, grow,
                                                               feather, dst, code, alpha, st);
    e = hipGetLastError();
  }
  return mem.finish(e);
}

template <class T>
int erase_dense(int device, int n, const T *frames, int w, int h, int channels, int P, const T *plate, int W, int H, int ox, int oy,
                const int *index, const float *flows, const unsigned char *plate_code, const unsigned char *mask, const unsigned char *remove,
                int grow, int feather, T *dst, unsigned char *code, short *alpha, long long *stats, void *stream)
{
  const size_t bytes = n > 0 && w > 0 && h > 0 ? (size_t)n * w * h * 2 * sizeof(float) : 0;
  return erase_batch(device, n, DenseSrc{flows}, flows, bytes, frames, w, h, channels, P, plate, W, H, ox, oy, index, plate_code, mask, remove,
                     grow, feather, dst, code, alpha, stats, stream);
}

template <class T>
int erase_motion(int device, int n, const T *frames, int w, int h, int channels, int P, const T *plate, int W, int H, int ox, int oy,
                 const int *index, const double *params, const unsigned char *plate_code, const unsigned char *mask,
                 const unsigned char *remove, int grow, int feather, T *dst, unsigned char *code, short *alpha, long long *stats, void *stream)
{
  const size_t bytes = n > 0 ? (size_t)n * 6 * sizeof(double) : 0;
  return erase_batch(device, n, MotionSrc{params, w, h}, params, bytes, frames, w, h, channels, P, plate, W, H, ox, oy, index, plate_code,
                     mask, remove, grow, feather, dst, code, alpha, stats, stream);
}

template <class T>
int erase_fused(fotg_ctx *ctx, int n, const float *coarse, const T *frames, int channels, int P, const T *plate, int W, int H, int ox, int oy,
                const int *index, const unsigned char *plate_code, const unsigned char *mask, const unsigned char *remove, int grow,
                int feather, T *dst, unsigned char *code, short *alpha, long long *stats, void *stream)
{
  CtxUpsampleGeom g;
  if (!fused_geom(ctx, n, coarse, &g)) return FOTG_ERR_ARG;
  return erase_batch(g.device, n, upsample_src(g, coarse), coarse, (size_t)n * g.wl * g.hl * 2 * sizeof(float), frames, g.w_org, g.h_org,
                     channels, P, plate, W, H, ox, oy, index, plate_code, mask, remove, grow, feather, dst, code, alpha, stats, stream);
}

}  // namespace

extern "C" {

int fotg_erase(int device, int n, const float *frames, int w, int h, int channels, int P, const float *plate, int W, int H, int ox, int oy,
               const int *index, const float *flows, const unsigned char *plate_code, const unsigned char *mask, const unsigned char *remove,
               int grow, int feather, float *dst, unsigned char *code, short *alpha, long long *stats, void *stream)
{
  return erase_dense(device, n, frames, w, h, channels, P, plate, W, H, ox, oy, index, flows, plate_code, mask, remove, grow, feather, dst,
                     code, alpha, stats, stream);
}

int fotg_erase_u8(int device, int n, const unsigned char *frames, int w, int h, int channels, int P, const unsigned char *plate, int W, int H,
                  int ox, int oy, const int *index, const float *flows, const unsigned char *plate_code, const unsigned char *mask,
                  const unsigned char *remove, int grow, int feather, unsigned char *dst, unsigned char *code, short *alpha, long long *stats,
                  void *stream)
{
  return erase_dense(device, n, frames, w, h, channels, P, plate, W, H, ox, oy, index, flows, plate_code, mask, remove, grow, feather, dst,
                     code, alpha, stats, stream);
}

int fotg_erase_motion(int device, int n, const float *frames, int w, int h, int channels, int P, const float *plate, int W, int H, int ox,
                      int oy, const int *index, const double *params, const unsigned char *plate_code, const unsigned char *mask,
                      const unsigned char *remove, int grow, int feather, float *dst, unsigned char *code, short *alpha, long long *stats,
                      void *stream)
{
  return erase_motion(device, n, frames, w, h, channels, P, plate, W, H, ox, oy, index, params, plate_code, mask, remove, grow, feather, dst,
                      code, alpha, stats, stream);
}

int fotg_erase_motion_u8(int device, int n, const unsigned char *frames, int w, int h, int channels, int P, const unsigned char *plate, int W,
                         int H, int ox, int oy, const int *index, const double *params, const unsigned char *plate_code,
                         const unsigned char *mask, const unsigned char *remove, int grow, int feather, unsigned char *dst,
                         unsigned char *code, short *alpha, long long *stats, void *stream)
{
  return erase_motion(device, n, frames, w, h, channels, P, plate, W, H, ox, oy, index, params, plate_code, mask, remove, grow, feather, dst,
                      code, alpha, stats, stream);
}

int fotg_upsample_crop_erase(fotg_ctx *ctx, int n, const float *coarse_flows, const float *frames, int channels, int P, const float *plate,
                             int W, int H, int ox, int oy, const int *index, const unsigned char *plate_code, const unsigned char *mask,
                             const unsigned char *remove, int grow, int feather, float *dst, unsigned char *code, short *alpha,
                             long long *stats, void *stream)
{
  return erase_fused(ctx, n, coarse_flows, frames, channels, P, plate, W, H, ox, oy, index, plate_code, mask, remove, grow, feather, dst, code,
                     alpha, stats, stream);
}

int fotg_upsample_crop_erase_u8(fotg_ctx *ctx, int n, const float *coarse_flows, const unsigned char *frames, int channels, int P,
                                const unsigned char *plate, int W, int H, int ox, int oy, const int *index, const unsigned char *plate_code,
                                const unsigned char *mask, const unsigned char *remove, int grow, int feather, unsigned char *dst,
                                unsigned char *code, short *alpha, long long *stats, void *stream)
{
  return erase_fused(ctx, n, coarse_flows, frames, channels, P, plate, W, H, ox, oy, index, plate_code, mask, remove, grow, feather, dst, code,
                     alpha, stats, stream);
}

}  // extern "C"
