// fotg_subtract.hip -- C-ABI of the background subtraction against a plate (include/fotg.h fotg_subtract / fotg_subtract_motion /
// fotg_upsample_crop_subtract and their 8-bit forms), kernel in subtract.hip.h.  Per call: the validated plate indices, when given,
// copied into stream-ordered memory of the call, a stream-ordered memset of stats, and one launch over every frame.  Everything is
// enqueued on the caller's stream; the host array is consumed before the call returns; nothing synchronises.
#include <cmath>
#include <vector>
#include "host_call.h"
#include "subtract.hip.h"

using namespace fotg;

namespace {

// L = lrintf(16 low), Hh = lrintf(16 high); false unless 0 <= L <= Hh <= 32767
bool thresholds(float low, float high, int *L, int *Hh)
{
  const float l = 16.f * low, hi = 16.f * high;
  if (!(l >= -1.f && l <= 32768.f && hi >= -1.f && hi <= 32768.f)) return false;      // (a NaN fails every comparison)
  *L = (int)lrintf(l);
  *Hh = (int)lrintf(hi);
  return 0 <= *L && *L <= *Hh && *Hh <= SUB_MAXQ;
}

// src_mem / src_bytes: the extent of the memory behind `flow`
template <class Src, class T>
int subtract_batch(int device, int n, const Src &flow, const void *src_mem, size_t src_bytes, const T *frames, int w, int h, int channels,
                   int P, const T *plate, int W, int H, int ox, int oy, const int *index, const unsigned char *plate_code,
                   const unsigned char *mask, float low, float high, int window, unsigned char *code, short *diff, float *evidence,
                   long long *stats, void *stream_)
{
  int L = 0, Hh = 0;
  if (n < 1 || n > 65535 || P < 1 || P > 65535) return FOTG_ERR_ARG;
  if (w < 1 || h < 1 || w > SUB_MAX_DIM || h > SUB_MAX_DIM || W < 1 || H < 1 || W > SUB_MAX_DIM || H > SUB_MAX_DIM) return FOTG_ERR_ARG;
  if (ox < -SUB_MAX_ORIGIN || ox > SUB_MAX_ORIGIN || oy < -SUB_MAX_ORIGIN || oy > SUB_MAX_ORIGIN) return FOTG_ERR_ARG;
  if ((channels != 1 && channels != 3) || window < 0 || window > SUB_MAXR || !thresholds(low, high, &L, &Hh)) return FOTG_ERR_ARG;
  if (!frames || !plate || !src_mem) return FOTG_ERR_ARG;
  if (!code && !diff && !evidence && !stats) return FOTG_ERR_ARG;
  if (!index && P != 1 && P != n) return FOTG_ERR_ARG;
  std::vector<int> ix;
  if (index) {
    ix.assign(index, index + n);
    for (int v : ix)
      if (v < 0 || v >= P) return FOTG_ERR_ARG;
  }
  const size_t hw = (size_t)w * h, HW = (size_t)W * H;
  const Span out[4] = {{code, n * hw}, {diff, n * hw * sizeof(short)}, {evidence, n * hw * 2 * sizeof(float)},
                       {stats, (size_t)n * SUB_NSTAT * sizeof(long long)}};
  const Span in[5] = {{frames, n * hw * channels * sizeof(T)}, {plate, P * HW * channels * sizeof(T)}, {src_mem, src_bytes},
                      {plate_code, P * HW}, {mask, n * hw}};
  if (overlap_any(out, in) || overlap_among(out)) return FOTG_ERR_ARG;
  DevGuard guard(device);
  if (!guard.ok) return hip_fail(guard.err);
  hipStream_t stream = (hipStream_t)stream_;
  int *dix = nullptr;
  Scratch mem(stream);
  hipError_t e = hipSuccess;
  if (index) {
    mem.get(&dix, ix.size() * sizeof(int));
    if (mem.err != hipSuccess) return mem.finish(mem.err);
    e = hipMemcpyAsync(dix, ix.data(), ix.size() * sizeof(int), hipMemcpyHostToDevice, stream);           // pageable: consumed on return
  }
  if (stats && e == hipSuccess) e = hipMemsetAsync(stats, 0, (size_t)n * SUB_NSTAT * sizeof(long long), stream);
  if (e == hipSuccess) {
    const dim3 grid((unsigned)((w + SUB_TW - 1) / SUB_TW), (unsigned)((h + SUB_TH - 1) / SUB_TH), (unsigned)n);
    unsigned long long *st = reinterpret_cast<unsigned long long *>(stats);
    if (channels == 1)
      subtract_kernel<Src, T, 1><<<grid, SUB_THREADS, 0, stream>>>(flow, frames, plate, dix, P, plate_code, mask, w, h, W, H, ox, oy, window, L,
                                                                   Hh, code, diff, evidence, st);
    else
      subtract_kernel<Src, T, 3><<<grid, SUB_THREADS, 0, stream>>>(flow, frames, plate, dix, P, plate_code, mask, w, h, W, H, ox, oy, window, L,
                                                                   Hh, code, diff, evidence, st);
    e = hipGetLastError();
  }
  return mem.finish(e);
}

template <class T>
int subtract_dense(int device, int n, const T *frames, int w, int h, int channels, int P, const T *plate, int W, int H, int ox, int oy,
                   const int *index, const float *flows, const unsigned char *plate_code, const unsigned char *mask, float low, float high,
                   int window, unsigned char *code, short *diff, float *evidence, long long *stats, void *stream)
{
  const size_t bytes = n > 0 && w > 0 && h > 0 ? (size_t)n * w * h * 2 * sizeof(float) : 0;
  return subtract_batch(device, n, DenseSrc{flows}, flows, bytes, frames, w, h, channels, P, plate, W, H, ox, oy, index, plate_code, mask, low,
                        high, window, code, diff, evidence, stats, stream);
}

template <class T>
int subtract_motion(int device, int n, const T *frames, int w, int h, int channels, int P, const T *plate, int W, int H, int ox, int oy,
                    const int *index, const double *params, const unsigned char *plate_code, const unsigned char *mask, float low,
                    float high, int window, unsigned char *code, short *diff, float *evidence, long long *stats, void *stream)
{
  const size_t bytes = n > 0 ? (size_t)n * 6 * sizeof(double) : 0;
  return subtract_batch(device, n, MotionSrc{params, w, h}, params, bytes, frames, w, h, channels, P, plate, W, H, ox, oy, index, plate_code,
                        mask, low, high, window, code, diff, evidence, stats, stream);
}

template <class T>
int subtract_fused(fotg_ctx *ctx, int n, const float *coarse, const T *frames, int channels, int P, const T *plate, int W, int H, int ox,
                   int oy, const int *index, const unsigned char *plate_code, const unsigned char *mask, float low, float high, int window,
                   unsigned char *code, short *diff, float *evidence, long long *stats, void *stream)
{
  CtxUpsampleGeom g;
  if (!fused_geom(ctx, n, coarse, &g)) return FOTG_ERR_ARG;
  return subtract_batch(g.device, n, upsample_src(g, coarse), coarse, (size_t)n * g.wl * g.hl * 2 * sizeof(float), frames, g.w_org, g.h_org,
                        channels, P, plate, W, H, ox, oy, index, plate_code, mask, low, high, window, code, diff, evidence, stats, stream);
}

}  // namespace

extern "C" {

int fotg_subtract(int device, int n, const float *frames, int w, int h, int channels, int P, const float *plate, int W, int H, int ox,
                  int oy, const int *index, const float *flows, const unsigned char *plate_code, const unsigned char *mask, float low,
                  float high, int window, unsigned char *code, short *diff, float *evidence, long long *stats, void *stream)
{
  return subtract_dense(device, n, frames, w, h, channels, P, plate, W, H, ox, oy, index, flows, plate_code, mask, low, high, window, code,
                        diff, evidence, stats, stream);
}

int fotg_subtract_u8(int device, int n, const unsigned char *frames, int w, int h, int channels, int P, const unsigned char *plate, int W,
                     int H, int ox, int oy, const int *index, const float *flows, const unsigned char *plate_code,
                     const unsigned char *mask, float low, float high, int window, unsigned char *code, short *diff, float *evidence,
                     long long *stats, void *stream)
{
  return subtract_dense(device, n, frames, w, h, channels, P, plate, W, H, ox, oy, index, flows, plate_code, mask, low, high, window, code,
                        diff, evidence, stats, stream);
}

int fotg_subtract_motion(int device, int n, const float *frames, int w, int h, int channels, int P, const float *plate, int W, int H,
                         int ox, int oy, const int *index, const double *params, const unsigned char *plate_code,
                         const unsigned char *mask, float low, float high, int window, unsigned char *code, short *diff, float *evidence,
                         long long *stats, void *stream)
{
  return subtract_motion(device, n, frames, w, h, channels, P, plate, W, H, ox, oy, index, params, plate_code, mask, low, high, window, code,
                         diff, evidence, stats, stream);
}

int fotg_subtract_motion_u8(int device, int n, const unsigned char *frames, int w, int h, int channels, int P, const unsigned char *plate,
                            int W, int H, int ox, int oy, const int *index, const double *params, const unsigned char *plate_code,
                            const unsigned char *mask, float low, float high, int window, unsigned char *code, short *diff,
                            float *evidence, long long *stats, void *stream)
{
  return subtract_motion(device, n, frames, w, h, channels, P, plate, W, H, ox, oy, index, params, plate_code, mask, low, high, window, code,
                         diff, evidence, stats, stream);
}

int fotg_upsample_crop_subtract(fotg_ctx *ctx, int n, const float *coarse_flows, const float *frames, int channels, int P,
                                const float *plate, int W, int H, int ox, int oy, const int *index, const unsigned char *plate_code,
                                const unsigned char *mask, float low, float high, int window, unsigned char *code, short *diff,
                                float *evidence, long long *stats, void *stream)
{
  return subtract_fused(ctx, n, coarse_flows, frames, channels, P, plate, W, H, ox, oy, index, plate_code, mask, low, high, window, code,
                        diff, evidence, stats, stream);
}

int fotg_upsample_crop_subtract_u8(fotg_ctx *ctx, int n, const float *coarse_flows, const unsigned char *frames, int channels, int P,
                                   const unsigned char *plate, int W, int H, int ox, int oy, const int *index,
                                   const unsigned char *plate_code, const unsigned char *mask, float low, float high, int window,
                                   unsigned char *code, short *diff, float *evidence, long long *stats, void *stream)
{
  return subtract_fused(ctx, n, coarse_flows, frames, channels, P, plate, W, H, ox, oy, index, plate_code, mask, low, high, window, code,
                        diff, evidence, stats, stream);
}

}  // extern "C"
