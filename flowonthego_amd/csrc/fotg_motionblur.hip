// fotg_motionblur.hip -- C-ABI of the motion blur along a flow (include/fotg.h fotg_motion_blur / fotg_upsample_crop_motion_blur),
// kernels in motionblur.hip.h.  Per call: pass A (half-vectors and tile maxima into stream-ordered memory of the call), pass B (the
// gather) and, when statistics are asked for, a small launch that folds the per-tile partials.  Everything is enqueued on the
// caller's stream; no host synchronisation.
#include "host_call.h"
#include "motionblur.hip.h"

using namespace fotg;

namespace {

bool aligned(const void *p, size_t a) { return (reinterpret_cast<size_t>(p) & (a - 1)) == 0; }

template <class T>
void gather(dim3 grid, hipStream_t stream, int channels, const void *src, const unsigned *H, const unsigned *tilemax, int w, int h, int vec,
            void *dst, unsigned char *code, int *part)
{
  if (channels == 1)
    mblur_gather_kernel<T, 1><<<grid, MB_THREADS, 0, stream>>>((const T *)src, H, tilemax, w, h, vec, (T *)dst, code, part);
  else
    mblur_gather_kernel<T, 3><<<grid, MB_THREADS, 0, stream>>>((const T *)src, H, tilemax, w, h, vec, (T *)dst, code, part);
}

// flow_mem: the flow's memory, flow_bytes long; dense: pass A reads it with 16-byte loads
template <class Src>
int blur_batch(int device, int n, const Src &flow, const void *flow_mem, size_t flow_bytes, bool dense, const void *src, int type, int channels,
               int w, int h, const unsigned char *mask, int shutter256, int max_blur, void *dst, unsigned char *code, short *vectors,
               long long *stats, void *stream_)
{
  if (n < 1 || n > 65535 || w < 1 || h < 1 || w > MB_MAX_DIM || h > MB_MAX_DIM) return FOTG_ERR_ARG;
  if ((type != FOTG_BLUR_U8 && type != FOTG_BLUR_F32) || (channels != 1 && channels != 3)) return FOTG_ERR_ARG;
  if (shutter256 < 1 || shutter256 > MB_MAX_SHUTTER256 || max_blur < 1 || max_blur > MB_MAX_BLUR) return FOTG_ERR_ARG;
  if (!src || !flow_mem || !dst) return FOTG_ERR_ARG;
  const size_t px = (size_t)n * w * h, fbytes = px * channels * (type == FOTG_BLUR_F32 ? sizeof(float) : 1);
  const Span out[4] = {{dst, fbytes}, {code, px}, {vectors, px * 2 * sizeof(short)}, {stats, (size_t)n * MB_NSTAT * sizeof(long long)}};
  const Span in[3] = {{src, fbytes}, {flow_mem, flow_bytes}, {mask, px}};
  if (overlap_any(out, in) || overlap_among(out)) return FOTG_ERR_ARG;
  DevGuard guard(device);
  if (!guard.ok) return hip_fail(guard.err);
  hipStream_t stream = (hipStream_t)stream_;
  const int tw = (w + MB_TILE - 1) / MB_TILE, th = (h + MB_TILE - 1) / MB_TILE;
  const size_t tiles = (size_t)tw * th;
  unsigned *H = nullptr, *tilemax = nullptr;
  int *part = nullptr;
  Scratch mem(stream);
  if (!mem.get(&H, px * sizeof(unsigned)) || !mem.get(&tilemax, (size_t)n * tiles * sizeof(unsigned)) ||
      (stats && !mem.get(&part, (size_t)n * tiles * MB_NSTAT * sizeof(int))))
    return mem.finish(mem.err);
  const int vec = (dense && aligned(flow_mem, 16) ? 1 : 0) | (mask && aligned(mask, 4) ? 2 : 0) | (vectors && aligned(vectors, 8) ? 4 : 0) |
                  (aligned(src, 16) && aligned(dst, 16) ? 8 : 0);
  const dim3 grid((unsigned)tw, (unsigned)th, (unsigned)n);
  mblur_vectors_kernel<Src><<<grid, MB_THREADS, 0, stream>>>(flow, mask, w, h, (float)shutter256 / 32.f, 16 * max_blur, vec, H,
                                                             reinterpret_cast<unsigned *>(vectors), tilemax);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) {
    if (type == FOTG_BLUR_F32) gather<float>(grid, stream, channels, src, H, tilemax, w, h, vec, dst, code, part);
    else gather<unsigned char>(grid, stream, channels, src, H, tilemax, w, h, vec, dst, code, part);
    e = hipGetLastError();
  }
  if (stats && e == hipSuccess) {
    mblur_fold_kernel<<<dim3((unsigned)n), MB_THREADS, 0, stream>>>(part, (int)tiles, stats);
    e = hipGetLastError();
  }
  return mem.finish(e);
}

}  // namespace

extern "C" {

int fotg_motion_blur(int device, int n, const void *src, int type, int channels, const float *flow, int w, int h, const unsigned char *mask,
                     int shutter256, int max_blur, void *dst, unsigned char *code, short *vectors, long long *stats, void *stream)
{
  const size_t fbytes = (n > 0 && w > 0 && h > 0) ? (size_t)n * w * h * 2 * sizeof(float) : 0;
  return blur_batch(device, n, DenseSrc{flow}, flow, fbytes, true, src, type, channels, w, h, mask, shutter256, max_blur, dst, code, vectors,
                    stats, stream);
}

int fotg_upsample_crop_motion_blur(fotg_ctx *ctx, int n, const void *src, int type, int channels, const float *coarse_flow,
                                   const unsigned char *mask, int shutter256, int max_blur, void *dst, unsigned char *code, short *vectors,
                                   long long *stats, void *stream)
{
  CtxUpsampleGeom g;
  if (!fused_geom(ctx, n, coarse_flow, &g)) return FOTG_ERR_ARG;
  return blur_batch(g.device, n, upsample_src(g, coarse_flow), coarse_flow, (size_t)n * g.wl * g.hl * 2 * sizeof(float), false, src, type,
                    channels, g.w_org, g.h_org, mask, shutter256, max_blur, dst, code, vectors, stats, stream);
}

}  // extern "C"
