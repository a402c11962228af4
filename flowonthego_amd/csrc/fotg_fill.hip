// fotg_fill.hip -- C-ABI of the pull-push hole filling (include/fotg.h fotg_fill), kernels in fill.hip.h, level geometry in
// fill_levels.h.  Per call: a stream-ordered memset of stats, one stream-ordered allocation, and per chunk of images three launches
// (pull, top, push).  The allocation holds fill_chunk images' levels -- at most max(one image's, 1 GiB) -- and the chunks of a larger
// batch follow each other through it on the stream.  Everything is enqueued on the caller's stream; nothing synchronises.
#include "host_call.h"
#include "fill.hip.h"

using namespace fotg;

namespace {

template <typename T, int CH>
hipError_t fill_chunk_launch(int m, const T *src, const unsigned char *hole, unsigned fg, const FillLevels &g, unsigned char *scratch, T *dst,
                             unsigned char *code, long long *stats, hipStream_t stream)
{
  const dim3 grid((unsigned)g.tw, (unsigned)g.th, (unsigned)m);
  fill_pull_kernel<T, CH><<<grid, FILL_THREADS, 0, stream>>>(src, hole, fg, g, scratch);
  fill_top_kernel<CH><<<dim3((unsigned)m), FILL_THREADS, 0, stream>>>(g, scratch);
  fill_push_kernel<T, CH><<<grid, FILL_THREADS, 0, stream>>>(src, hole, fg, g, scratch, dst, code, reinterpret_cast<unsigned long long *>(stats));
  return hipGetLastError();
}

template <typename T>
int fill_call(int device, int n, const T *src, int w, int h, int ch, bool ch_ok, const unsigned char *hole, bool hole_needed, int fg_codes, T *dst,
              unsigned char *code, long long *stats, void *stream_)
{
  if (n < 1 || n > FILL_MAX_N || w < 1 || h < 1 || w > FILL_MAX_DIM || h > FILL_MAX_DIM || !ch_ok) return FOTG_ERR_ARG;
  if (!src || (hole_needed && !hole) || fg_codes < 0 || fg_codes > 255 || (!dst && !code && !stats)) return FOTG_ERR_ARG;
  const size_t npx = (size_t)n * w * h;
  const Span outs[3] = {{dst, npx * ch * sizeof(T)}, {code, npx}, {stats, (size_t)n * FILL_NSTAT * sizeof(long long)}};
  const Span in[2] = {{src, npx * ch * sizeof(T)}, {hole, npx}};
  if (overlap_any(outs, in) || overlap_among(outs)) return FOTG_ERR_ARG;
  DevGuard guard(device);
  if (!guard.ok) return hip_fail(guard.err);
  hipStream_t stream = (hipStream_t)stream_;
  const FillLevels g = fill_levels(w, h, ch);
  const int chunk = fill_chunk(n, g.bytes);
  Scratch mem(stream);
  unsigned char *scratch = nullptr;
  if (!mem.get(&scratch, (size_t)g.bytes * chunk)) return mem.finish(mem.err);
  hipError_t e = hipSuccess;
  if (stats) e = hipMemsetAsync(stats, 0, (size_t)n * FILL_NSTAT * sizeof(long long), stream);
  const size_t ipx = (size_t)w * h;
  for (int i0 = 0; i0 < n && e == hipSuccess; i0 += chunk) {
    const int m = n - i0 < chunk ? n - i0 : chunk;
    const T *s = src + i0 * ipx * ch;
    const unsigned char *ho = hole ? hole + i0 * ipx : nullptr;
    T *d = dst ? dst + i0 * ipx * ch : nullptr;
    unsigned char *co = code ? code + i0 * ipx : nullptr;
    long long *st = stats ? stats + (size_t)i0 * FILL_NSTAT : nullptr;
    if (ch == 1) e = fill_chunk_launch<T, 1>(m, s, ho, (unsigned)fg_codes, g, scratch, d, co, st, stream);
    else if (ch == 3) e = fill_chunk_launch<T, 3>(m, s, ho, (unsigned)fg_codes, g, scratch, d, co, st, stream);
    else if constexpr (sizeof(T) == 4) e = fill_chunk_launch<T, 2>(m, s, ho, (unsigned)fg_codes, g, scratch, d, co, st, stream);
  }
  return mem.finish(e);
}

}  // namespace

extern "C" {

int fotg_fill(int device, int n, const float *src, int w, int h, int ch, const unsigned char *hole, int fg_codes, float *dst, unsigned char *code,
              long long *stats, void *stream)
{
  return fill_call<float>(device, n, src, w, h, ch, ch >= 1 && ch <= 3, hole, false, fg_codes, dst, code, stats, stream);
}

int fotg_fill_u8(int device, int n, const unsigned char *src, int w, int h, int ch, const unsigned char *hole, int fg_codes, unsigned char *dst,
                 unsigned char *code, long long *stats, void *stream)
{
  return fill_call<unsigned char>(device, n, src, w, h, ch, ch == 1 || ch == 3, hole, true, fg_codes, dst, code, stats, stream);
}

int fotg_fill_scratch(int n, int w, int h, int ch, long long *bytes)
{
  if (n < 1 || n > FILL_MAX_N || w < 1 || h < 1 || w > FILL_MAX_DIM || h > FILL_MAX_DIM || ch < 1 || ch > 3 || !bytes) return FOTG_ERR_ARG;
  *bytes = fill_scratch_bytes(n, w, h, ch);
  return FOTG_OK;
}

}  // extern "C"
