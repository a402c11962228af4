// fotg_morph.hip -- C-ABI of the binary morphology (include/fotg.h fotg_morph), kernel in morph.hip.h.  Per call: a stream-ordered
// memset of stats and one launch over every map, whatever the chain.  ops and radii are host arrays, consumed before the call
// returns.  Everything is enqueued on the caller's stream; nothing synchronises.
#include "host_call.h"
#include "morph.hip.h"

using namespace fotg;

namespace {

// the half-widths floor(sqrt(r^2 - dy^2)) of the disc's rows |dy| = 0 .. r, 4 bits each (integers only)
unsigned long long half_widths(int r)
{
  unsigned long long hw = 0;
  for (int dy = 0; dy <= r; ++dy) {
    int k = 0;
    while ((k + 1) * (k + 1) + dy * dy <= r * r) ++k;
    hw |= (unsigned long long)k << (4 * dy);
  }
  return hw;
}

}  // namespace

extern "C" {

int fotg_morph(int device, int n, const unsigned char *src, int w, int h, int fg_codes, int nstage, const int *ops, const int *radii,
               unsigned char *out, long long *stats, void *stream_)
{
  if (n < 1 || n > 65535 || w < 1 || h < 1 || w > MO_MAX_DIM || h > MO_MAX_DIM) return FOTG_ERR_ARG;
  if (!src || (!out && !stats) || fg_codes < 0 || fg_codes > 255) return FOTG_ERR_ARG;
  if ((nstage != 1 && nstage != 2) || !ops || !radii) return FOTG_ERR_ARG;
  int op[2] = {MO_DILATE, MO_DILATE}, r[2] = {0, 0};
  for (int k = 0; k < nstage; ++k) {
    op[k] = ops[k];
    r[k] = radii[k];
    if ((op[k] != MO_ERODE && op[k] != MO_DILATE) || r[k] < 0 || r[k] > MO_MAXR) return FOTG_ERR_ARG;
  }
  const size_t hw = (size_t)w * h;
  const Span outs[2] = {{out, n * hw}, {stats, (size_t)n * MO_NSTAT * sizeof(long long)}};
  const Span in[1] = {{src, n * hw}};
  if (overlap_any(outs, in) || overlap_among(outs)) return FOTG_ERR_ARG;
  DevGuard guard(device);
  if (!guard.ok) return hip_fail(guard.err);
  hipStream_t stream = (hipStream_t)stream_;
  hipError_t e = hipSuccess;
  if (stats) e = hipMemsetAsync(stats, 0, (size_t)n * MO_NSTAT * sizeof(long long), stream);
  if (e == hipSuccess) {
    const dim3 grid((unsigned)((w + MO_TW - 1) / MO_TW), (unsigned)((h + MO_TH - 1) / MO_TH), (unsigned)n);
    morph_kernel<<<grid, MO_THREADS, 0, stream>>>(src, w, h, (unsigned)fg_codes, nstage, op[0] == MO_ERODE, r[0], half_widths(r[0]),
                                                  op[1] == MO_ERODE, r[1], half_widths(r[1]), out,
                                                  reinterpret_cast<unsigned long long *>(stats));
    e = hipGetLastError();
  }
  return e == hipSuccess ? FOTG_OK : hip_fail(e);
}

}  // extern "C"
