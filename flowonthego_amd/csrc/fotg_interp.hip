// fotg_interp.hip -- C-ABI of the frame interpolation (include/fotg.h fotg_interp / fotg_upsample_crop_interp and their 8-bit
// forms), kernels in interp.hip.h.  Per call and chunk of images: the consistency check when the caller gave no masks, a memset
// of the key planes to all ones, the candidate launch (both directions), the resolve launch and, when statistics are asked for,
// warp_fold_kernel.  Key planes, masks of the call's own check and partial sums live in stream-ordered memory of the call.
// The key planes take 16 bytes per pixel and image (two directions of 64-bit keys): the batch is processed in chunks of as many
// images as fit INTERP_KEY_BYTES (256 MiB; one image when a single one is larger), so a 64 x 1080p call holds 8 images' planes
// at a time instead of 2.1 GB.  Asynchronous on the caller's stream; no host synchronisation.
#include "host_call.h"
#include "fbcheck.hip.h"
#include "interp.hip.h"

using namespace fotg;

namespace {

const size_t INTERP_KEY_BYTES = (size_t)256 << 20;

// the source of the images first, first + 1, ... of a batch
DenseSrc from_image(const DenseSrc &s, long first, long hw) { return DenseSrc{s.flow + 2 * first * hw}; }
UpsampleSrc from_image(UpsampleSrc s, long first, long) { s.flow += first * s.in_stride; return s; }

template <class Src, class T, int NOC>
hipError_t launch_chunk(int n, const Src &fw, const Src &bw, const T *I0, const T *I1, const unsigned char *mF, const unsigned char *mB,
                        interp_key *keys, const T *ref, int w, int h, float t, T *dst, unsigned char *code, WarpPartial *part,
                        unsigned blocks, hipStream_t stream)
{
  hipError_t e = hipMemsetAsync(keys, 0xff, (size_t)n * 2 * (size_t)w * h * sizeof(interp_key), stream);
  if (e != hipSuccess) return e;
  interp_candidate_kernel<Src, T, NOC><<<dim3(blocks, (unsigned)n, 2), WARP_THREADS, 0, stream>>>(fw, bw, I0, I1, mF, mB, w, h, t, keys);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  interp_resolve_kernel<Src, T, NOC><<<dim3(blocks, (unsigned)n), WARP_THREADS, 0, stream>>>(fw, bw, I0, I1, mF, mB, keys, ref, w, h, t,
                                                                                           dst, code, part);
  return hipGetLastError();
}

template <class Src, class T>
int interp_batch(int device, int n, const Src &fw, const Src &bw, const T *I0, const T *I1, int w, int h, int channels, float t,
                 const unsigned char *mask_fw, const unsigned char *mask_bw, float alpha1, float alpha2, const T *ref, T *dst,
                 unsigned char *code, double *stats, void *stream_)
{
  if (n < 1 || !I0 || !I1 || w <= 0 || h <= 0 || (channels != 1 && channels != 3) || !(t > 0.f && t < 1.f)) return FOTG_ERR_ARG;
  if ((!dst && !code && !stats) || (mask_fw == nullptr) != (mask_bw == nullptr)) return FOTG_ERR_ARG;
  const long hw = (long)w * h;
  if (hw > 0xffffffffL || n > 65535) return FOTG_ERR_ARG;          // the key holds the source index in 32 bits
  const long blocks = ((hw + 3) / 4 + WARP_THREADS - 1) / WARP_THREADS;
  const size_t bytes = (size_t)n * hw * channels * sizeof(T);
  const Span out[1] = {{dst, bytes}}, in[2] = {{I0, bytes}, {I1, bytes}};
  if (overlap_any(out, in)) return FOTG_ERR_ARG;      // the taps of a pixel are read after other pixels have been written: not in place
  DevGuard guard(device);
  if (!guard.ok) return hip_fail(guard.err);
  hipStream_t stream = (hipStream_t)stream_;
  long chunk = (long)(INTERP_KEY_BYTES / ((size_t)hw * 2 * sizeof(interp_key)));
  chunk = chunk < 1 ? 1 : (chunk > n ? n : chunk);
  interp_key *keys = nullptr;
  unsigned char *own_masks = nullptr;
  WarpPartial *part = nullptr;
  Scratch mem(stream);
  mem.get(&keys, (size_t)chunk * 2 * hw * sizeof(interp_key));
  if (!mask_fw) mem.get(&own_masks, (size_t)chunk * 2 * hw);
  if (stats) mem.get(&part, (size_t)n * blocks * sizeof(WarpPartial));
  hipError_t e = mem.err;
  for (long first = 0; e == hipSuccess && first < n; first += chunk) {
    const int m = (int)(n - first < chunk ? n - first : chunk);
    const Src f = from_image(fw, first, hw), b = from_image(bw, first, hw);
    const unsigned char *mF = mask_fw ? mask_fw + first * hw : own_masks, *mB = mask_bw ? mask_bw + first * hw : own_masks + (size_t)m * hw;
    if (!mask_fw) {
      fb_check_kernel<Src><<<dim3((unsigned)blocks, (unsigned)m, 2), 256, 0, stream>>>(f, b, w, h, alpha1, alpha2, own_masks,
                                                                                     own_masks + (size_t)m * hw, nullptr);
      if ((e = hipGetLastError()) != hipSuccess) break;
    }
    const size_t img = (size_t)first * hw * channels;
    const T *r = ref ? ref + img : nullptr;
    T *d = dst ? dst + img : nullptr;
    unsigned char *c = code ? code + first * hw : nullptr;
    WarpPartial *p = part ? part + first * blocks : nullptr;
    e = channels == 1 ? launch_chunk<Src, T, 1>(m, f, b, I0 + img, I1 + img, mF, mB, keys, r, w, h, t, d, c, p, (unsigned)blocks, stream)
                      : launch_chunk<Src, T, 3>(m, f, b, I0 + img, I1 + img, mF, mB, keys, r, w, h, t, d, c, p, (unsigned)blocks, stream);
  }
  if (e == hipSuccess && stats) e = warp_fold(part, (int)blocks, n, stats, stream);
  return mem.finish(e);
}

template <class T>
int interp_dense(int device, int n, const T *I0, const T *I1, const float *flow_fw, const float *flow_bw, int w, int h, int channels,
                 float t, const unsigned char *mask_fw, const unsigned char *mask_bw, float alpha1, float alpha2, const T *ref, T *dst,
                 unsigned char *code, double *stats, void *stream)
{
  if (!flow_fw || !flow_bw) return FOTG_ERR_ARG;
  return interp_batch(device, n, DenseSrc{flow_fw}, DenseSrc{flow_bw}, I0, I1, w, h, channels, t, mask_fw, mask_bw, alpha1, alpha2, ref,
                      dst, code, stats, stream);
}

template <class T>
int interp_fused(fotg_ctx *ctx, int n, const float *flow_fw, const float *flow_bw, const T *I0, const T *I1, int channels, float t,
                 const unsigned char *mask_fw, const unsigned char *mask_bw, float alpha1, float alpha2, const T *ref, T *dst,
                 unsigned char *code, double *stats, void *stream)
{
  CtxUpsampleGeom g;
  if (!ctx || !flow_fw || !flow_bw || ctx_upsample_geom(ctx, &g) != FOTG_OK) return FOTG_ERR_ARG;
  if (!g.bidir) return FOTG_ERR_UNSUPPORTED;
  if (n < 1 || n > g.max_batch || g.nch != 2) return FOTG_ERR_ARG;
  return interp_batch(g.device, n, upsample_src(g, flow_fw), upsample_src(g, flow_bw), I0, I1, g.w_org, g.h_org, channels, t, mask_fw,
                      mask_bw, alpha1, alpha2, ref, dst, code, stats, stream);
}

}  // namespace

extern "C" {

int fotg_interp(int device, int n, const float *I0, const float *I1, const float *flow_fw, const float *flow_bw, int w, int h,
                int channels, float t, const unsigned char *mask_fw, const unsigned char *mask_bw, float alpha1, float alpha2,
                const float *ref, float *dst, unsigned char *code, double *stats, void *stream)
{
  return interp_dense(device, n, I0, I1, flow_fw, flow_bw, w, h, channels, t, mask_fw, mask_bw, alpha1, alpha2, ref, dst, code, stats, stream);
}

int fotg_interp_u8(int device, int n, const unsigned char *I0, const unsigned char *I1, const float *flow_fw, const float *flow_bw,
                   int w, int h, int channels, float t, const unsigned char *mask_fw, const unsigned char *mask_bw, float alpha1,
                   float alpha2, const unsigned char *ref, unsigned char *dst, unsigned char *code, double *stats, void *stream)
{
  return interp_dense(device, n, I0, I1, flow_fw, flow_bw, w, h, channels, t, mask_fw, mask_bw, alpha1, alpha2, ref, dst, code, stats, stream);
}

int fotg_upsample_crop_interp(fotg_ctx *ctx, int n, const float *coarse_fw, const float *coarse_bw, const float *I0, const float *I1,
                              int channels, float t, const unsigned char *mask_fw, const unsigned char *mask_bw, float alpha1,
                              float alpha2, const float *ref, float *dst, unsigned char *code, double *stats, void *stream)
{
  return interp_fused(ctx, n, coarse_fw, coarse_bw, I0, I1, channels, t, mask_fw, mask_bw, alpha1, alpha2, ref, dst, code, stats, stream);
}

int fotg_upsample_crop_interp_u8(fotg_ctx *ctx, int n, const float *coarse_fw, const float *coarse_bw, const unsigned char *I0,
                                 const unsigned char *I1, int channels, float t, const unsigned char *mask_fw,
                                 const unsigned char *mask_bw, float alpha1, float alpha2, const unsigned char *ref, unsigned char *dst,
                                 unsigned char *code, double *stats, void *stream)
{
  return interp_fused(ctx, n, coarse_fw, coarse_bw, I0, I1, channels, t, mask_fw, mask_bw, alpha1, alpha2, ref, dst, code, stats, stream);
}

}  // extern "C"
