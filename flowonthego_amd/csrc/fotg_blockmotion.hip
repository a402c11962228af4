// fotg_blockmotion.hip -- C-ABI of the block motion vectors (include/fotg.h fotg_block_motion / fotg_upsample_crop_block_motion),
// kernels in blockmotion.hip.h.  Per call: one launch and, when statistics are asked for, a second small launch that folds the
// per-block figures (the squared errors travel through stream-ordered memory of the call).  Everything is enqueued on the caller's
// stream.
#include "host_call.h"
#include "blockmotion.hip.h"

using namespace fotg;

namespace {

template <class Src, int NOC, int B>
hipError_t launch(const dim3 &grid, hipStream_t stream, const Src &flow, const unsigned char *cur, const unsigned char *ref,
                  const unsigned char *mask, int w, int h, int bw, int bh, int refine, short *mv, unsigned *cost, unsigned char *kind,
                  unsigned char *pred, unsigned *sse)
{
  blockmv_kernel<Src, NOC, B><<<grid, BM_THREADS, 0, stream>>>(flow, cur, ref, mask, w, h, bw, bh, refine, mv, cost, kind, pred, sse);
  return hipGetLastError();
}

template <class Src, int NOC, class... A>
hipError_t launch_block(int block, A... a)
{
  if (block == 8) return launch<Src, NOC, 8>(a...);
  if (block == 16) return launch<Src, NOC, 16>(a...);
  return launch<Src, NOC, 32>(a...);
}

template <class Src>
int block_motion_batch(int device, int n, const Src &flow, const void *flow_mem, const unsigned char *cur, const unsigned char *ref,
                       int w, int h, int channels, const unsigned char *mask, int block, int refine, short *mv, unsigned *cost,
                       unsigned char *kind, unsigned char *pred, long long *stats, void *stream_)
{
  if (n < 1 || n > 65535 || w < 1 || h < 1 || w > BM_MAX_DIM || h > BM_MAX_DIM || (channels != 1 && channels != 3)) return FOTG_ERR_ARG;
  if ((block != 8 && block != 16 && block != 32) || refine < 0 || refine > 3) return FOTG_ERR_ARG;
  if (!flow_mem || !cur || !ref || !mv || !cost || !kind) return FOTG_ERR_ARG;
  const size_t fbytes = (size_t)n * w * h * channels;
  const Span out[1] = {{pred, fbytes}}, in[2] = {{cur, fbytes}, {ref, fbytes}};
  if (overlap_any(out, in)) return FOTG_ERR_ARG;                                     // other blocks read them
  const int bw = (w + block - 1) / block, bh = (h + block - 1) / block, nblk = bw * bh;
  DevGuard guard(device);
  if (!guard.ok) return hip_fail(guard.err);
  hipStream_t stream = (hipStream_t)stream_;
  unsigned *sse = nullptr;
  Scratch mem(stream);
  if (stats) mem.get(&sse, (size_t)n * nblk * sizeof(unsigned));
  hipError_t e = mem.err;
  if (e == hipSuccess) {
    const dim3 grid((unsigned)((nblk + BM_WAVES - 1) / BM_WAVES), (unsigned)n);
    if (channels == 1)
      e = launch_block<Src, 1>(block, grid, stream, flow, cur, ref, mask, w, h, bw, bh, refine, mv, cost, kind, pred, sse);
    else
      e = launch_block<Src, 3>(block, grid, stream, flow, cur, ref, mask, w, h, bw, bh, refine, mv, cost, kind, pred, sse);
  }
  if (stats && e == hipSuccess) {
    blockmv_fold_kernel<<<dim3((unsigned)n), BM_THREADS, 0, stream>>>(cost, kind, sse, nblk, stats);
    e = hipGetLastError();
  }
  return mem.finish(e);
}

}  // namespace

extern "C" {

int fotg_block_motion(int device, int n, const unsigned char *cur, const unsigned char *ref, int w, int h, int channels,
                      const float *flow, const unsigned char *mask, int block, int refine, short *mv, unsigned *cost,
                      unsigned char *kind, unsigned char *pred, long long *stats, void *stream)
{
  return block_motion_batch(device, n, DenseSrc{flow}, flow, cur, ref, w, h, channels, mask, block, refine, mv, cost, kind, pred,
                            stats, stream);
}

int fotg_upsample_crop_block_motion(fotg_ctx *ctx, int n, const float *coarse_flow, const unsigned char *cur, const unsigned char *ref,
                                    int channels, const unsigned char *mask, int block, int refine, short *mv, unsigned *cost,
                                    unsigned char *kind, unsigned char *pred, long long *stats, void *stream)
{
  CtxUpsampleGeom g;
  if (!fused_geom(ctx, n, coarse_flow, &g)) return FOTG_ERR_ARG;
  return block_motion_batch(g.device, n, upsample_src(g, coarse_flow), coarse_flow, cur, ref, g.w_org, g.h_org, channels, mask, block,
                            refine, mv, cost, kind, pred, stats, stream);
}

}  // extern "C"
