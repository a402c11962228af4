// include/fotg/blockmotion.h -- block motion vectors from a dense flow, for a video encoder, over the C-ABI of libfotg.so
// (fotg_block_motion / fotg_upsample_crop_block_motion): one quarter-pel vector per 8 x 8, 16 x 16 or 32 x 32 block of cur, chosen
// among the vectors the flow proposes for the block by the SAD of its prediction from ref, optionally refined by full-, half- and
// quarter-pel steps.  All pointers are device pointers.  Asynchronous on `stream` (a hipStream_t, 0 = the null stream); each call
// returns a FOTG_* status.  The definition, all of it integer arithmetic, is in include/fotg.h.
// Stream-ordered memory: a second call on a stream whose earlier call is still pending may wait on the host (include/fotg.h,
// STREAM-ORDERED MEMORY); the first returns at once.
#ifndef FOTG_BLOCKMOTION_HEADER
#define FOTG_BLOCKMOTION_HEADER
#include "../fotg.h"

namespace OFC {

enum { BLOCKMOTION_MAX_REFINE = 3, BLOCKMOTION_MAX_DIM = 16384 };
// kind: per block the winning candidate, | BLOCKMOTION_MOVED if a refinement step moved the vector
enum BlockMotionKind { BLOCKMOTION_ZERO = 0, BLOCKMOTION_MEAN = 1, BLOCKMOTION_CENTRE = 2, BLOCKMOTION_TOP_LEFT = 3,
                       BLOCKMOTION_TOP_RIGHT = 4, BLOCKMOTION_BOTTOM_LEFT = 5, BLOCKMOTION_BOTTOM_RIGHT = 6, BLOCKMOTION_MOVED = 8 };
// stats: per image eleven 64-bit integers; BLOCKMOTION_N_WON + k counts the blocks candidate k won
enum BlockMotionStat { BLOCKMOTION_SAD = 0, BLOCKMOTION_SAD_ZERO = 1, BLOCKMOTION_SSE = 2, BLOCKMOTION_N_MOVED = 3,
                       BLOCKMOTION_N_WON = 4, BLOCKMOTION_NSTAT = 11 };

inline bool BlockMotionValidBlock(int block) { return block == 8 || block == 16 || block == 32; }
// the block grid of a width x height frame
inline void BlockMotionGrid(int width, int height, int block, int &bw, int &bh)
{
  bw = (width + block - 1) / block; bh = (height + block - 1) / block;
}

// cur, ref: n x height x width x channels 8-bit, channels 1 or 3; flow: n x height x width x 2 float32 from cur to ref.  mv (n x bh x
// bw x 2 int16, quarter pixels), cost (n x bh x bw x 2 uint32: SAD of mv, SAD of the zero vector), kind (n x bh x bw uint8): outputs.
// pred (like cur, not overlapping cur or ref), stats (n x 11 int64) and mask (n x height x width uint8, a mask of FbCheck) may be
// NULL.
inline int BlockMotion(const unsigned char *cur, const unsigned char *ref, const float *flow, int width, int height, int channels,
                       int n, short *mv, unsigned *cost, unsigned char *kind, unsigned char *pred = nullptr,
                       long long *stats = nullptr, const unsigned char *mask = nullptr, int block = 16, int refine = 2, int device = 0,
                       void *stream = nullptr)
{
  return fotg_block_motion(device, n, cur, ref, width, height, channels, flow, mask, block, refine, mv, cost, kind, pred, stats,
                           stream);
}

// the same on a context's coarse flow (n of fotg_out_size, n <= max_batch), upsampled and cropped on the fly: frames, mask and pred
// at the original frame size; the full-resolution flow is never written
inline int UpsampleCropBlockMotion(fotg_ctx *ctx, const float *coarse_flow, const unsigned char *cur, const unsigned char *ref,
                                   int channels, int n, short *mv, unsigned *cost, unsigned char *kind,
                                   unsigned char *pred = nullptr, long long *stats = nullptr, const unsigned char *mask = nullptr,
                                   int block = 16, int refine = 2, void *stream = nullptr)
{
  return fotg_upsample_crop_block_motion(ctx, n, coarse_flow, cur, ref, channels, mask, block, refine, mv, cost, kind, pred, stats,
                                         stream);
}

}  // namespace OFC
#endif
