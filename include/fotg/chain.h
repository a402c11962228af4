// include/fotg/chain.h -- flow chaining over the C-ABI of libfotg.so (fotg_flow_chain / fotg_track_points and their fused forms): a
// pixel or a point followed through the T flows of a sequence, with a code per chain (0 valid to the end, 1 occluded, 2 leaves the
// frame, 3 unknown: the alphabet of include/fotg/fbcheck.h) and the number of steps it was followed.  Device pointers throughout,
// asynchronous on `stream` (a hipStream_t, 0 = the null stream); each call returns a FOTG_* status.  The definition is in
// include/fotg.h.
#ifndef FOTG_CHAIN_HEADER
#define FOTG_CHAIN_HEADER
#include "../fotg.h"

namespace OFC {

// stats: per sequence five unsigned 64-bit integers
enum ChainStat { CHAIN_VALID = 0, CHAIN_OCCLUDED = 1, CHAIN_OUTSIDE = 2, CHAIN_UNKNOWN = 3, CHAIN_SUM_STEPS = 4 };

// flows (frame k -> k+1), flows_bw (frame k+1 -> k, or nullptr: no occlusion test): n_seq x T x height x width x 2 float32.
// total n_seq x height x width x 2 float32, code uint8, steps int32, stats n_seq x 5: each may be nullptr, not all.
inline int FlowChain(const float *flows, const float *flows_bw, int T, int width, int height, float *total,
                     unsigned char *code = nullptr, int *steps = nullptr, unsigned long long *stats = nullptr, float alpha1 = 0.01f,
                     float alpha2 = 0.5f, int n_seq = 1, int device = 0, void *stream = nullptr)
{
  return fotg_flow_chain(device, n_seq, T, flows, flows_bw, width, height, alpha1, alpha2, total, code, steps, stats, stream);
}

// pts n_seq x P x 2 (x, y); traj n_seq x (T+1) x P x 2: the position in every frame
inline int TrackPoints(const float *flows, const float *flows_bw, int T, int width, int height, int P, const float *pts, float *traj,
                       unsigned char *code = nullptr, int *steps = nullptr, unsigned long long *stats = nullptr, float alpha1 = 0.01f,
                       float alpha2 = 0.5f, int n_seq = 1, int device = 0, void *stream = nullptr)
{
  return fotg_track_points(device, n_seq, T, flows, flows_bw, width, height, alpha1, alpha2, P, pts, traj, code, steps, stats, stream);
}

// the same along T coarse flows of a context (the outflows of fotg_calc_sequence / fotg_calc_sequence_bidir), upsampled and cropped
// on the fly: one sequence of frames at the original size
inline int UpsampleCropFlowChain(fotg_ctx *ctx, int T, const float *coarse_flows, const float *coarse_bw, float *total,
                                 unsigned char *code = nullptr, int *steps = nullptr, unsigned long long *stats = nullptr,
                                 float alpha1 = 0.01f, float alpha2 = 0.5f, void *stream = nullptr)
{
  return fotg_upsample_crop_flow_chain(ctx, T, coarse_flows, coarse_bw, alpha1, alpha2, total, code, steps, stats, stream);
}

inline int UpsampleCropTrackPoints(fotg_ctx *ctx, int T, const float *coarse_flows, const float *coarse_bw, int P, const float *pts,
                                   float *traj, unsigned char *code = nullptr, int *steps = nullptr, unsigned long long *stats = nullptr,
                                   float alpha1 = 0.01f, float alpha2 = 0.5f, void *stream = nullptr)
{
  return fotg_upsample_crop_track_points(ctx, T, coarse_flows, coarse_bw, alpha1, alpha2, P, pts, traj, code, steps, stats, stream);
}

}  // namespace OFC
#endif
