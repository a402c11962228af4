// include/fotg/fill.h -- hole filling by pull-push over the C-ABI of libfotg.so (fotg_fill, fotg_fill_u8, fotg_fill_scratch): the
// unknown pixels of frames and flows filled from the known ones, at any hole size.  src, hole and the outputs are device pointers.
// Asynchronous on `stream` (a hipStream_t, 0 = the null stream); each call returns a FOTG_* status.  The definition is in
// include/fotg.h.
// Stream-ordered memory: a second call on a stream whose earlier call is still pending may wait on the host (include/fotg.h,
// STREAM-ORDERED MEMORY); the first returns at once.
#ifndef FOTG_FILL_HEADER
#define FOTG_FILL_HEADER
#include "../fotg.h"

namespace OFC {

enum { FILL_MAX_DIM = 16384, FILL_MAX_IMAGES = 65535 };
// code: per pixel
enum FillCode { FILL_KNOWN = 0, FILL_FILLED = 1, FILL_UNFILLED = 2 };
// stats: per image four 64-bit integers
enum FillStat { FILL_N_KNOWN = 0, FILL_N_FILLED = 1, FILL_N_UNFILLED = 2, FILL_DEPTH = 3, FILL_STATS = 4 };
// fg_codes: 0 = every non-zero byte of hole is a hole; otherwise bit c set = the byte value c (0 .. 7) is a hole, as for LabelComponents
enum { FILL_FG_NONZERO = 0 };

// src: n x height x width x channels float (channels 1 .. 3); hole: n x height x width uint8 or null -- a pixel that is not finite or
// beyond +-32768 is a hole as well; dst as src, code: n x height x width uint8, stats: n x 4 long long; each may be left out, not all
inline int FillHoles(const float *src, int n, int width, int height, int channels, const unsigned char *hole, float *dst,
                     unsigned char *code = nullptr, long long *stats = nullptr, int fg_codes = FILL_FG_NONZERO, int device = 0,
                     void *stream = nullptr)
{
  return fotg_fill(device, n, src, width, height, channels, hole, fg_codes, dst, code, stats, stream);
}

// the same on 8-bit frames (channels 1 or 3); hole is needed
inline int FillHoles(const unsigned char *src, int n, int width, int height, int channels, const unsigned char *hole, unsigned char *dst,
                     unsigned char *code = nullptr, long long *stats = nullptr, int fg_codes = FILL_FG_NONZERO, int device = 0,
                     void *stream = nullptr)
{
  return fotg_fill_u8(device, n, src, width, height, channels, hole, fg_codes, dst, code, stats, stream);
}

// a flow with rejected (mask != 0, fb_check's map, or null) and unknown (1e9, not finite) vectors made dense
inline int FillFlow(const float *flow, int n, int width, int height, const unsigned char *mask, float *dst, int device = 0,
                    void *stream = nullptr)
{
  return fotg_fill(device, n, flow, width, height, 2, mask, FILL_FG_NONZERO, dst, nullptr, nullptr, stream);
}

// the stream-ordered memory a call takes, in bytes (host only); -1: arguments out of range
inline long long FillScratchBytes(int n, int width, int height, int channels)
{
  long long bytes = -1;
  return fotg_fill_scratch(n, width, height, channels, &bytes) == FOTG_OK ? bytes : -1;
}

}  // namespace OFC
#endif
