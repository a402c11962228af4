// include/fotg/morph.h -- binary morphology of masks and code maps over the C-ABI of libfotg.so (fotg_morph): erode, dilate, open
// and close by a disc, and the cleaning of a mask by an opening and a closing.  src and the outputs are device pointers.
// Asynchronous on `stream` (a hipStream_t, 0 = the null stream); each call returns a FOTG_* status.  The definition is in
// include/fotg.h.
#ifndef FOTG_MORPH_HEADER
#define FOTG_MORPH_HEADER
#include "../fotg.h"

namespace OFC {

enum { MORPH_MAX_DIM = 16384, MORPH_MAX_RADIUS = 8 };
// a stage of a chain
enum MorphStage { MORPH_ERODE = 0, MORPH_DILATE = 1 };
// the four operations of Morphology()
enum MorphOp { MORPH_OP_ERODE = 0, MORPH_OP_DILATE = 1, MORPH_OP_OPEN = 2, MORPH_OP_CLOSE = 3 };
// stats: per map four 64-bit integers
enum MorphStat { MORPH_N_BEFORE = 0, MORPH_N_AFTER = 1, MORPH_N_ADDED = 2, MORPH_N_REMOVED = 3, MORPH_STATS = 4 };
// fg_codes: 0 = every non-zero byte is set; otherwise bit c set = the byte value c (0 .. 7) is set, as for LabelComponents
enum { MORPH_FG_NONZERO = 0 };

// src: n x height x width uint8; a chain of one or two stages (MorphStage) with a radius 0 .. 8 each, in one launch; out:
// n x height x width uint8, 0 or 1, and stats: n x 4 long long, either may be left out
inline int MorphChain(const unsigned char *src, int n, int width, int height, int nstage, const int *stages, const int *radii,
                      unsigned char *out, long long *stats = nullptr, int fg_codes = MORPH_FG_NONZERO, int device = 0, void *stream = nullptr)
{
  return fotg_morph(device, n, src, width, height, fg_codes, nstage, stages, radii, out, stats, stream);
}

// erode, dilate, open (erode, then dilate) or close (dilate, then erode) by the disc of `radius`: one launch
inline int Morphology(const unsigned char *src, int n, int width, int height, MorphOp op, int radius, unsigned char *out,
                      long long *stats = nullptr, int fg_codes = MORPH_FG_NONZERO, int device = 0, void *stream = nullptr)
{
  const int first = (op == MORPH_OP_ERODE || op == MORPH_OP_OPEN) ? MORPH_ERODE : MORPH_DILATE;
  const int stages[2] = {first, first == MORPH_ERODE ? MORPH_DILATE : MORPH_ERODE}, radii[2] = {radius, radius};
  return MorphChain(src, n, width, height, (op == MORPH_OP_OPEN || op == MORPH_OP_CLOSE) ? 2 : 1, stages, radii, out, stats, fg_codes, device,
                    stream);
}

// the opening by `open` and then the closing by `close`, a launch each; tmp: n x height x width bytes for the opened map (it may
// overlaps neither src nor out); stats: 2 x n x 4 long long or null, the opening's table and then the closing's
inline int CleanMask(const unsigned char *src, int n, int width, int height, int open, int close, unsigned char *tmp, unsigned char *out,
                     long long *stats = nullptr, int fg_codes = MORPH_FG_NONZERO, int device = 0, void *stream = nullptr)
{
  const int st = Morphology(src, n, width, height, MORPH_OP_OPEN, open, tmp, stats, fg_codes, device, stream);
  if (st != FOTG_OK) return st;
  return Morphology(tmp, n, width, height, MORPH_OP_CLOSE, close, out, stats ? stats + (long long)n * MORPH_STATS : nullptr, MORPH_FG_NONZERO,
                    device, stream);
}

}  // namespace OFC
#endif
