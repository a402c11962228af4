// fill_levels.h -- the level geometry of the pull-push hole filling (fill.hip.h, fotg_fill.hip), in plain C++ (no HIP): the sizes of
// the levels, where each level lives in the stream-ordered memory of a call, and how much of that memory an image and a call take.
// tests/fill_levels_drv.cpp builds this header with g++ for tests/test_host_fill.py.
//
// Level l of a w x h image has ceil(w / 2^l) x ceil(h / 2^l) blocks (the recurrence w_{l+1} = (w_l + 1) >> 1 in closed form); L is
// the first level of one block.  A 64 x 64 tile of level 0 is one block of level 6, so level 6 has one block per tile.
// Per image, in this order, every part at a multiple of 16 bytes:
//   mean[l], l = 1 .. 5: the means of level l as ch floats per block (NaN in every channel: nothing known), a plane of
//                        (tw << (6 - l)) x (th << (6 - l)) blocks -- level l padded to whole tiles, tw x th the tile grid;
//   dep: tw x th int32, per tile 1 + the largest level l <= min(5, L) at which a block of the tile has N_l == 0, or 0;
//   for l = 6 .. top, top = max(L, 6): sum[l]  w_l x h_l x ch int64, the exact sums S_l;
//                                      cnt[l]  w_l x h_l int32, the counts N_l;
//                                      val[l]  w_l x h_l x ch floats, the pushed values F_l;
//   flags: four int32: [0] 1 if the image knows nothing, [1] depth.
// (Above L every level is the one block of level L again, so that an image smaller than a tile needs no case of its own.)
#pragma once

#ifdef __HIPCC__
#define FILL_HD __host__ __device__
#else
#define FILL_HD
#endif

namespace fotg {

enum { FILL_TILE = 64, FILL_TILE_LOG = 6, FILL_MAX_DIM = 16384, FILL_MAX_N = 65535, FILL_MAX_LEVEL = 14, FILL_NSTAT = 4, FILL_NFLAG = 4 };

// the blocks of level l along a dimension of v pixels
FILL_HD inline int fill_dim(int v, int l) { return (v + (1 << l) - 1) >> l; }

struct FillLevels {
  int w, h, ch;
  int L;                                  // the first level of size 1 x 1
  int top;                                // max(L, 6)
  int tw, th;                             // the tile grid = the size of level 6
  long long mean[FILL_TILE_LOG];          // [1 .. 5]: byte offsets of the padded mean planes ([0] unused)
  long long dep;                          // byte offset of the tiles' depths
  long long sum[FILL_MAX_LEVEL + 1];      // [6 .. top]: byte offsets
  long long cnt[FILL_MAX_LEVEL + 1];
  long long val[FILL_MAX_LEVEL + 1];
  long long flags;
  long long bytes;                        // of one image, a multiple of 256
};

inline long long fill_align(long long v, long long a) { return (v + a - 1) / a * a; }

// the width of the padded mean plane of level l = 1 .. 5 (its height likewise from th)
FILL_HD inline int fill_plane_dim(int tiles, int l) { return tiles << (FILL_TILE_LOG - l); }

inline FillLevels fill_levels(int w, int h, int ch)
{
  FillLevels g = {};
  g.w = w; g.h = h; g.ch = ch;
  g.L = 0;
  while (fill_dim(w, g.L) > 1 || fill_dim(h, g.L) > 1) ++g.L;
  g.top = g.L > FILL_TILE_LOG ? g.L : FILL_TILE_LOG;
  g.tw = fill_dim(w, FILL_TILE_LOG); g.th = fill_dim(h, FILL_TILE_LOG);
  long long at = 0;
  for (int l = 1; l < FILL_TILE_LOG; ++l) {
    g.mean[l] = at;
    at = fill_align(at + (long long)fill_plane_dim(g.tw, l) * fill_plane_dim(g.th, l) * ch * 4, 16);
  }
  g.dep = at; at = fill_align(at + (long long)g.tw * g.th * 4, 16);
  for (int l = FILL_TILE_LOG; l <= g.top; ++l) {
    const long long blocks = (long long)fill_dim(w, l) * fill_dim(h, l);
    g.sum[l] = at; at = fill_align(at + blocks * ch * 8, 16);
    g.cnt[l] = at; at = fill_align(at + blocks * 4, 16);
    g.val[l] = at; at = fill_align(at + blocks * ch * 4, 16);
  }
  g.flags = at; at += FILL_NFLAG * 4;
  g.bytes = fill_align(at, 256);
  return g;
}

// A call works through its n images in chunks of fill_chunk images, one allocation for all of them: as many images as fit in
// FILL_SCRATCH_CAP bytes, at least one.  The memory of a call is therefore at most max(the bytes of one image, FILL_SCRATCH_CAP).
const long long FILL_SCRATCH_CAP = 1ll << 30;

inline int fill_chunk(int n, long long image_bytes)
{
  const long long fit = FILL_SCRATCH_CAP / image_bytes;
  return fit < 1 ? 1 : (fit < n ? (int)fit : n);
}

inline long long fill_scratch_bytes(int n, int w, int h, int ch)
{
  const long long per = fill_levels(w, h, ch).bytes;
  return per * fill_chunk(n, per);
}

}  // namespace fotg
