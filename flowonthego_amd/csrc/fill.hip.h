// fill.hip.h -- hole filling by pull-push: the unknown pixels of an image or a flow filled from the known ones, at any hole size
// (include/fotg.h fotg_fill has the same definition; Gortler et al., "The Lumigraph", 1996; Kraus, "The pull-push algorithm
// revisited", 2009).
//
// n images of w x h pixels with ch interleaved channels, 1 <= w, h <= 16384, 1 <= n <= 65535.  f32 images take ch in {1, 2, 3}, uint8
// images ch in {1, 3}.  hole is n x h x w uint8, or NULL (f32 only).  fg_codes in 0 .. 255 follows fotg_morph's rule: with
// fg_codes == 0 every non-zero byte is a hole; otherwise byte b is a hole iff b < 8 && ((fg_codes >> b) & 1), so that a code map
// goes in unconverted.
// Known pixels: a pixel is known iff it is not a hole and, for f32, every channel v is finite with |v| <= 32768.  A NaN, an infinity
// and the .flo unknown marker 1e9 are therefore holes with no map at all.
// Pull (exact integers): q = lrintf(256 v) per channel (256 v is exact in f32; for uint8 q = 256 v).  Level 0 has S_0 = q and N_0 = 1
// at known pixels and 0 elsewhere.  Level l+1 has size w_{l+1} = (w_l + 1) >> 1, h_{l+1} = (h_l + 1) >> 1; S_{l+1}(X, Y) and
// N_{l+1}(X, Y) are the sums over the children (2X + i, 2Y + j), i, j in {0, 1}, that lie inside level l.  L is the first level of
// size 1 x 1.  S is an int64 per channel with |S| <= 2^51, N an integer <= 2^28.
// Empty image: if N_L == 0 the image knows nothing; then dst = src bit for bit and code is 2 at every hole pixel and 0 at every known
// pixel.
// Mean of a block with N_l > 0: M_l = (float)((double)S_l / (double)(256 N_l)), one f64 division rounded once to f32 (exact to
// restate, because |S| < 2^53).
// Push, for l = L-1 down to 0: F_L = M_L.  At level l a pixel with N_l > 0 and l >= 1 has F_l = M_l.  A pixel with N_l == 0 at (x, y)
// takes the bilinear value of its four parents: px = x >> 1, px2 = clamp(px + (x & 1 ? 1 : -1), 0, w_{l+1} - 1), py and py2 likewise;
// a = F_{l+1}(px, py), b = F_{l+1}(px2, py), c = F_{l+1}(px, py2), d = F_{l+1}(px2, py2);
//   F_l = ((a*9 + b*3) + (c*3 + d)) * 0.0625 in f32, in exactly this order, with no contraction.
// At level 0 a known pixel keeps its source value bit for bit (it does not become its quantised value); a hole pixel gets F_0, for
// uint8 rintf, clamped to [0, 255] (fotg_warp's to_u8).
// Outputs, each optional, at least one: dst (same type and shape as src), code (n x h x w uint8: 0 known (kept), 1 filled, 2 nothing
// known in this image (kept)), stats (n x 4 int64: known, filled, unfilled, depth).  depth = 1 + the largest l at which some block
// has N_l == 0, and 0 without holes: the log2 scale of the widest hole.  stats is zeroed by a stream-ordered memset and accumulated
// with integer atomics and integer maxima: the same bytes every run.
//
// Three launches per chunk of images, over the stream-ordered memory fill_levels.h lays out; levels that depend on each other across
// tiles are separated by the launches, and no workgroup ever waits for another.  A 64 x 64 tile of level 0 is one block of level 6
// and level blocks align with tiles, so below level 6 no tile needs another's sums.
// fill_pull_kernel<T, CH>: grid (tw, th, images), 256 threads, a workgroup per tile.  A thread reads a 4 x 4 block of pixels, tests
//   the hole byte and the value, and sums its four blocks of level 1 and its block of level 2 in registers (32-bit: 16 pixels of
//   |q| <= 2^23).  Levels 3 .. 6 are summed through LDS by 64, 16, 4 and 1 threads, in 64 bits.  It writes the means of the levels
//   1 .. 5 (NaN: N == 0) into planes padded to whole tiles, the exact S and N of level 6, and the tile's share of depth.
// fill_top_kernel<CH>: grid (images), a workgroup per image.  It takes the maximum of the tiles' depths, pulls the levels 7 .. L from
//   the sums of level 6 (at most 256 x 256 blocks), writes the empty flag and the depth, and pushes F_L .. F_6 back down.  A level is
//   read only after the barrier that follows its writing.
// fill_push_kernel<T, CH>: grid (tw, th, images), a workgroup per tile.  A tile of an empty image, and a tile without a hole
//   (N_6 == its pixels), is copied.  Otherwise the workgroup stages in LDS, with a halo of one block, F_6 (3 x 3), and then level by
//   level F_5 (4 x 4) .. F_1 (34 x 34): a block's mean where it has one, the bilinear value of its staged parents where it has
//   none.  A halo block is computed by the same formula from the same numbers as in the tile that owns it, so neighbouring tiles
//   agree.  (1641 blocks: 19.2 KB at ch = 3.)  Then a thread takes a pixel of each of 16 rows: a known pixel is copied, a hole takes
//   the bilinear value of its parents in F_1.  dst and code are stored element by element, at any alignment; the counts are summed
//   per wave by xor shuffles, per workgroup through LDS, one integer atomic per non-zero count; tile (0, 0) stores the depth.
// No private memory; the only floating-point operations are the division, the bilinear formula and the conversions.
#pragma once
#include "common.h"
#include "fill_levels.h"

namespace fotg {

enum { FILL_THREADS = 256,
       FILL_PULL_BLOCKS = 256 + 64 + 16 + 4 + 1,                  // the blocks of the levels 2 .. 6 of a tile
       FILL_PUSH_BLOCKS = 9 + 16 + 36 + 100 + 324 + 1156 };       // the blocks of the levels 6 .. 1 of a tile with their halo

__device__ __forceinline__ bool fill_is_hole(unsigned b, unsigned fg) { return fg ? (b < 8u && ((fg >> b) & 1u)) : b != 0u; }

__device__ __forceinline__ float fill_mean(long long S, int N) { return (float)((double)S / (double)(256ll * (long long)N)); }

__device__ __forceinline__ float fill_bilinear(float a, float b, float c, float d) { return ((a * 9.0f + b * 3.0f) + (c * 3.0f + d)) * 0.0625f; }

// the value of a pixel: is it known, and its channels as 256 v
__device__ __forceinline__ bool fill_known(float v, int *q)
{
  const bool ok = fabsf(v) <= 32768.0f;                           // false for a NaN
  *q = ok ? (int)rintf(256.0f * v) : 0;
  return ok;
}
__device__ __forceinline__ bool fill_known(unsigned char v, int *q)
{
  *q = 256 * (int)v;
  return true;
}

__device__ __forceinline__ void fill_store(float *p, float f) { *p = f; }
__device__ __forceinline__ void fill_store(unsigned char *p, float f) { *p = (unsigned char)fminf(fmaxf(rintf(f), 0.0f), 255.0f); }

// One pixel: raw[CH] its channels as they are, q[CH] as integers (0 where it is not known); returns whether it is known.
template <typename T, int CH>
__device__ __forceinline__ bool fill_pixel(const T *__restrict__ in, const unsigned char *__restrict__ hole, size_t p, unsigned fg, T *raw, int *q)
{
  bool known = hole ? !fill_is_hole(hole[p], fg) : true;
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    raw[c] = in[p * CH + c];
    known = fill_known(raw[c], &q[c]) && known;
  }
  if (!known) {
#pragma unroll
    for (int c = 0; c < CH; ++c) q[c] = 0;
  }
  return known;
}

// src: images x h x w x CH; hole: images x h x w or null; scratch: images x g.bytes
template <typename T, int CH>
__global__ __launch_bounds__(FILL_THREADS) void fill_pull_kernel(const T *__restrict__ src, const unsigned char *__restrict__ hole, unsigned fg,
                                                                  FillLevels g, unsigned char *__restrict__ scratch)
{
  __shared__ long long pl_sum[FILL_PULL_BLOCKS * CH];
  __shared__ int pl_cnt[FILL_PULL_BLOCKS];
  __shared__ int pl_depth;
  const int t = threadIdx.x, bx = t & 15, by = t >> 4, tx = blockIdx.x, ty = blockIdx.y;
  const size_t img = blockIdx.z, npx = (size_t)g.w * g.h;
  const T *__restrict__ in = src + img * npx * CH;
  const unsigned char *__restrict__ ho = hole ? hole + img * npx : nullptr;
  unsigned char *__restrict__ sc = scratch + img * (size_t)g.bytes;
  const float nanf_ = __builtin_nanf("");
  if (t == 0) pl_depth = 0;

  // the thread's 4 x 4 pixels: four blocks of level 1
  int s1[4][CH], n1[4] = {0, 0, 0, 0};
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int c = 0; c < CH; ++c) s1[k][c] = 0;
  int depth = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int x = tx * FILL_TILE + bx * 4 + i, y = ty * FILL_TILE + by * 4 + j;
      if (x < g.w && y < g.h) {
        T raw[CH];
        int q[CH];
        const bool known = fill_pixel<T, CH>(in, ho, (size_t)y * g.w + x, fg, raw, q);
        if (!known) depth = 1;
        n1[(j >> 1) * 2 + (i >> 1)] += known ? 1 : 0;
#pragma unroll
        for (int c = 0; c < CH; ++c) s1[(j >> 1) * 2 + (i >> 1)][c] += q[c];
      }
    }
  }
  {
    float *__restrict__ plane = reinterpret_cast<float *>(sc + g.mean[1]);
    const int pw = fill_plane_dim(g.tw, 1), w1 = fill_dim(g.w, 1), h1 = fill_dim(g.h, 1);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int X = tx * 32 + bx * 2 + (k & 1), Y = ty * 32 + by * 2 + (k >> 1);
#pragma unroll
      for (int c = 0; c < CH; ++c) plane[((size_t)Y * pw + X) * CH + c] = n1[k] > 0 ? fill_mean(s1[k][c], n1[k]) : nanf_;
      if (n1[k] == 0 && X < w1 && Y < h1 && g.L >= 1) depth = 2;
    }
  }
  {
    float *__restrict__ plane = reinterpret_cast<float *>(sc + g.mean[2]);
    const int pw = fill_plane_dim(g.tw, 2), X = tx * 16 + bx, Y = ty * 16 + by;
    const int n2 = n1[0] + n1[1] + n1[2] + n1[3];
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int s2 = s1[0][c] + s1[1][c] + s1[2][c] + s1[3][c];
      plane[((size_t)Y * pw + X) * CH + c] = n2 > 0 ? fill_mean(s2, n2) : nanf_;
      pl_sum[t * CH + c] = s2;
    }
    pl_cnt[t] = n2;
    if (n2 == 0 && X < fill_dim(g.w, 2) && Y < fill_dim(g.h, 2) && g.L >= 2) depth = 3;
  }

  // the levels 3 .. 6 of the tile through LDS: level l has dim x dim blocks at `off`
  int off = 0, dim = 16;
  for (int l = 3; l <= FILL_TILE_LOG; ++l) {
    __syncthreads();
    const int nd = dim >> 1, noff = off + dim * dim;
    if (t < nd * nd) {
      const int X = t % nd, Y = t / nd;
      long long s[CH];
      int n = 0;
#pragma unroll
      for (int c = 0; c < CH; ++c) s[c] = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int at = off + (2 * Y + (k >> 1)) * dim + 2 * X + (k & 1);
        n += pl_cnt[at];
#pragma unroll
        for (int c = 0; c < CH; ++c) s[c] += pl_sum[at * CH + c];
      }
      pl_cnt[noff + t] = n;
#pragma unroll
      for (int c = 0; c < CH; ++c) pl_sum[(noff + t) * CH + c] = s[c];
      const int GX = tx * nd + X, GY = ty * nd + Y;
      if (l < FILL_TILE_LOG) {
        float *__restrict__ plane = reinterpret_cast<float *>(sc + g.mean[l]);
        const int pw = fill_plane_dim(g.tw, l);
#pragma unroll
        for (int c = 0; c < CH; ++c) plane[((size_t)GY * pw + GX) * CH + c] = n > 0 ? fill_mean(s[c], n) : nanf_;
        if (n == 0 && GX < fill_dim(g.w, l) && GY < fill_dim(g.h, l) && g.L >= l) depth = l + 1;
      } else {
        const size_t b = (size_t)ty * g.tw + tx;
        long long *__restrict__ sum6 = reinterpret_cast<long long *>(sc + g.sum[FILL_TILE_LOG]);
#pragma unroll
        for (int c = 0; c < CH; ++c) sum6[b * CH + c] = s[c];
        reinterpret_cast<int *>(sc + g.cnt[FILL_TILE_LOG])[b] = n;
      }
    }
    off = noff;
    dim = nd;
  }
  if (depth) atomicMax(&pl_depth, depth);
  __syncthreads();
  if (t == 0) reinterpret_cast<int *>(sc + g.dep)[(size_t)ty * g.tw + tx] = pl_depth;
}

template <int CH>
__global__ __launch_bounds__(FILL_THREADS) void fill_top_kernel(FillLevels g, unsigned char *__restrict__ scratch)
{
  __shared__ int tp_depth;
  const int t = threadIdx.x;
  unsigned char *sc = scratch + (size_t)blockIdx.x * (size_t)g.bytes;
  if (t == 0) tp_depth = 0;
  int depth = 0;
  {
    const int *dep = reinterpret_cast<const int *>(sc + g.dep);
    for (int i = t; i < g.tw * g.th; i += FILL_THREADS) depth = dep[i] > depth ? dep[i] : depth;
  }
  // level 6 counts as well: a tile that knows nothing
  {
    const int *c6 = reinterpret_cast<const int *>(sc + g.cnt[FILL_TILE_LOG]);
    if (g.L >= FILL_TILE_LOG)
      for (int i = t; i < g.tw * g.th; i += FILL_THREADS)
        if (c6[i] == 0) depth = depth > FILL_TILE_LOG + 1 ? depth : FILL_TILE_LOG + 1;
  }
  // pull: the levels 7 .. L
  for (int l = FILL_TILE_LOG + 1; l <= g.top; ++l) {
    const int wl = fill_dim(g.w, l), hl = fill_dim(g.h, l), wc = fill_dim(g.w, l - 1), hc = fill_dim(g.h, l - 1);
    const long long *cs = reinterpret_cast<const long long *>(sc + g.sum[l - 1]);
    const int *cn = reinterpret_cast<const int *>(sc + g.cnt[l - 1]);
    long long *ps = reinterpret_cast<long long *>(sc + g.sum[l]);
    int *pn = reinterpret_cast<int *>(sc + g.cnt[l]);
    for (int i = t; i < wl * hl; i += FILL_THREADS) {
      const int X = i % wl, Y = i / wl;
      long long s[CH];
      int n = 0;
#pragma unroll
      for (int c = 0; c < CH; ++c) s[c] = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int cx = 2 * X + (k & 1), cy = 2 * Y + (k >> 1);
        if (cx < wc && cy < hc) {
          n += cn[cy * wc + cx];
#pragma unroll
          for (int c = 0; c < CH; ++c) s[c] += cs[(size_t)(cy * wc + cx) * CH + c];
        }
      }
      pn[i] = n;
#pragma unroll
      for (int c = 0; c < CH; ++c) ps[(size_t)i * CH + c] = s[c];
      if (n == 0) depth = l + 1;                                    // (l <= L here; later levels are larger)
    }
    __syncthreads();
  }
  if (depth) atomicMax(&tp_depth, depth);
  __syncthreads();
  const bool empty = reinterpret_cast<const int *>(sc + g.cnt[g.top])[0] == 0;          // (uniform)
  if (t == 0) {
    int *flags = reinterpret_cast<int *>(sc + g.flags);
    flags[0] = empty ? 1 : 0;
    flags[1] = tp_depth;
    flags[2] = 0;
    flags[3] = 0;
  }
  if (empty) return;
  // push: F_top .. F_6
  for (int l = g.top; l >= FILL_TILE_LOG; --l) {
    const int wl = fill_dim(g.w, l), hl = fill_dim(g.h, l), wp = fill_dim(g.w, l + 1), hp = fill_dim(g.h, l + 1);
    const long long *ls = reinterpret_cast<const long long *>(sc + g.sum[l]);
    const int *ln = reinterpret_cast<const int *>(sc + g.cnt[l]);
    float *lv = reinterpret_cast<float *>(sc + g.val[l]);
    const float *pv = reinterpret_cast<const float *>(sc + g.val[l < g.top ? l + 1 : l]);
    for (int i = t; i < wl * hl; i += FILL_THREADS) {
      const int n = ln[i];
      if (n > 0) {
#pragma unroll
        for (int c = 0; c < CH; ++c) lv[(size_t)i * CH + c] = fill_mean(ls[(size_t)i * CH + c], n);
      } else {                                                      // (l < top: the top block of an image that is not empty has n > 0)
        const int X = i % wl, Y = i / wl;
        const int px = X >> 1, px2 = clampi(px + ((X & 1) ? 1 : -1), wp), py = Y >> 1, py2 = clampi(py + ((Y & 1) ? 1 : -1), hp);
#pragma unroll
        for (int c = 0; c < CH; ++c)
          lv[(size_t)i * CH + c] = fill_bilinear(pv[(size_t)(py * wp + px) * CH + c], pv[(size_t)(py * wp + px2) * CH + c],
                                                 pv[(size_t)(py2 * wp + px) * CH + c], pv[(size_t)(py2 * wp + px2) * CH + c]);
      }
    }
    __syncthreads();
  }
}

// dst, code, stats: each may be null; stats: images x 4 (cleared by the host)
template <typename T, int CH>
__global__ __launch_bounds__(FILL_THREADS) void fill_push_kernel(const T *__restrict__ src, const unsigned char *__restrict__ hole, unsigned fg,
                                                                  FillLevels g, const unsigned char *__restrict__ scratch, T *__restrict__ dst,
                                                                  unsigned char *__restrict__ code, unsigned long long *__restrict__ stats)
{
  __shared__ float ps_val[FILL_PUSH_BLOCKS * CH];
  __shared__ unsigned ps_red[FILL_THREADS / FOTG_WAVE][3];
  const int t = threadIdx.x, lane = t % FOTG_WAVE, wave = t / FOTG_WAVE, tx = blockIdx.x, ty = blockIdx.y;
  const size_t img = blockIdx.z, npx = (size_t)g.w * g.h;
  const T *__restrict__ in = src + img * npx * CH;
  const unsigned char *__restrict__ ho = hole ? hole + img * npx : nullptr;
  const unsigned char *__restrict__ sc = scratch + img * (size_t)g.bytes;
  const int *flags = reinterpret_cast<const int *>(sc + g.flags);
  const bool empty = flags[0] != 0;                                                     // (uniform)
  const int tile_w = g.w - tx * FILL_TILE < FILL_TILE ? g.w - tx * FILL_TILE : FILL_TILE;
  const int tile_h = g.h - ty * FILL_TILE < FILL_TILE ? g.h - ty * FILL_TILE : FILL_TILE;
  const bool stage = !empty && reinterpret_cast<const int *>(sc + g.cnt[FILL_TILE_LOG])[(size_t)ty * g.tw + tx] != tile_w * tile_h;

  int at1 = 0;                                                                          // where F_1 is staged
  if (stage) {                                                                          // (uniform)
    if (t < 9) {
      const int X = tx - 1 + t % 3, Y = ty - 1 + t / 3;
      if (X >= 0 && X < g.tw && Y >= 0 && Y < g.th) {
        const float *v6 = reinterpret_cast<const float *>(sc + g.val[FILL_TILE_LOG]);
#pragma unroll
        for (int c = 0; c < CH; ++c) ps_val[t * CH + c] = v6[((size_t)Y * g.tw + X) * CH + c];
      }
    }
    __syncthreads();
    int pat = 0, at = 9;                                            // the staged parents' level and this one, in blocks
    for (int l = FILL_TILE_LOG - 1; l >= 1; --l) {
      const int sz = 1 << (FILL_TILE_LOG - l), d = sz + 2, dp = (sz >> 1) + 2;
      const int wl = fill_dim(g.w, l), hl = fill_dim(g.h, l), wp = fill_dim(g.w, l + 1), hp = fill_dim(g.h, l + 1);
      const int x0 = tx * sz - 1, y0 = ty * sz - 1, xp0 = tx * (sz >> 1) - 1, yp0 = ty * (sz >> 1) - 1;
      const float *__restrict__ plane = reinterpret_cast<const float *>(sc + g.mean[l]);
      const int pw = fill_plane_dim(g.tw, l);
      for (int i = t; i < d * d; i += FILL_THREADS) {
        const int X = x0 + i % d, Y = y0 + i / d;
        if (X >= 0 && X < wl && Y >= 0 && Y < hl) {
          float v[CH];
#pragma unroll
          for (int c = 0; c < CH; ++c) v[c] = plane[((size_t)Y * pw + X) * CH + c];
          if (v[0] != v[0]) {                                       // nothing known in this block
            const int px = (X >> 1) - xp0, px2 = clampi((X >> 1) + ((X & 1) ? 1 : -1), wp) - xp0;
            const int py = (Y >> 1) - yp0, py2 = clampi((Y >> 1) + ((Y & 1) ? 1 : -1), hp) - yp0;
#pragma unroll
            for (int c = 0; c < CH; ++c)
              v[c] = fill_bilinear(ps_val[(pat + py * dp + px) * CH + c], ps_val[(pat + py * dp + px2) * CH + c],
                                   ps_val[(pat + py2 * dp + px) * CH + c], ps_val[(pat + py2 * dp + px2) * CH + c]);
          }
#pragma unroll
          for (int c = 0; c < CH; ++c) ps_val[(at + i) * CH + c] = v[c];
        }
      }
      __syncthreads();
      pat = at;
      at += d * d;
    }
    at1 = pat;
  }

  // level 0: a pixel of each of 16 rows
  unsigned nk = 0, nf = 0, nu = 0;
  const int wp = fill_dim(g.w, 1), hp = fill_dim(g.h, 1), xp0 = tx * 32 - 1, yp0 = ty * 32 - 1;
  const int x = tx * FILL_TILE + lane;
  for (int k = 0; k < FILL_TILE / (FILL_THREADS / FOTG_WAVE); ++k) {
    const int y = ty * FILL_TILE + wave + k * (FILL_THREADS / FOTG_WAVE);
    if (x < g.w && y < g.h) {
      const size_t p = (size_t)y * g.w + x;
      T raw[CH];
      int q[CH];
      const bool known = fill_pixel<T, CH>(in, ho, p, fg, raw, q);
      const bool fillit = !known && !empty;
      nk += known ? 1u : 0u; nf += fillit ? 1u : 0u; nu += (!known && empty) ? 1u : 0u;
      if (code) code[img * npx + p] = known ? 0 : (empty ? 2 : 1);
      if (dst) {
        T *__restrict__ o = dst + (img * npx + p) * CH;
        if (fillit) {
          const int px = (x >> 1) - xp0, px2 = clampi((x >> 1) + ((x & 1) ? 1 : -1), wp) - xp0;
          const int py = (y >> 1) - yp0, py2 = clampi((y >> 1) + ((y & 1) ? 1 : -1), hp) - yp0;
#pragma unroll
          for (int c = 0; c < CH; ++c)
            fill_store(o + c, fill_bilinear(ps_val[(at1 + py * 34 + px) * CH + c], ps_val[(at1 + py * 34 + px2) * CH + c],
                                            ps_val[(at1 + py2 * 34 + px) * CH + c], ps_val[(at1 + py2 * 34 + px2) * CH + c]));
        } else {
#pragma unroll
          for (int c = 0; c < CH; ++c) o[c] = raw[c];
        }
      }
    }
  }

  if (stats) {                                                                          // (uniform)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { nk += __shfl_xor(nk, o, 64); nf += __shfl_xor(nf, o, 64); nu += __shfl_xor(nu, o, 64); }
    if (lane == 0) { ps_red[wave][0] = nk; ps_red[wave][1] = nf; ps_red[wave][2] = nu; }
    __syncthreads();
    if (t < 3) {
      unsigned long long tot = 0;
      for (int i = 0; i < FILL_THREADS / FOTG_WAVE; ++i) tot += ps_red[i][t];
      if (tot) atomicAdd(stats + img * FILL_NSTAT + t, tot);
    }
    if (t == 3 && tx == 0 && ty == 0) stats[img * FILL_NSTAT + 3] = (unsigned long long)flags[1];
  }
}

}  // namespace fotg
