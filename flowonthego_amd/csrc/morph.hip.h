// morph.hip.h -- binary morphology of byte maps: erode, dilate, open and close by a disc (include/fotg.h fotg_morph has the same
// definition).
//
// n maps of w x h bytes, 1 <= w, h <= 16384, n <= 65535.  A pixel is set if its byte belongs to the foreground set: with
// fg_codes == 0 every non-zero byte; otherwise fg_codes is an 8-bit set as in fotg_label_components and byte b is set iff
// b < 8 && ((fg_codes >> b) & 1), so that a code map goes in unconverted.  The structuring element is the disc
// dx^2 + dy^2 <= r^2 with r an integer in 0 .. 8, the disc of fotg_erase's grow.  Per map X and stage, on the whole frame:
//   dilate(X, r): a pixel is set iff some pixel of the frame within the disc around it is set;
//   erode(X, r):  a pixel is set iff every pixel of the frame within the disc around it is set.
// Pixels outside the frame take no part in either: the frame border does not erode, and inside the frame exactly
// erode(X, r) = not dilate(not X, r).  r = 0 is the identity and yields the 0 / 1 map of the foreground set.
// A call evaluates a chain of nstage = 1 or 2 stages, stage k an erode (ops[k] == 0) or a dilate (ops[k] == 1) with its own radius
// radii[k], the second on the whole-frame result of the first:
//   open(X, r) = dilate(erode(X, r), r);  close(X, r) = erode(dilate(X, r), r).
// Outputs, each optional, at least one: out (n x h x w uint8, 0 or 1), stats (n x 4 int64 per map: [0] the set pixels of the
// input, [1] the set pixels of the result, [2] the pixels added -- set in the result and not in the input --, [3] the pixels
// removed).  stats is cleared by a stream-ordered memset inside the call and accumulated by integer atomics: the same bytes every run.
//
// morph_kernel: one launch for the whole chain, grid (ceil(w / 64), ceil(h / MO_TH), n), 256 threads: a workgroup owns a 64 x MO_TH
// tile of one map; the intermediate map of a two-stage chain lives in LDS only.  No distance is taken: a binary result needs none.
// Staging: H = the sum of the radii.  The tile and its halo of H as bits, a staged row a string of 128 bits for the columns
// tx0 - 32 .. tx0 + 95 in four dwords (the tile's 64 columns are dwords 1 and 2, the halo the upper 16 bits of dword 0 and the lower
// 16 of dword 3) and a fifth dword of zero padding, MO_TH + 2 H <= MO_TH + 32 rows.  A wave takes two rows at a step with three byte
// loads per lane and three ballots (the 64 tile columns of either row, then the 2 x 16 halo columns of both), as erase_kernel does,
// but the loads of four steps leave together before the first ballot waits for them -- one round trip to memory per four steps --
// and none of them sits behind a branch: a lane without a pixel reads the map's first byte and ignores it.
// The waves also collect whether any staged pixel of the frame is set and whether any is clear: a workgroup whose staged area is
// all clear or all set (the common cases) skips the passes and stores its constant, which every chain leaves unchanged.
// A stage: an item is one dword of one row of its result.  For every dy in -r .. r the 48 bits around the dword are cut from row
// y + dy of the plane before (three dword reads: the row stride of five dwords is odd, the padding serves as the zero beyond either
// end) and dilated horizontally by the disc's half-width floor(sqrt(r^2 - dy^2)) -- a table of nine 4-bit entries the host packs
// into one 64-bit argument -- with shifts and ors that double the run: at most five steps for the 17 columns of r = 8; the 2 r + 1
// rows are or-ed.  Erosion is the same on the complement: a plane is written complemented, and cleared outside the frame, when the
// stage that reads it erodes, and the stage complements its result again.  Stage 1 covers the tile and the halo of stage 2 (rows
// and columns beyond it hold bits that no pixel of the tile depends on), the last stage the tile.
// Stores: a thread owns eight adjacent pixels of a tile row: one 8-byte nontemporal store where the address allows it, two dword
// stores where that allows it, bytes otherwise and at the right border.  Statistics: population counts of the thread's eight bits
// before and after, summed per wave by xor shuffles, per workgroup through LDS, one 64-bit integer atomic per non-zero column.
// No floating point, no private memory, no workgroup waits for another.
// MO_TH = 64: at H = 16 the staged area is 2.25 times the tile (4.5 times at 16 rows, 3 times at 32); measured at 16, 32 and 64 rows,
// 64 was the fastest for every operation and map.
#pragma once
#include "common.h"

namespace fotg {

#ifndef MO_TH
#define MO_TH 64
#endif
enum { MO_TW = 64, MO_THREADS = 256, MO_MAXR = 8, MO_MAXH = 2 * MO_MAXR, MO_ROWS = MO_TH + 2 * MO_MAXH, MO_STRIDE = 5,
       MO_PLANE = MO_ROWS * MO_STRIDE + 2, MO_BATCH = 4, MO_NSTAT = 4, MO_MAX_DIM = 16384, MO_ERODE = 0, MO_DILATE = 1 };

// the bits of dword m (columns x0 .. x0 + 31, x0 >= -32) that lie inside a frame of w columns
__device__ __forceinline__ unsigned morph_colmask(int x0, int w)
{
  const int lo = x0 < 0 ? -x0 : 0, hi = w - x0 < 32 ? w - x0 : 32;
  if (hi <= lo) return 0u;
  const unsigned below_hi = hi == 32 ? ~0u : (1u << hi) - 1u, below_lo = lo == 32 ? ~0u : (1u << lo) - 1u;
  return below_hi & ~below_lo;
}

// One stage.  src, dst: planes of MO_PLANE dwords, staged row j at dword 1 + j * MO_STRIDE; the rows j0 .. j1 - 1 of dst are made
// from the rows j0 - r .. j1 - 1 + r of src.  src holds the stage's input, complemented inside the frame if the stage erodes;
// dst receives its result, complemented inside the frame if comp_next (the stage that reads it erodes).
__device__ __forceinline__ void morph_stage(const unsigned *__restrict__ src, unsigned *__restrict__ dst, int j0, int j1, int r,
                                            unsigned long long hw, bool erode, bool comp_next, int ytop, int h, unsigned cm0, unsigned cm1,
                                            unsigned cm2, unsigned cm3)
{
  typedef unsigned long long u64;
  for (int i = (int)threadIdx.x; i < (j1 - j0) * 4; i += MO_THREADS) {
    const int j = j0 + (i >> 2), m = i & 3;
    unsigned acc = 0u;
    for (int dy = -r; dy <= r; ++dy) {                            // (uniform)
      const int k = (int)((hw >> (4 * (dy < 0 ? -dy : dy))) & 15u);
      const unsigned *row = src + (j + dy) * MO_STRIDE + m;       // row[0]: the dword before (or padding), row[1]: this one, row[2]: the next
      const u64 win = ((u64)row[0] >> 24) | ((u64)row[1] << 8) | ((u64)row[2] << 40);      // bit b: column 32 m - 8 + b
      // the or of the 2 k + 1 columns from -k on: runs of 1, 2, 4 ... columns, then two of them overlapped
      u64 c = win >> (8 - k);
      const int len = 2 * k + 1;
      int run = 1;
      while (2 * run <= len) { c |= c >> run; run *= 2; }
      c |= c >> (len - run);
      acc |= (unsigned)c;
    }
    const int y = ytop + j;
    const unsigned fm = (y >= 0 && y < h) ? (m == 0 ? cm0 : m == 1 ? cm1 : m == 2 ? cm2 : cm3) : 0u;
    unsigned res = (erode ? ~acc : acc) & fm;
    if (comp_next) res = ~res & fm;
    dst[1 + j * MO_STRIDE + m] = res;
  }
}

// four bits -> four bytes of 0 / 1 (the shifted copies of b do not meet: nothing carries)
__device__ __forceinline__ unsigned morph_spread4(unsigned b) { return ((b & 15u) * 0x00204081u) & 0x01010101u; }

// src: n x h x w bytes; fg: 0 or the 8-bit set; ns: 1 or 2 stages, stage k erodes if e<k> and has radius r<k> and the packed
// half-widths hw<k> (4 bits per |dy|); out: n x h x w bytes or null; stats: n x 4 (cleared by the host) or null.
__global__ __launch_bounds__(MO_THREADS) void morph_kernel(const unsigned char *__restrict__ src, int w, int h, unsigned fg, int ns, int e1,
                                                            int r1, unsigned long long hw1, int e2, int r2, unsigned long long hw2,
                                                            unsigned char *__restrict__ out, unsigned long long *__restrict__ stats)
{
  typedef unsigned long long u64;
  __shared__ unsigned mo_plane[3][MO_PLANE];                      // the input, the result of stage 1, the result of stage 2
  __shared__ unsigned mo_seen[MO_THREADS / FOTG_WAVE][2];
  __shared__ unsigned mo_red[MO_THREADS / FOTG_WAVE][MO_NSTAT];
  const int img = blockIdx.z, t = threadIdx.x, lane = t % FOTG_WAVE, wave = t / FOTG_WAVE;
  const int tx0 = blockIdx.x * MO_TW, ty0 = blockIdx.y * MO_TH;
  const int H = ns == 2 ? r1 + r2 : r1;
  const int ytop = ty0 - H, nrows = MO_TH + 2 * H;
  const unsigned char *__restrict__ in = src + (size_t)img * w * h;
  const unsigned cm0 = morph_colmask(tx0 - 32, w), cm1 = morph_colmask(tx0, w), cm2 = morph_colmask(tx0 + 32, w),
                 cm3 = morph_colmask(tx0 + 64, w);

  // the padding dwords, and the rows the stages never write
  for (int i = t; i < 3 * MO_PLANE; i += MO_THREADS) (&mo_plane[0][0])[i] = 0u;
  __syncthreads();

  // staging: two rows per wave and step.  c: the column in the 128-bit string; `known`: a pixel of the frame within the halo
  auto known = [&](int j, int c) -> bool {
    const int x = tx0 - 32 + c, y = ytop + j;
    return j < nrows && c >= 32 - H && c < 32 + MO_TW + H && x >= 0 && x < w && y >= 0 && y < h;
  };
  // the byte of a known pixel, of the map's first pixel otherwise: a load without a branch
  auto probe = [&](int j, int c) -> unsigned {
    return in[known(j, c) ? (size_t)(ytop + j) * w + (tx0 - 32 + c) : (size_t)0];
  };
  auto set = [&](unsigned b, bool k) -> bool { return k && (fg ? (b < 8u && ((fg >> b) & 1u)) : b != 0u); };
  u64 any_set = 0, any_clear = 0;
  const int cc = (lane & 16) ? 96 + (lane & 15) : 16 + (lane & 15);           // lanes 0 .. 31: the halo columns of row j, 32 .. 63: of row j + 1
  for (int p0 = wave; 2 * p0 < nrows; p0 += MO_BATCH * (MO_THREADS / FOTG_WAVE)) {
    // the loads of MO_BATCH steps leave together, then their ballots: one round trip to memory per batch, not per step
    unsigned va[MO_BATCH], vb[MO_BATCH], vc[MO_BATCH];
#pragma unroll
    for (int u = 0; u < MO_BATCH; ++u) {
      const int j = 2 * (p0 + u * (MO_THREADS / FOTG_WAVE));
      va[u] = probe(j, 32 + lane); vb[u] = probe(j + 1, 32 + lane); vc[u] = probe(j + (lane >> 5), cc);
    }
#pragma unroll
    for (int u = 0; u < MO_BATCH; ++u) {
      const int j = 2 * (p0 + u * (MO_THREADS / FOTG_WAVE));
      const u64 ka = __ballot(known(j, 32 + lane)), kb = __ballot(known(j + 1, 32 + lane)), kc = __ballot(known(j + (lane >> 5), cc));
      const u64 a = __ballot(set(va[u], known(j, 32 + lane))), b = __ballot(set(vb[u], known(j + 1, 32 + lane))),
                c = __ballot(set(vc[u], known(j + (lane >> 5), cc)));
      any_set |= a | b | c;
      any_clear |= (ka & ~a) | (kb & ~b) | (kc & ~c);
      if (lane == 0) {
        unsigned d[2][4] = {{((unsigned)c & 0xffffu) << 16, (unsigned)a, (unsigned)(a >> 32), ((unsigned)c >> 16) & 0xffffu},
                            {((unsigned)(c >> 32) & 0xffffu) << 16, (unsigned)b, (unsigned)(b >> 32), (unsigned)(c >> 48) & 0xffffu}};
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const int y = ytop + j + q;
          if (j + q < nrows) {
            const bool inside = y >= 0 && y < h;
            unsigned *row = &mo_plane[0][1 + (j + q) * MO_STRIDE];
            if (e1) {                                               // stage 1 erodes: it reads the complement inside the frame
              row[0] = inside ? ~d[q][0] & cm0 : 0u; row[1] = inside ? ~d[q][1] & cm1 : 0u;
              row[2] = inside ? ~d[q][2] & cm2 : 0u; row[3] = inside ? ~d[q][3] & cm3 : 0u;
            } else {
              row[0] = d[q][0]; row[1] = d[q][1]; row[2] = d[q][2]; row[3] = d[q][3];
            }
          }
        }
      }
    }
  }
  if (lane == 0) { mo_seen[wave][0] = any_set != 0 ? 1u : 0u; mo_seen[wave][1] = any_clear != 0 ? 1u : 0u; }
  __syncthreads();
  const bool some_set = (mo_seen[0][0] | mo_seen[1][0] | mo_seen[2][0] | mo_seen[3][0]) != 0u;       // (uniform over the workgroup)
  const bool some_clear = (mo_seen[0][1] | mo_seen[1][1] | mo_seen[2][1] | mo_seen[3][1]) != 0u;
  const bool constant = !(some_set && some_clear);

  if (!constant) {
    if (ns == 2) {
      morph_stage(mo_plane[0], mo_plane[1], r1, nrows - r1, r1, hw1, e1 != 0, e2 != 0, ytop, h, cm0, cm1, cm2, cm3);
      __syncthreads();
      morph_stage(mo_plane[1], mo_plane[2], H, H + MO_TH, r2, hw2, e2 != 0, false, ytop, h, cm0, cm1, cm2, cm3);
    } else {
      morph_stage(mo_plane[0], mo_plane[2], H, H + MO_TH, r1, hw1, e1 != 0, false, ytop, h, cm0, cm1, cm2, cm3);
    }
    __syncthreads();
  }

  // the thread's eight pixels: before and after
  unsigned nbefore = 0, nafter = 0, nadd = 0, nrem = 0;
  for (int i = t; i < MO_TH * (MO_TW / 8); i += MO_THREADS) {
    const int ty = i / (MO_TW / 8), g = i % (MO_TW / 8);
    const int x0 = tx0 + 8 * g, y = ty0 + ty;
    const int nb = y < h ? (w - x0 < 8 ? (w - x0 < 0 ? 0 : w - x0) : 8) : 0;
    if (nb > 0) {
      const unsigned keep = (1u << nb) - 1u;
      const int at = 1 + (H + ty) * MO_STRIDE + 1 + (g >> 2), sh = 8 * (g & 3);
      unsigned was, now;
      if (constant) {
        was = now = some_set ? keep : 0u;
      } else {
        const unsigned a = mo_plane[0][at] >> sh;
        was = (e1 ? ~a : a) & keep;
        now = (mo_plane[2][at] >> sh) & keep;
      }
      nbefore += __popc(was); nafter += __popc(now); nadd += __popc(now & ~was); nrem += __popc(was & ~now);
      if (out) {
        unsigned char *o = out + ((size_t)img * h + y) * w + x0;
        const unsigned lo = morph_spread4(now), hi = morph_spread4(now >> 4);
        int k = 0;
        if ((((size_t)o) & 3) == 0) {
          if (nb == 8 && (((size_t)o) & 7) == 0) {
            typedef unsigned vu2 __attribute__((ext_vector_type(2)));
            __builtin_nontemporal_store(vu2{lo, hi}, reinterpret_cast<vu2 *>(o));
            k = 8;
          } else {
            if (nb >= 4) { __builtin_nontemporal_store(lo, reinterpret_cast<unsigned *>(o)); k = 4; }
            if (nb == 8) { __builtin_nontemporal_store(hi, reinterpret_cast<unsigned *>(o) + 1); k = 8; }
          }
        }
        for (; k < nb; ++k) o[k] = (unsigned char)((now >> k) & 1u);
      }
    }
  }

  if (stats) {                                                    // (uniform)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      nbefore += __shfl_xor(nbefore, o, 64); nafter += __shfl_xor(nafter, o, 64);
      nadd += __shfl_xor(nadd, o, 64); nrem += __shfl_xor(nrem, o, 64);
    }
    if (lane == 0) { mo_red[wave][0] = nbefore; mo_red[wave][1] = nafter; mo_red[wave][2] = nadd; mo_red[wave][3] = nrem; }
    __syncthreads();
    if (t < MO_NSTAT) {
      u64 tot = 0;
      for (int i = 0; i < MO_THREADS / FOTG_WAVE; ++i) tot += mo_red[i][t];
      if (tot) atomicAdd(stats + (size_t)img * MO_NSTAT + t, tot);
    }
  }
}

}  // namespace fotg
