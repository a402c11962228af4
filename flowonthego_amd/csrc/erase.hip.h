// erase.hip.h -- object removal: a mask grown by a disc, feathered at its rim and filled from the plate (include/fotg.h fotg_erase has
// the same definition).
//
// n frames of w x h with 1 or 3 interleaved channels, f32 or 8-bit; P plates on a W x H canvas with integer origin (ox, oy), index,
// plate_code, mask and the three sources of the vector frame i -> reference (dense flows, six f64 parameters per frame through
// MotionSrc, a context's coarse flows through UpsampleSrc) exactly as in fotg_subtract.  remove: n x h x w bytes, non-zero = take
// this pixel out.  grow = G and feather = F are integers, 0 <= G <= 8, 0 <= F <= 8; R = G + F.  Per frame pixel (x, y), in this order:
//   1. Distance (integers).  D2 = the smallest (x - x')^2 + (y - y')^2 over the pixels (x', y') of the frame with remove != 0,
//      |x - x'| <= R and |y - y'| <= R; without one the pixel is far.  Pixels outside the frame hold nothing.
//   2. Weight, alpha in 0 .. 256 (integers).  far: alpha = 0;  D2 <= G * G: alpha = 256;  otherwise with F == 0: alpha = 0;  otherwise
//        D16 = floor(sqrt(256 * D2)), the exact integer root;  E = 16 * (G + F) - D16;
//        alpha = E <= 0 ? 0 : min(256, (256 * E + 8 * F) / (16 * F))          (integer division)
//      256 at distance G, 0 from distance G + F on, 16 steps per pixel between.
//   3. Sample, only where alpha > 0: steps 1 to 4 of fotg_subtract with the same helpers (warp_inside, warp_sat, clampi, warp_taps),
//      except that a NaN in the frame pixel does not disqualify:
//        (u, v) not finite, or mask[i][y][x] != 0:                                                            code 3
//        Xc = (float)(x + ox) + u;  Yc = (float)(y + oy) + v;  !warp_inside(Xc, Yc, W, H):                    code 2
//        plate_code[index[i]] non-zero at any of the four clamped tap pixels of fotg_warp at (Xc, Yc):        code 2
//        s = warp_taps(plate[index[i]], W, H, Xc, Yc);  any channel of s is NaN:                              code 3
//   4. Value, f the frame's pixel.  alpha == 0, or code 2 or 3: dst = f, copied bit for bit.  alpha == 256 and a good sample: dst = s
//      (8-bit: warp_to_u8(s)), code 1.  0 < alpha < 256 and a good sample: code 4, a = (float)alpha * 0.00390625f and per channel
//      dst = f + (s - f) * a, every operation rounded on its own (8-bit: through warp_to_u8).
//      alphabet: 0 untouched, 1 replaced, 2 no plate there (kept), 3 unknown (kept), 4 blended
//   5. Outputs, each optional, at least one: dst (the frames' type and shape), code (n x h x w uint8), alpha (n x h x w int16),
//      stats (n x 8 int64 per frame: [0..4] the pixels of code 0 .. 4, [5] the pixels with alpha == 256 and code 2 or 3 -- the holes,
//      where an object is still visible --, [6] the pixels with remove != 0, [7] the sum of alpha).  stats is cleared by a
//      stream-ordered memset inside the call and accumulated by integer atomics: the same bytes every run.
//   With alpha as the only output nothing is sampled: frames, the plate and the source of the vectors are not read and may be null;
//   alpha == 256 is then the dilation of remove by the disc of radius G (flowonthego_amd.erase.grow_mask).
//
// erase_kernel: one launch, grid (ceil(w / 64), ceil(h / 16), n), 256 threads: a workgroup owns a 64 x 16 tile of one frame.
// Staging: remove for the tile and its halo as bits, one 16-byte LDS word per staged row: 96 columns (the tile's 64 and 16 either
// side, of which those within R are loaded) in three dwords and one of padding, 16 + 2R <= 48 rows.  A wave takes two rows at a
// time with three byte loads per lane and three ballots -- the 64 left columns of either row, then the 32 right columns of both --
// and its first lane writes the two words.  The waves also or their ballots together: a workgroup whose staged area holds no set
// pixel (the common case) copies its tile from frames to dst with 16-byte nontemporal loads and stores where source and
// destination are aligned alike (the bytes before and after the aligned run, and everything otherwise, one by one), stores zero
// code and alpha, and samples nothing.  The copy's loads are issued before the staging's, so that both are in flight together;
// a tile that is not copied has read its frame pixels into the cache early.
// Otherwise the distance is the capped two-pass transform.  Pass 1: per staged row and tile column hd = the horizontal distance to
// the nearest set bit within R (255 without one): the 33 bits around the column are cut from the row's 96, count-trailing-zeros
// finds the nearest to the right, count-leading-zeros the nearest to the left.  An item is four adjacent columns of one row: one
// 16-byte LDS read (the 16 lanes of a row read one address: a broadcast), four hd bytes written as one dword, consecutive lanes to
// consecutive dwords.  Pass 2: thread t owns the four adjacent pixels 4 (t % 16) .. + 3 of tile row t / 16 and takes the minimum of
// hd^2 + dy^2 over the 2R + 1 rows: one dword read per row; a wave's 64 lanes (4 rows x 16 dwords) read 64 consecutive dwords,
// each half of 32 lanes its own 32 banks: no conflicts anywhere.  Why two passes, in LDS reads per thread at R = 16: pass 1 costs
// three 16-byte reads and three dword writes, pass 2 33 dword reads for four pixels; a thread that derived hd itself from the bits
// would read 33 x 16 bytes and run the bit search 132 times instead of 12 (each hd serves the 2R + 1 pixels above and below it);
// a direct search of the (2R + 1)^2 window would test 1089 bits per pixel.
// Only pixels with alpha > 0 touch the vectors and the plate (its taps gathered through L2).  Stores per four pixels: dst through
// warp_store4, code through warp_store_code4, alpha in one 8-byte store, where the span is whole and aligned, elements otherwise.
// Statistics: integer sums per thread, per wave by xor shuffles, per workgroup through LDS, then one 64-bit integer atomic per
// non-zero column per workgroup.  No floating-point atomics, no private memory.
#pragma once
#include "common.h"
#include "flowsrc.hip.h"
#include "plate.hip.h"        // MotionSrc
#include "warp.hip.h"

namespace fotg {

enum { ER_TW = 64, ER_TH = 16, ER_THREADS = 256, ER_MAXG = 8, ER_MAXF = 8, ER_MAXR = ER_MAXG + ER_MAXF, ER_LDH = ER_TH + 2 * ER_MAXR,
       ER_QUADS = ER_TW / 4, ER_NSTAT = 8, ER_NRED = 5, ER_FAR = 255, ER_MAX_DIM = 16384, ER_MAX_ORIGIN = 1 << 20 };

// step 2 of the head of this file; D2 > R^2 stands for a far pixel too (its root is at least 16 R, so E <= 0)
__device__ __forceinline__ unsigned erase_alpha(unsigned D2, int G, int F)
{
  const int R = G + F;
  if (D2 > (unsigned)(R * R)) return 0u;
  if (D2 <= (unsigned)(G * G)) return 256u;
  // G^2 < D2 <= R^2 <= 256, so F > 0.  n <= 2^16: the f32 root is within one of the integer root, the exact products decide
  // (mh_mag's short path, histograms.hip.h)
  const unsigned n = D2 << 8;
  unsigned s = (unsigned)__builtin_amdgcn_sqrtf((float)n);
  s -= __umul24(s, s) > n ? 1u : 0u;
  s += __umul24(s + 1, s + 1) <= n ? 1u : 0u;
  const int E = 16 * R - (int)s;
  if (E <= 0) return 0u;
  const unsigned a = (256u * (unsigned)E + 8u * (unsigned)F) / (16u * (unsigned)F);
  return a > 256u ? 256u : a;
}

// step 3 for frame pixel (x, y) of frame img: 1 and the sample in s, or the code 2 or 3
template <class Src, class T, int NOC>
__device__ __forceinline__ unsigned erase_sample(const Src &flow, const T *__restrict__ plate, const unsigned char *__restrict__ pcode,
                                                 const unsigned char *__restrict__ mask, int img, int x, int y, int w, int h, int W, int H,
                                                 int ox, int oy, float (&s)[NOC])
{
#pragma unroll
  for (int ch = 0; ch < NOC; ++ch) s[ch] = 0.f;
  const long q = (long)img * w * h + (long)y * w + x;
  float u, v;
  flow.at(q, img, x, y, u, v);
  if (!(__builtin_isfinite(u) && __builtin_isfinite(v))) return 3u;
  if (mask && mask[q]) return 3u;
  const float Xc = (float)(x + ox) + u, Yc = (float)(y + oy) + v;
  if (!warp_inside(Xc, Yc, W, H)) return 2u;
  if (pcode) {
    const int xi = warp_sat(floorf(Xc), W), yi = warp_sat(floorf(Yc), H);
    const int x1 = clampi(xi, W), x2 = clampi(xi + 1, W), y1 = clampi(yi, H), y2 = clampi(yi + 1, H);
    if (pcode[(size_t)y1 * W + x1] | pcode[(size_t)y1 * W + x2] | pcode[(size_t)y2 * W + x1] | pcode[(size_t)y2 * W + x2]) return 2u;
  }
  warp_taps<T, NOC>(plate, W, H, Xc, Yc, s);
  bool nan = false;
#pragma unroll
  for (int ch = 0; ch < NOC; ++ch) nan = nan || s[ch] != s[ch];
  return nan ? 3u : 1u;
}

// the thread's nb (<= 4) pixels at f as floats: 16-byte / dword loads where the span is whole and aligned (warp_store4's rule)
template <class T, int NOC>
__device__ __forceinline__ void erase_load4(const T *__restrict__ f, float (&val)[4 * NOC], int nb)
{
  typedef float vf4 __attribute__((ext_vector_type(4)));
  if constexpr (sizeof(T) == 4) {
    if (nb == 4 && (((size_t)f) & 15) == 0) {
#pragma unroll
      for (int k = 0; k < NOC; ++k) {
        const vf4 a = __builtin_nontemporal_load(reinterpret_cast<const vf4 *>(f) + k);
        val[4 * k] = a.x; val[4 * k + 1] = a.y; val[4 * k + 2] = a.z; val[4 * k + 3] = a.w;
      }
      return;
    }
  } else {
    if (nb == 4 && (((size_t)f) & 3) == 0) {
#pragma unroll
      for (int k = 0; k < NOC; ++k) {
        const unsigned a = __builtin_nontemporal_load(reinterpret_cast<const unsigned *>(f) + k);
        val[4 * k] = (float)(a & 255u); val[4 * k + 1] = (float)((a >> 8) & 255u);
        val[4 * k + 2] = (float)((a >> 16) & 255u); val[4 * k + 3] = (float)(a >> 24);
      }
      return;
    }
  }
#pragma unroll
  for (int k = 0; k < 4 * NOC; ++k) {
    val[k] = 0.f;
    if (k < nb * NOC) val[k] = warp_elem(f, (size_t)k);
  }
}

// The copy of a tile, rows x cols pixels at (tx0, ty0) of frame img, from frames to dst by the whole workgroup, in two halves so
// that its loads are in flight together with the staging's: item i is slot v = i % SLOTS of tile row i / SLOTS; a row whose source
// and destination are aligned alike holds nvec < SLOTS aligned 16-byte runs, slots 0 .. nvec - 1, and slot SLOTS - 1 takes the
// bytes around them; the slots of any other row share its bytes one by one.
template <class T, int NOC>
struct EraseCopy {
  enum { PIX = NOC * (int)sizeof(T), SLOTS = ER_TW * PIX / 16 + 1, ITEMS = ER_TH * SLOTS, ITERS = (ITEMS + ER_THREADS - 1) / ER_THREADS };
  typedef unsigned vu4 __attribute__((ext_vector_type(4)));
  const unsigned char *s;
  unsigned char *d;
  int len, head, nvec, v;
  bool row, aligned;

  __device__ __forceinline__ EraseCopy(const T *__restrict__ frames, T *__restrict__ dst, int img, int tx0, int ty0, int cols, int rows, int w,
                                       int h, int i)
  {
    const int r = i / SLOTS;
    v = i - r * SLOTS;
    row = r < rows;
    const size_t off = (((size_t)img * h + (ty0 + (row ? r : 0))) * w + tx0) * PIX;
    s = reinterpret_cast<const unsigned char *>(frames) + off;
    d = reinterpret_cast<unsigned char *>(dst) + off;
    len = cols * PIX;
    aligned = (((size_t)s ^ (size_t)d) & 15) == 0;
    head = (int)((16 - ((size_t)s & 15)) & 15);
    head = head < len ? head : len;
    nvec = (len - head) >> 4;
  }
  __device__ __forceinline__ bool run() const { return row && aligned && v < nvec; }
};

// the first half: the thread's aligned runs into reg, a bit per run that was read
template <class T, int NOC>
__device__ __forceinline__ unsigned erase_copy_load(const T *__restrict__ frames, T *__restrict__ dst, int img, int tx0, int ty0, int cols,
                                                    int rows, int w, int h, typename EraseCopy<T, NOC>::vu4 (&reg)[EraseCopy<T, NOC>::ITERS])
{
  typedef EraseCopy<T, NOC> C;
  unsigned got = 0u;
#pragma unroll
  for (int k = 0; k < C::ITERS; ++k) {
    const int i = (int)threadIdx.x + k * ER_THREADS;
    reg[k] = typename C::vu4{0u, 0u, 0u, 0u};
    if (i < C::ITEMS) {
      const C c(frames, dst, img, tx0, ty0, cols, rows, w, h, i);
      if (c.run()) {
        reg[k] = __builtin_nontemporal_load(reinterpret_cast<const typename C::vu4 *>(c.s + c.head) + c.v);
        got |= 1u << k;
      }
    }
  }
  return got;
}

// the second half: the runs that were read, then the bytes no run covers
template <class T, int NOC>
__device__ __forceinline__ void erase_copy_store(const T *__restrict__ frames, T *__restrict__ dst, int img, int tx0, int ty0, int cols, int rows,
                                                 int w, int h, const typename EraseCopy<T, NOC>::vu4 (&reg)[EraseCopy<T, NOC>::ITERS], unsigned got)
{
  typedef EraseCopy<T, NOC> C;
#pragma unroll
  for (int k = 0; k < C::ITERS; ++k) {
    const int i = (int)threadIdx.x + k * ER_THREADS;
    if (i < C::ITEMS) {
      const C c(frames, dst, img, tx0, ty0, cols, rows, w, h, i);
      if ((got >> k) & 1u) {
        __builtin_nontemporal_store(reg[k], reinterpret_cast<typename C::vu4 *>(c.d + c.head) + c.v);
      } else if (c.row && c.aligned) {
        if (c.v == C::SLOTS - 1) {
          for (int b = 0; b < c.head; ++b) c.d[b] = c.s[b];
          for (int b = c.head + 16 * c.nvec; b < c.len; ++b) c.d[b] = c.s[b];
        }
      } else if (c.row) {
        for (int b = c.v; b < c.len; b += C::SLOTS) c.d[b] = c.s[b];
      }
    }
  }
}

// flow: the vectors frame -> reference; frames: n x h x w x NOC; plates: P x H x W x NOC; idx: n plate indices, validated by the
// host, or null (plate 0 for P == 1, plate img otherwise); pcode: P x H x W bytes or null; mask: n x h x w bytes or null; remove:
// n x h x w bytes; dst: n x h x w x NOC, code: n x h x w bytes, alpha: n x h x w int16, stats: n x 8 (cleared by the host), each or
// null.  With dst, code and stats all null nothing but remove is read.
template <class Src, class T, int NOC>
__global__ __launch_bounds__(ER_THREADS) void erase_kernel(Src flow, const T *__restrict__ frames, const T *__restrict__ plates,
                                                            const int *__restrict__ idx, int P, const unsigned char *__restrict__ pcode,
                                                            const unsigned char *__restrict__ mask, const unsigned char *__restrict__ remove,
                                                            int w, int h, int W, int H, int ox, int oy, int G, int F, T *__restrict__ dst,
                                                            unsigned char *__restrict__ code, short *__restrict__ alpha,
                                                            unsigned long long *__restrict__ stats)
{
  typedef unsigned vu4 __attribute__((ext_vector_type(4)));
  typedef unsigned long long u64;
  __shared__ vu4 er_bits[ER_LDH];                                 // row j: columns tx0 - 16 .. tx0 + 79 of frame row ty0 - R + j
  __shared__ unsigned er_hd[ER_LDH * ER_QUADS];                   // row j, tile columns 4 q .. 4 q + 3: four hd bytes
  __shared__ unsigned er_any[ER_THREADS / FOTG_WAVE];
  __shared__ unsigned er_red[ER_THREADS / FOTG_WAVE][ER_NRED];
  const int img = blockIdx.z, t = threadIdx.x, lane = t % FOTG_WAVE, wave = t / FOTG_WAVE;
  const int tx0 = blockIdx.x * ER_TW, ty0 = blockIdx.y * ER_TH;
  const int R = G + F;
  const unsigned char *__restrict__ rm = remove + (size_t)img * w * h;

  // staging: two rows per wave and step
  auto set = [&](int j, int c) -> bool {
    const int x = tx0 - ER_MAXR + c, y = ty0 - R + j;
    return c >= ER_MAXR - R && c < ER_MAXR + ER_TW + R && x >= 0 && x < w && y >= 0 && y < h && rm[(size_t)y * w + x] != 0;
  };
  // the copy's loads leave first, before it is known whether the tile is copied: one round trip to memory, not two
  const int cols = w - tx0 < ER_TW ? w - tx0 : ER_TW, rows = h - ty0 < ER_TH ? h - ty0 : ER_TH;
  typename EraseCopy<T, NOC>::vu4 creg[EraseCopy<T, NOC>::ITERS];
  unsigned cgot = 0u;
  if (dst) cgot = erase_copy_load<T, NOC>(frames, dst, img, tx0, ty0, cols, rows, w, h, creg);
  u64 seen = 0;
  for (int pr = wave; pr < ER_TH / 2 + R; pr += ER_THREADS / FOTG_WAVE) {
    const int j = 2 * pr;
    const u64 a = __ballot(set(j, lane)), b = __ballot(set(j + 1, lane)), c = __ballot(set(j + (lane >> 5), 64 + (lane & 31)));
    seen |= a | b | c;
    if (lane == 0) {
      er_bits[j] = vu4{(unsigned)a, (unsigned)(a >> 32), (unsigned)c, 0u};
      er_bits[j + 1] = vu4{(unsigned)b, (unsigned)(b >> 32), (unsigned)(c >> 32), 0u};
    }
  }
  if (lane == 0) er_any[wave] = seen != 0 ? 1u : 0u;
  __syncthreads();
  const bool empty = (er_any[0] | er_any[1] | er_any[2] | er_any[3]) == 0u;       // (uniform over the workgroup)

  const int qx = t % ER_QUADS, ty = t / ER_QUADS;
  const int x0 = tx0 + 4 * qx, y = ty0 + ty;
  const int nb = y < h ? (w - x0 < 4 ? (w - x0 < 0 ? 0 : w - x0) : 4) : 0;
  const bool sample = dst || code || stats;
  unsigned al[4] = {0u, 0u, 0u, 0u}, mine = 0u;

  if (empty) {
    if (dst) erase_copy_store<T, NOC>(frames, dst, img, tx0, ty0, cols, rows, w, h, creg, cgot);
  } else {
    // pass 1: the horizontal distances
    for (int i = t; i < (ER_TH + 2 * R) * ER_QUADS; i += ER_THREADS) {
      const vu4 b = er_bits[i / ER_QUADS];
      const int s = 4 * (i % ER_QUADS);
      // the 64 bits from column s on: bit k of the window of column s + m is bit k + m, and stands for dx = k - 16
      const u64 X = s < 32 ? (((u64)b.x | (u64)b.y << 32) >> s) | (((u64)b.z << 32) << (32 - s)) : ((u64)b.y | (u64)b.z << 32) >> (s - 32);
      unsigned out = 0u;
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const u64 win = X >> m;
        const unsigned right = (unsigned)(win >> 16) & 0x1ffffu, left = (unsigned)win & 0x1ffffu;
        const unsigned dr = right ? (unsigned)__builtin_ctz(right) : (unsigned)ER_FAR;
        const unsigned dl = left ? (unsigned)__builtin_clz(left) - 15u : (unsigned)ER_FAR;
        unsigned hd = dl < dr ? dl : dr;
        hd = hd > (unsigned)R ? (unsigned)ER_FAR : hd;
        out |= hd << (8 * m);
      }
      er_hd[i] = out;
    }
    __syncthreads();
    // pass 2: the minimum over the rows
    unsigned D2[4] = {~0u, ~0u, ~0u, ~0u};
    for (int k = 0; k <= 2 * R; ++k) {
      const unsigned wd = er_hd[(ty + k) * ER_QUADS + qx];
      const unsigned dy2 = (unsigned)((k - R) * (k - R));
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const unsigned hd = (wd >> (8 * m)) & 255u;
        const unsigned d = __umul24(hd, hd) + dy2;
        D2[m] = d < D2[m] ? d : D2[m];
      }
    }
#pragma unroll
    for (int m = 0; m < 4; ++m) al[m] = erase_alpha(D2[m], G, F);
    const int col = ER_MAXR + 4 * qx;
    mine = (reinterpret_cast<const unsigned *>(er_bits)[(ty + R) * 4 + (col >> 5)] >> (col & 31)) & 15u;      // remove at the four pixels
  }

  unsigned c01 = 0, c23 = 0, c4h = 0, nrem = 0, asum = 0;
  if (nb > 0) {
    const size_t p0 = ((size_t)img * h + y) * w + x0;
    unsigned cword = 0;
    if (!empty && sample) {                                       // (the first uniform)
      const int pl = idx ? idx[img] : (P == 1 ? 0 : img);
      const T *__restrict__ plate = plates + (size_t)pl * W * H * NOC;
      const unsigned char *__restrict__ pc = pcode ? pcode + (size_t)pl * W * H : nullptr;
      float val[4 * NOC];
      if (dst) {
        erase_load4<T, NOC>(frames + p0 * NOC, val, nb);
      } else {
#pragma unroll
        for (int k = 0; k < 4 * NOC; ++k) val[k] = 0.f;
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        unsigned cd = 0u;
        if (i < nb && al[i] > 0u) {
          float s[NOC];
          cd = erase_sample<Src, T, NOC>(flow, plate, pc, mask, img, x0 + i, y, w, h, W, H, ox, oy, s);
          if (cd == 1u) {
            if (al[i] == 256u) {
#pragma unroll
              for (int ch = 0; ch < NOC; ++ch) val[i * NOC + ch] = s[ch];
            } else {
              cd = 4u;
              const float a = (float)al[i] * 0.00390625f;
#pragma unroll
              for (int ch = 0; ch < NOC; ++ch) val[i * NOC + ch] = val[i * NOC + ch] + (s[ch] - val[i * NOC + ch]) * a;
            }
          }
        }
        cword |= cd << (8 * i);
        if (i < nb) {
          if (cd < 2u) c01 += 1u << (16 * cd); else if (cd < 4u) c23 += 1u << (16 * (cd - 2u)); else c4h += 1u;
          if (al[i] == 256u && (cd == 2u || cd == 3u)) c4h += 1u << 16;
        }
      }
      if (dst) warp_store4<T, NOC>(dst + p0 * NOC, val, nb);
    } else {
      c01 = (unsigned)nb;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (i < nb) { asum += al[i]; nrem += (mine >> i) & 1u; }
    if (code) warp_store_code4(code + p0, cword, nb);
    if (alpha) {
      short *o = alpha + p0;
      if (nb == 4 && (((size_t)o) & 7) == 0) {
        typedef unsigned vu2 __attribute__((ext_vector_type(2)));
        __builtin_nontemporal_store(vu2{al[0] | al[1] << 16, al[2] | al[3] << 16}, reinterpret_cast<vu2 *>(o));
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (i < nb) o[i] = (short)al[i];
      }
    }
  }

  if (stats) {                                                    // (uniform) a workgroup holds at most 1024 pixels: 16-bit halves suffice
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      c01 += __shfl_xor(c01, o, 64); c23 += __shfl_xor(c23, o, 64); c4h += __shfl_xor(c4h, o, 64);
      nrem += __shfl_xor(nrem, o, 64); asum += __shfl_xor(asum, o, 64);
    }
    if (lane == 0) {
      er_red[wave][0] = c01; er_red[wave][1] = c23; er_red[wave][2] = c4h; er_red[wave][3] = nrem; er_red[wave][4] = asum;
    }
    __syncthreads();
    if (t < ER_NSTAT) {
      const int word = t < 6 ? t >> 1 : t - 3;                    // columns 0 .. 5 share three words, 6 and 7 have their own
      u64 tot = 0;
      for (int i = 0; i < ER_THREADS / FOTG_WAVE; ++i) {
        const unsigned v = er_red[i][word];
        tot += t < 6 ? ((t & 1) ? v >> 16 : v & 0xffffu) : v;
      }
      if (tot) atomicAdd(stats + (size_t)img * ER_NSTAT + t, tot);
    }
  }
}

}  // namespace fotg
