// subtract.hip.h -- background subtraction against a plate, with two thresholds for hysteresis (include/fotg.h fotg_subtract has the
// definition).  n frames of w x h, P plates on a W x H canvas with integer origin (ox, oy) whose pixel (X, Y) is the reference
// coordinate (X - ox, Y - oy) as in fotg_plate; index[i] is the plate of frame i.  The vector frame i -> reference at frame pixel
// (x, y) comes from a dense flow (n, h, w, 2), from six f64 parameters per frame,
// motion_predict(motion_coef(P_i, w, h), 2x - (w-1), 2y - (h-1)), or from a context's coarse flows.  Per frame pixel, every f32
// operation rounded on its own, in this order; taps, warp_inside, warp_sat and clampi are fotg_warp's (warp.hip.h):
//
//   1. (u, v) not finite, or mask[i][y][x] != 0:                                                           code 3
//   2. Xc = (float)(x + ox) + u;  Yc = (float)(y + oy) + v;  !warp_inside(Xc, Yc, W, H):                   code 2
//   3. plate_code[index[i]] non-zero at any of the four clamped tap pixels of fotg_warp at (Xc, Yc):       code 2
//   4. s = warp_taps(plate[index[i]], W, H, Xc, Yc);  any channel of s or of the frame pixel f is NaN:     code 3
//   5. otherwise the pixel is admissible:
//        d  = 0;  per channel in order: e = fabsf(f_ch - s_ch);  d = e > d ? e : d       (the frame value converted to float, the
//                                                                                          taps of an 8-bit plate left unrounded)
//        Dq = (int)(fminf(d * 16.f, 32767.f) + 0.5f)                   (1/16 grey levels, saturating at 2047.9 levels)
//   window r in {0, 1, 2} (1 x 1, 3 x 3, 5 x 5), over the pixels of the frame within the window:
//        S = sum of Dq over the admissible pixels,  C = their number                      (integers: no order matters)
//   L = lrintf(16 low), Hh = lrintf(16 high), 0 <= L <= Hh <= 32767
//   code of an admissible pixel: S >= Hh * C ? 4 : (S >= L * C ? 1 : 0)
//   alphabet: 0 background, 1 foreground, 2 no plate there, 3 unknown, 4 strong foreground
//   diff = Dq (0 where inadmissible);  evidence = (code == 4 ? 1 : 0, Dq / 16) ((0, 0) where inadmissible)
//   stats (7 x int64 per frame): pixels of code 0 .. 4, sum of Dq over admissible pixels, sum of Dq over pixels of code 1 or 4
//
// subtract_kernel: one launch, grid (ceil(w / 64), ceil(h / 16), n), 256 threads: a workgroup owns a 64 x 16 tile of one frame.
// Phase 1 stages one 32-bit word per position of the tile plus a halo of r pixels (at most 68 x 20 words, row stride 68) in LDS:
// Dq | 1 << 24 for an admissible pixel, code << 30 (code 2 or 3) otherwise; a halo position is evaluated exactly as an interior
// one (its own vector, its own taps gathered through L2), a position outside the frame is inadmissible.  After the one barrier
// thread t classifies the four adjacent pixels 4 (t % 16) .. + 3 of tile row t / 16.  It reads the 2r + 1 window rows as two
// 16-byte LDS reads each (the row stride of 68 words keeps them aligned and moves consecutive rows by one 16-byte slot) and adds
// the words masked to their low 30 bits: the low 24 bits of the sum are S (at most 25 x 32767), bits 24 .. 28 are C.  The window
// is summed directly, not separably: with four pixels per thread the 5 x 5 window costs ten 16-byte reads, a row-sum plane would
// cost as many reads plus its writes and a second barrier.  Stores per four pixels: the code in one 4-byte store, diff
// in one 8-byte store, evidence in two 16-byte stores, where the span is whole and aligned, elements otherwise.
// Statistics: integer sums per thread, per wave by xor shuffles, per workgroup through LDS, then one 64-bit integer atomic per
// column per workgroup into stats, which the host clears by a stream-ordered memset; integer addition is exact in any order, so the
// result is the same every run.  No floating-point atomics, no private memory.
#pragma once
#include "common.h"
#include "flowsrc.hip.h"
#include "plate.hip.h"        // MotionSrc
#include "warp.hip.h"

namespace fotg {

enum { SUB_TW = 64, SUB_TH = 16, SUB_THREADS = 256, SUB_MAXR = 2, SUB_LDW = SUB_TW + 2 * SUB_MAXR, SUB_LDH = SUB_TH + 2 * SUB_MAXR,
       SUB_NSTAT = 7, SUB_MAX_DIM = 16384, SUB_MAX_ORIGIN = 1 << 20, SUB_MAXQ = 32767 };
enum : unsigned { SUB_ONE = 1u << 24, SUB_SUM_MASK = 0x3fffffffu, SUB_S_MASK = 0xffffffu };

// the staged word of frame pixel (x, y) of frame img: steps 1 to 5 of the head of this file
template <class Src, class T, int NOC>
__device__ __forceinline__ unsigned subtract_word(const Src &flow, const T *__restrict__ frames, const T *__restrict__ plate,
                                                  const unsigned char *__restrict__ pcode, const unsigned char *__restrict__ mask,
                                                  int img, int x, int y, int w, int h, int W, int H, int ox, int oy)
{
  const long q = (long)img * w * h + (long)y * w + x;
  float u, v;
  flow.at(q, img, x, y, u, v);
  if (!(__builtin_isfinite(u) && __builtin_isfinite(v))) return 3u << 30;
  if (mask && mask[q]) return 3u << 30;
  const float Xc = (float)(x + ox) + u, Yc = (float)(y + oy) + v;
  if (!warp_inside(Xc, Yc, W, H)) return 2u << 30;
  if (pcode) {
    const int xi = warp_sat(floorf(Xc), W), yi = warp_sat(floorf(Yc), H);
    const int x1 = clampi(xi, W), x2 = clampi(xi + 1, W), y1 = clampi(yi, H), y2 = clampi(yi + 1, H);
    if (pcode[(size_t)y1 * W + x1] | pcode[(size_t)y1 * W + x2] | pcode[(size_t)y2 * W + x1] | pcode[(size_t)y2 * W + x2]) return 2u << 30;
  }
  float s[NOC];
  warp_taps<T, NOC>(plate, W, H, Xc, Yc, s);
  float d = 0.f;
  bool nan = false;
#pragma unroll
  for (int ch = 0; ch < NOC; ++ch) {
    const float f = warp_elem(frames, (size_t)q * NOC + ch);
    nan = nan || s[ch] != s[ch] || f != f;
    const float e = fabsf(f - s[ch]);
    d = e > d ? e : d;
  }
  if (nan) return 3u << 30;
  return (unsigned)(int)(fminf(d * 16.f, 32767.f) + 0.5f) | SUB_ONE;
}

// flow: the vectors frame -> reference; frames: n x h x w x NOC; plates: P x H x W x NOC; idx: n plate indices, validated by the
// host, or null (plate 0 for P == 1, plate img otherwise); pcode: P x H x W bytes or null; mask: n x h x w bytes or null;
// code: n x h x w bytes, diff: n x h x w int16, evidence: n x h x w x 2 f32, stats: n x 7 (cleared by the host), each or null.
template <class Src, class T, int NOC>
__global__ __launch_bounds__(SUB_THREADS) void subtract_kernel(Src flow, const T *__restrict__ frames, const T *__restrict__ plates,
                                                               const int *__restrict__ idx, int P, const unsigned char *__restrict__ pcode,
                                                               const unsigned char *__restrict__ mask, int w, int h, int W, int H, int ox,
                                                               int oy, int r, int L, int Hh, unsigned char *__restrict__ code,
                                                               short *__restrict__ diff, float *__restrict__ evidence,
                                                               unsigned long long *__restrict__ stats)
{
  typedef unsigned vu4 __attribute__((ext_vector_type(4)));
  typedef float vf4 __attribute__((ext_vector_type(4)));
  __shared__ vu4 sub_tile4[SUB_LDH * SUB_LDW / 4];
  __shared__ unsigned sub_red[SUB_THREADS / FOTG_WAVE][5];
  unsigned *tile = reinterpret_cast<unsigned *>(sub_tile4);
  const int img = blockIdx.z, t = threadIdx.x;
  const int tx0 = blockIdx.x * SUB_TW, ty0 = blockIdx.y * SUB_TH;
  const int pl = idx ? idx[img] : (P == 1 ? 0 : img);
  const T *__restrict__ plate = plates + (size_t)pl * W * H * NOC;
  const unsigned char *__restrict__ pc = pcode ? pcode + (size_t)pl * W * H : nullptr;

  // phase 1: the tile and its halo
  const int pw = SUB_TW + 2 * r, npos = pw * (SUB_TH + 2 * r);
  for (int p = t; p < npos; p += SUB_THREADS) {
    const int ly = p / pw, lx = p - ly * pw;
    const int x = tx0 - r + lx, y = ty0 - r + ly;
    unsigned word = 2u << 30;                                     // outside the frame: inadmissible, never a centre
    if (x >= 0 && x < w && y >= 0 && y < h) word = subtract_word<Src, T, NOC>(flow, frames, plate, pc, mask, img, x, y, w, h, W, H, ox, oy);
    tile[ly * SUB_LDW + lx] = word;
  }
  __syncthreads();

  // phase 2: the window sums and the codes of four adjacent pixels
  const int qx = t % (SUB_TW / 4), ty = t / (SUB_TW / 4);
  unsigned win[4] = {0u, 0u, 0u, 0u}, own[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int dy = 0; dy <= 2 * SUB_MAXR; ++dy) {
    if (dy <= 2 * r) {                                            // (uniform)
      const vu4 a = sub_tile4[((ty + dy) * SUB_LDW + 4 * qx) / 4], b = sub_tile4[((ty + dy) * SUB_LDW + 4 * qx) / 4 + 1];
      const unsigned e[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int dx = 0; dx <= 2 * SUB_MAXR; ++dx)
          if (dx <= 2 * r) win[i] += e[i + dx] & SUB_SUM_MASK;
        if (dy == r) own[i] = r == 0 ? e[i] : (r == 1 ? e[i + 1] : e[i + 2]);
      }
    }
  }

  const int x0 = tx0 + 4 * qx, y = ty0 + ty;
  const int nb = y < h ? (w - x0 < 4 ? (w - x0 < 0 ? 0 : w - x0) : 4) : 0;
  unsigned c01 = 0, c23 = 0, c4 = 0, sum_all = 0, sum_fg = 0, cword = 0;
  unsigned dq[4];
  float strong[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    unsigned cd = own[i] >> 30;
    dq[i] = 0u;
    if (cd == 0) {
      dq[i] = own[i] & 0xffffu;
      const int S = (int)(win[i] & SUB_S_MASK), C = (int)(win[i] >> 24);
      cd = S >= Hh * C ? 4u : (S >= L * C ? 1u : 0u);
    }
    strong[i] = cd == 4 ? 1.f : 0.f;
    cword |= cd << (8 * i);
    if (i < nb) {
      if (cd < 2) c01 += 1u << (16 * cd); else if (cd < 4) c23 += 1u << (16 * (cd - 2)); else c4 += 1u;
      sum_all += dq[i];
      if (cd == 1 || cd == 4) sum_fg += dq[i];
    }
  }
  if (nb > 0) {
    const size_t p0 = ((size_t)img * h + y) * w + x0;
    if (code) warp_store_code4(code + p0, cword, nb);
    if (diff) {
      short *o = diff + p0;
      if (nb == 4 && (((size_t)o) & 7) == 0) {
        typedef unsigned vu2 __attribute__((ext_vector_type(2)));
        __builtin_nontemporal_store(vu2{dq[0] | dq[1] << 16, dq[2] | dq[3] << 16}, reinterpret_cast<vu2 *>(o));
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (i < nb) o[i] = (short)dq[i];
      }
    }
    if (evidence) {
      float *o = evidence + 2 * p0;
      const float lv[4] = {(float)dq[0] * 0.0625f, (float)dq[1] * 0.0625f, (float)dq[2] * 0.0625f, (float)dq[3] * 0.0625f};
      if (nb == 4 && (((size_t)o) & 15) == 0) {
        __builtin_nontemporal_store(vf4{strong[0], lv[0], strong[1], lv[1]}, reinterpret_cast<vf4 *>(o));
        __builtin_nontemporal_store(vf4{strong[2], lv[2], strong[3], lv[3]}, reinterpret_cast<vf4 *>(o) + 1);
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (i < nb) { o[2 * i] = strong[i]; o[2 * i + 1] = lv[i]; }
      }
    }
  }

  if (stats) {                                                    // (uniform) a workgroup holds at most 1024 pixels: 32 bits suffice
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      c01 += __shfl_xor(c01, o, 64); c23 += __shfl_xor(c23, o, 64); c4 += __shfl_xor(c4, o, 64);
      sum_all += __shfl_xor(sum_all, o, 64); sum_fg += __shfl_xor(sum_fg, o, 64);
    }
    const int wave = t / FOTG_WAVE;
    if (t % FOTG_WAVE == 0) {
      sub_red[wave][0] = c01; sub_red[wave][1] = c23; sub_red[wave][2] = c4; sub_red[wave][3] = sum_all; sub_red[wave][4] = sum_fg;
    }
    __syncthreads();
    if (t < SUB_NSTAT) {
      const int word = t < 4 ? t >> 1 : t - 2;                    // columns 0, 1 in word 0, 2, 3 in word 1, then one word each
      unsigned long long tot = 0;
      for (int i = 0; i < SUB_THREADS / FOTG_WAVE; ++i) {
        const unsigned v = sub_red[i][word];
        tot += t < 4 ? ((t & 1) ? v >> 16 : v & 0xffffu) : v;
      }
      if (tot) atomicAdd(stats + (size_t)img * SUB_NSTAT + t, tot);
    }
  }
}

}  // namespace fotg
