// motionblur.hip.h -- motion blur synthesised along a flow (a shutter simulated per frame): the tile-max / neighbour-max
// scatter-as-gather reconstruction filter of McGuire et al. 2012 with the direction test of Guertin et al. 2014, both without depth.
// A pixel's own vector says nothing about what passes over it, so every pixel gathers along the dominant vector D of its
// neighbourhood of tiles and weighs each tap by how far the tap's (or its own) vector reaches along that line.  One f32 multiply per
// component, integers after it; lengths are in 1/16 pixel.  The definition, in order:
//
// 1. Half-vector.  shutter256 in 1 .. 512 is round(256 shutter); s = (float)shutter256 / 32 (exact); hx = (int)rintf(u s),
//    hy = (int)rintf(v s).  A pixel is unknown, H = (0, 0), when (u, v) is not motion_known (|u|, |v| <= 4096; false for a NaN or
//    an infinity) or a mask is given and its byte is non-zero.  len = M(hx, hy), the exact integer root mh_mag of histograms.hip.h;
//    cap16 = 16 max_blur, max_blur in 1 .. 32; if len > cap16 then hx = hx cap16 / len, hy = hy cap16 / len (C integer division:
//    towards zero) and len = M(hx, hy) again.  H is int16 x 2 per pixel.
// 2. Tiles of 32 x 32 pixels, partial at the right and bottom edges.  tilemax = the H of the tile's pixel with the largest
//    hx hx + hy hy, the lowest linear pixel index on a tie.  D(tile) = the tilemax with the largest squared length among the up to
//    nine tiles around it, the first in raster order on a tie.  lenD = M(Dx, Dy).
// 3. Gather, for the pixel X = (x, y) of a tile with D.  lenD < 8: dst = src, code 0, or 3 if X is unknown (the copy path).
//    Otherwise L = (lenD + 15) / 16 (at most 32) and for k = -L .. L, with a = |k|:
//      o_k = (ox, oy): ox = sign(Dx k) ((2 |Dx| a + L) / (2 L)), oy alike (half away from zero: o_-k = -o_k)
//      Y_k = (x + ((ox + 8) >> 4), y + ((oy + 8) >> 4)) (arithmetic shift: the nearest pixel, a half towards +inf), clamped to the
//            frame; the tap is `clamped` when the clamp moved it
//      d_k = lenD a / L
//      r(P) = |Hx(P) Dx + Hy(P) Dy| / lenD                                     (integer division; the reach of P along the line)
//      w_k = clamp(max(r(Y_k), r(X)) + 16 - d_k, 0, 16)                          (so w_0 = 16)
//    8-bit frames, per channel: dst = (2 sum w_k c_k + W) / (2 W), W = sum w_k, in integers.  f32 frames: acc = 0, then
//    acc = acc + (float)w_k c_k for k ascending, every tap (those of weight 0 too), every operation rounded on its own; dst = acc / (float)W.
//    code = the first that applies of: 3, X is unknown; 2, a tap with w_k > 0 was clamped; 1, a tap k != 0 had w_k > 0; 0.
// 4. stats, per image eight int64: the pixels of code 0, 1, 2, 3; the taps with w_k > 0 summed over the pixels of the gather path
//    (k = 0 included; a pixel of the copy path adds none); the tiles that took the copy path; the largest len; 0.
// tests/motionblur_ref.py restates all of this in numpy.
//
// mblur_vectors_kernel<Src> (pass A): grid (tiles across, tiles down, n), 256 threads, one workgroup per tile.  Thread (t % 8, t / 8)
//   owns four adjacent pixels of a tile row: a dense flow leaves in two 16-byte loads, the mask in one 4-byte load, H goes out in two
//   8-byte stores (one by one where the address does not allow it; the fused source evaluates its taps per pixel).  H of an unknown
//   pixel is written as MB_UNKNOWN to the call's own memory, which is how pass B learns of code 3 without reading flow and mask
//   again; `vectors`, the caller's copy, gets (0, 0).  The tile maximum is one integer key per pixel, (squared length << 10) |
//   (1023 - index in the tile): a DPP maximum over the wave, four waves through LDS, and the thread that owns the winning key
//   stores its H.  No atomics.
// mblur_gather_kernel<T, NOC> (pass B): the same grid.  Every thread folds the nine tilemax entries from LDS, so D, lenD and L are
//   workgroup-uniform and live in scalar registers.  Copy path: a tile row is a span of bytes that leaves in 16-byte loads and
//   stores between a head and a tail of single bytes.  Gather path: 2 L + 1 threads write the table of (pixel offset, d_k); the
//   workgroup stages H of the window tile +- ((|Dx| + 8) >> 4, (|Dy| + 8) >> 4) pixels at clamped coordinates into LDS (at most
//   96 x 96 x 4 B = 36 KB, pitch 96 words: the two rows of a wave fall into different halves of the banks), then thread
//   (t % 32, t / 32) walks the taps for its four pixels (rows t / 32 + 8 j): the trip count and the offsets are uniform, the loop has
//   no divergent branch, the divisions by lenD and by W are a v_rcp_f32 estimate settled by one exact product.  Colour is gathered
//   from memory through L2 at the clamped tap, as warp.hip.h gathers its taps.  (-DFOTG_MBLUR_STAGE_COLOUR=1, never in the shipped
//   build, is the variant that lost: the 8-bit colour of the window staged in a second 36 KB of LDS, packed to 4 B per pixel.)
// mblur_fold_kernel: one workgroup per image adds the per-tile partials of pass B into the eight int64 (integers: any order).
#pragma once
#include <type_traits>
#include "common.h"
#include "flowsrc.hip.h"
#include "histograms.hip.h"
#include "motion_model.hip.h"

#ifndef FOTG_MBLUR_STAGE_COLOUR
#define FOTG_MBLUR_STAGE_COLOUR 0
#endif

namespace fotg {

enum { MB_THREADS = 256, MB_TILE = 32, MB_PITCH = 96, MB_MAX_DIM = 16384, MB_MAX_BLUR = 32, MB_MAX_SHUTTER256 = 512, MB_COPY_BELOW = 8,
       MB_NSTAT = 8, MB_TAPS = 2 * MB_MAX_BLUR + 1 };
enum : unsigned { MB_UNKNOWN = 0x00008000u };                // hx = -32768, hy = 0: no vector of the definition (|hx| <= 512)

__device__ __forceinline__ unsigned mblur_pack(int hx, int hy) { return ((unsigned)hy << 16) | ((unsigned)hx & 0xffffu); }
__device__ __forceinline__ int mblur_hx(unsigned p) { return (int)(short)(p & 0xffffu); }
__device__ __forceinline__ int mblur_hy(unsigned p) { return (int)p >> 16; }
__device__ __forceinline__ int mblur_sq(unsigned p) { return mblur_hx(p) * mblur_hx(p) + mblur_hy(p) * mblur_hy(p); }

// step 1 for one pixel: H packed, MB_UNKNOWN for an unknown one
__device__ __forceinline__ unsigned mblur_half(float u, float v, unsigned mk, float s, int cap16)
{
  if (mk != 0 || !motion_known(u, v)) return MB_UNKNOWN;
  int hx = (int)rintf(u * s), hy = (int)rintf(v * s);
  const int len = (int)mh_mag(hx, hy);
  if (len > cap16) { hx = hx * cap16 / len; hy = hy * cap16 / len; }
  return mblur_pack(hx, hy);
}

// a / b for a < 2^22, b >= 1, rb = 1 / (float)b: the f32 quotient is within one of it, the exact product decides
__device__ __forceinline__ unsigned mblur_div(unsigned a, unsigned b, float rb)
{
  unsigned q = (unsigned)((float)a * rb);
  const int r = (int)(a - q * b);
  return r < 0 ? q - 1 : ((unsigned)r >= b ? q + 1 : q);
}

template <int CTRL>
__device__ __forceinline__ int mblur_dpp(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, false); }

// over the wave: quad_perm [1 0 3 2], quad_perm [2 3 0 1], row_half_mirror, row_mirror inside rows of 16, two xor shuffles across
__device__ __forceinline__ int mblur_wave_max(int v)
{
  v = max(v, mblur_dpp<0xB1>(v)); v = max(v, mblur_dpp<0x4E>(v)); v = max(v, mblur_dpp<0x141>(v)); v = max(v, mblur_dpp<0x140>(v));
  v = max(v, __shfl_xor(v, 16, FOTG_WAVE)); v = max(v, __shfl_xor(v, 32, FOTG_WAVE));
  return v;
}
__device__ __forceinline__ int mblur_wave_sum(int v)
{
  v += mblur_dpp<0xB1>(v); v += mblur_dpp<0x4E>(v); v += mblur_dpp<0x141>(v); v += mblur_dpp<0x140>(v);
  v += __shfl_xor(v, 16, FOTG_WAVE); v += __shfl_xor(v, 32, FOTG_WAVE);
  return v;
}

// Pass A.  H: n x h x w packed, the call's own (256-byte aligned); vectors: null or the caller's n x h x w x 2 int16; tilemax: n x
// tiles down x tiles across packed.  vec: bit 0 a dense flow is aligned for 16-byte loads, bit 1 the mask for 4-byte loads, bit 2
// `vectors` for 8-byte stores.
template <class Src>
__global__ __launch_bounds__(MB_THREADS) void mblur_vectors_kernel(Src flow, const unsigned char *__restrict__ mask, int w, int h, float s,
                                                                   int cap16, int vec, unsigned *__restrict__ H,
                                                                   unsigned *__restrict__ vectors, unsigned *__restrict__ tilemax)
{
  __shared__ int wbest[MB_THREADS / FOTG_WAVE];
  const int t = threadIdx.x, tx = t % 8, ty = t / 8, pair = blockIdx.z;
  const int gx0 = (int)blockIdx.x * MB_TILE + 4 * tx, gy = (int)blockIdx.y * MB_TILE + ty;
  int key = -1;
  unsigned win = 0;
  if (gy < h && gx0 < w) {
    const size_t row = ((size_t)pair * h + gy) * w;
    const bool whole = gx0 + 4 <= w, even = whole && ((row + gx0) & 1) == 0;
    float u[4], v[4];
    bool got = false;
    if constexpr (std::is_same<Src, DenseSrc>::value) {
      if (even && (vec & 1)) {
        const float4 *f = reinterpret_cast<const float4 *>(flow.flow + 2 * (row + gx0));
        const float4 a = f[0], b = f[1];
        u[0] = a.x; v[0] = a.y; u[1] = a.z; v[1] = a.w; u[2] = b.x; v[2] = b.y; u[3] = b.z; v[3] = b.w;
        got = true;
      }
    }
    if (!got) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int cx = gx0 + q < w ? gx0 + q : w - 1;
        flow.at((long)(row + cx), pair, cx, gy, u[q], v[q]);
      }
    }
    unsigned mk = 0;
    if (mask) {
      if (whole && (vec & 2) && ((row + gx0) & 3) == 0) mk = *reinterpret_cast<const unsigned *>(mask + row + gx0);
      else {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int cx = gx0 + q < w ? gx0 + q : w - 1;
          mk |= (unsigned)mask[row + cx] << (8 * q);
        }
      }
    }
    unsigned hp[4], hc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      hp[q] = mblur_half(u[q], v[q], (mk >> (8 * q)) & 0xffu, s, cap16);
      hc[q] = hp[q] == MB_UNKNOWN ? 0u : hp[q];
      const int k = (mblur_sq(hc[q]) << 10) | (MB_TILE * MB_TILE - 1 - (ty * MB_TILE + 4 * tx + q));
      if (gx0 + q < w && k > key) { key = k; win = hc[q]; }
    }
    if (even) {
      uint2 *o = reinterpret_cast<uint2 *>(H + row + gx0);
      o[0] = make_uint2(hp[0], hp[1]); o[1] = make_uint2(hp[2], hp[3]);
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (gx0 + q < w) H[row + gx0 + q] = hp[q];
    }
    if (vectors) {
      if (even && (vec & 4)) {
        uint2 *o = reinterpret_cast<uint2 *>(vectors + row + gx0);
        o[0] = make_uint2(hc[0], hc[1]); o[1] = make_uint2(hc[2], hc[3]);
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (gx0 + q < w) vectors[row + gx0 + q] = hc[q];
      }
    }
  }
  const int wmax = mblur_wave_max(key);
  if (t % FOTG_WAVE == 0) wbest[t / FOTG_WAVE] = wmax;
  __syncthreads();
  const int best = max(max(wbest[0], wbest[1]), max(wbest[2], wbest[3]));
  if (key == best && key >= 0)                               // the index is part of the key: one thread
    tilemax[((size_t)pair * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = win;
}

// Pass B.  part: null or n x tiles x MB_NSTAT ints, the tile's part of the statistics.  vec: bit 3 src and dst are both aligned for
// 16-byte access (the copy path).
template <class T, int NOC>
__global__ __launch_bounds__(MB_THREADS) void mblur_gather_kernel(const T *__restrict__ src, const unsigned *__restrict__ H,
                                                                  const unsigned *__restrict__ tilemax, int w, int h, int vec,
                                                                  T *__restrict__ dst, unsigned char *__restrict__ code, int *__restrict__ part)
{
  __shared__ unsigned sh[MB_PITCH * MB_PITCH];               // H of the window, (0, 0) for an unknown pixel
  constexpr bool STAGE = FOTG_MBLUR_STAGE_COLOUR != 0 && std::is_same<T, unsigned char>::value;
  __shared__ unsigned scol[STAGE ? MB_PITCH * MB_PITCH : 1];  // (the variant: the window's colour, channel c in byte c)
  __shared__ int stab[MB_TAPS];                              // tap k - L: d_k << 16 | (pixel offset y & 255) << 8 | (pixel offset x & 255)
  __shared__ unsigned snine[9];
  __shared__ int sstat[3];
  const int t = threadIdx.x, pair = blockIdx.z, bx = blockIdx.x, by = blockIdx.y, tw = gridDim.x, th = gridDim.y;
  const int X0 = bx * MB_TILE, Y0 = by * MB_TILE;
  const size_t img = (size_t)pair * h * w, tile = ((size_t)pair * th + by) * tw + bx;
  if (t < 9) {
    const int nx = bx + t % 3 - 1, ny = by + t / 3 - 1;
    snine[t] = (nx >= 0 && nx < tw && ny >= 0 && ny < th) ? tilemax[((size_t)pair * th + ny) * tw + nx] : 0u;
  }
  if (t < 3) sstat[t] = 0;
  __syncthreads();
  unsigned dp = snine[0];
#pragma unroll
  for (int i = 1; i < 9; ++i) {
    const unsigned c = snine[i];
    if (mblur_sq(c) > mblur_sq(dp)) dp = c;
  }
  dp = (unsigned)__builtin_amdgcn_readfirstlane((int)dp);
  const int Dx = mblur_hx(dp), Dy = mblur_hy(dp), lenD = (int)mh_mag(Dx, Dy);
  const int tx = t % MB_TILE, ty0 = t / MB_TILE, x = X0 + tx;
  const bool want_code = code != nullptr || part != nullptr;

  if (lenD < MB_COPY_BELOW) {                                // ---- the copy path (workgroup-uniform)
    const int rows = min(MB_TILE, h - Y0), r = t / 8, j = t % 8;
    if (r < rows) {
      const size_t nbytes = (size_t)min(MB_TILE, w - X0) * NOC * sizeof(T);
      const size_t off = (img + (size_t)(Y0 + r) * w + X0) * NOC * sizeof(T), end = off + nbytes;
      const unsigned char *sb = reinterpret_cast<const unsigned char *>(src);
      unsigned char *db = reinterpret_cast<unsigned char *>(dst);
      size_t hend = end, tstart = end;                       // without 16-byte alignment everything is head
      if (vec & 8) {
        const size_t a0 = (off + 15) & ~(size_t)15, a1 = end & ~(size_t)15;
        hend = a0 < end ? a0 : end;
        tstart = a1 > hend ? a1 : hend;
        for (size_t a = a0 + 16 * (size_t)j; a + 16 <= a1; a += 16 * 8)
          *reinterpret_cast<uint4 *>(db + a) = *reinterpret_cast<const uint4 *>(sb + a);
      }
      for (size_t a = off + j; a < hend; a += 8) db[a] = sb[a];
      for (size_t a = tstart + j; a < end; a += 8) db[a] = sb[a];
    }
    if (want_code) {
      int n0 = 0, n3 = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int y = Y0 + ty0 + 8 * q;
        if (x < w && y < h) {
          const size_t p = img + (size_t)y * w + x;
          const bool unk = H[p] == MB_UNKNOWN;
          if (code) code[p] = unk ? 3 : 0;
          n0 += unk ? 0 : 1; n3 += unk ? 1 : 0;
        }
      }
      if (part) {
        n0 = mblur_wave_sum(n0); n3 = mblur_wave_sum(n3);
        if (t % FOTG_WAVE == 0) { atomicAdd(&sstat[0], n0); atomicAdd(&sstat[1], n3); }
        __syncthreads();
        if (t < MB_NSTAT)
          part[tile * MB_NSTAT + t] = t == 0 ? sstat[0] : t == 3 ? sstat[1] : t == 5 ? 1 : t == 6 ? (int)mh_mag(mblur_hx(snine[4]), mblur_hy(snine[4])) : 0;
      }
    }
    return;
  }

  // ---- the gather path
  const int L = (lenD + 15) >> 4, aDx = Dx < 0 ? -Dx : Dx, aDy = Dy < 0 ? -Dy : Dy;
  const int Rx = (aDx + 8) >> 4, Ry = (aDy + 8) >> 4;
  if (t <= 2 * L) {
    const int k = t - L, a = k < 0 ? -k : k;
    int ox = (2 * aDx * a + L) / (2 * L), oy = (2 * aDy * a + L) / (2 * L);
    if ((Dx < 0) != (k < 0)) ox = -ox;
    if ((Dy < 0) != (k < 0)) oy = -oy;
    stab[t] = ((lenD * a / L) << 16) | ((((oy + 8) >> 4) & 255) << 8) | (((ox + 8) >> 4) & 255);
  }
  {
    const int WW = MB_TILE + 2 * Rx, WH = MB_TILE + 2 * Ry, lane = t % FOTG_WAVE;
    for (int ly = t / FOTG_WAVE; ly < WH; ly += MB_THREADS / FOTG_WAVE) {
      const int gy = min(max(Y0 - Ry + ly, 0), h - 1);
      for (int lx = lane; lx < WW; lx += FOTG_WAVE) {
        const int gx = min(max(X0 - Rx + lx, 0), w - 1);
        const unsigned v = H[img + (size_t)gy * w + gx];
        sh[ly * MB_PITCH + lx] = v == MB_UNKNOWN ? 0u : v;
        if constexpr (STAGE) {
          const T *c = src + (img + (size_t)gy * w + gx) * NOC;
          unsigned pk = 0;
#pragma unroll
          for (int ch = 0; ch < NOC; ++ch) pk |= (unsigned)c[ch] << (8 * ch);
          scol[ly * MB_PITCH + lx] = pk;
        }
      }
    }
  }
  __syncthreads();

  const float rD = __builtin_amdgcn_rcpf((float)lenD);
  using Acc = typename std::conditional<std::is_same<T, float>::value, float, int>::type;
  Acc acc[4][NOC];
  int W[4], rX[4], taps[4], flags[4];                        // flags: bit 0 a tap k != 0 with weight, bit 1 a clamped tap with weight
#pragma unroll
  for (int q = 0; q < 4; ++q) {
#pragma unroll
    for (int c = 0; c < NOC; ++c) acc[q][c] = 0;
    const unsigned hv = sh[(ty0 + 8 * q + Ry) * MB_PITCH + tx + Rx];
    const int dot = mblur_hx(hv) * Dx + mblur_hy(hv) * Dy;
    rX[q] = (int)mblur_div((unsigned)(dot < 0 ? -dot : dot), (unsigned)lenD, rD);
    W[q] = 0; taps[q] = 0; flags[q] = 0;
  }
  for (int k = 0; k <= 2 * L; ++k) {
    const int e = __builtin_amdgcn_readfirstlane(stab[k]);
    const int dxp = (int)(signed char)(e & 255), dyp = (int)(signed char)((e >> 8) & 255), dk = e >> 16;
    const int off = k != L ? 1 : 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int ly = ty0 + 8 * q;
      const unsigned hv = sh[(ly + Ry + dyp) * MB_PITCH + tx + Rx + dxp];
      const int dot = mblur_hx(hv) * Dx + mblur_hy(hv) * Dy;
      const int rY = (int)mblur_div((unsigned)(dot < 0 ? -dot : dot), (unsigned)lenD, rD);
      const int wk = min(max(max(rY, rX[q]) + 16 - dk, 0), 16);
      const int px = x + dxp, py = Y0 + ly + dyp;
      const int cx = min(max(px, 0), w - 1), cy = min(max(py, 0), h - 1);
      const int on = wk > 0 ? 1 : 0;
      flags[q] |= (on & off) | ((on & ((cx != px || cy != py) ? 1 : 0)) << 1);
      taps[q] += on;
      W[q] += wk;
      if constexpr (STAGE) {
        const unsigned pk = scol[(ly + Ry + dyp) * MB_PITCH + tx + Rx + dxp];
#pragma unroll
        for (int ch = 0; ch < NOC; ++ch) acc[q][ch] += wk * (int)((pk >> (8 * ch)) & 255u);
      } else {
        const T *c = src + (img + (size_t)cy * w + cx) * NOC;
#pragma unroll
        for (int ch = 0; ch < NOC; ++ch) {
          if constexpr (std::is_same<T, float>::value) acc[q][ch] = acc[q][ch] + (float)wk * c[ch];
          else acc[q][ch] += wk * (int)c[ch];
        }
      }
    }
  }
  int n01 = 0, n23 = 0, nt = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int y = Y0 + ty0 + 8 * q;
    if (x < w && y < h) {
      const size_t p = img + (size_t)y * w + x;
      T *o = dst + p * NOC;
      if constexpr (std::is_same<T, float>::value) {
        const float fW = (float)W[q];
#pragma unroll
        for (int ch = 0; ch < NOC; ++ch) o[ch] = acc[q][ch] / fW;
      } else {
        const unsigned W2 = 2u * (unsigned)W[q];
        const float rW = __builtin_amdgcn_rcpf((float)W2);
#pragma unroll
        for (int ch = 0; ch < NOC; ++ch) o[ch] = (T)mblur_div(2u * (unsigned)acc[q][ch] + (unsigned)W[q], W2, rW);
      }
      if (want_code) {
        const int cd = H[p] == MB_UNKNOWN ? 3 : (flags[q] & 2) ? 2 : (flags[q] & 1);
        if (code) code[p] = (unsigned char)cd;
        n01 += cd == 0 ? 1 : cd == 1 ? 1 << 16 : 0;
        n23 += cd == 2 ? 1 : cd == 3 ? 1 << 16 : 0;
        nt += taps[q];
      }
    }
  }
  if (part) {
    n01 = mblur_wave_sum(n01); n23 = mblur_wave_sum(n23); nt = mblur_wave_sum(nt);
    if (t % FOTG_WAVE == 0) { atomicAdd(&sstat[0], n01); atomicAdd(&sstat[1], n23); atomicAdd(&sstat[2], nt); }
    __syncthreads();
    if (t < MB_NSTAT) {
      const int a = sstat[0], b = sstat[1];
      part[tile * MB_NSTAT + t] = t == 0 ? a & 0xffff : t == 1 ? a >> 16 : t == 2 ? b & 0xffff : t == 3 ? b >> 16 : t == 4 ? sstat[2]
                                  : t == 6 ? (int)mh_mag(mblur_hx(snine[4]), mblur_hy(snine[4])) : 0;
    }
  }
}

// stats[image][c] = the sum over the image's tiles of part[.][c]; column 6 is a maximum
__global__ __launch_bounds__(MB_THREADS) void mblur_fold_kernel(const int *__restrict__ part, int tiles, long long *__restrict__ stats)
{
  __shared__ long long sm[MB_NSTAT][MB_THREADS];
  const int t = threadIdx.x;
  const int *p = part + (size_t)blockIdx.x * tiles * MB_NSTAT;
  long long a[MB_NSTAT];
#pragma unroll
  for (int c = 0; c < MB_NSTAT; ++c) a[c] = 0;
  for (int i = t; i < tiles; i += MB_THREADS) {
#pragma unroll
    for (int c = 0; c < MB_NSTAT; ++c) {
      const long long v = p[(size_t)i * MB_NSTAT + c];
      a[c] = c == 6 ? (v > a[c] ? v : a[c]) : a[c] + v;
    }
  }
#pragma unroll
  for (int c = 0; c < MB_NSTAT; ++c) sm[c][t] = a[c];
  __syncthreads();
  for (int s = MB_THREADS / 2; s > 0; s >>= 1) {
    if (t < s) {
#pragma unroll
      for (int c = 0; c < MB_NSTAT; ++c) {
        const long long v = sm[c][t + s];
        sm[c][t] = c == 6 ? (v > sm[c][t] ? v : sm[c][t]) : sm[c][t] + v;
      }
    }
    __syncthreads();
  }
  if (t < MB_NSTAT) stats[(size_t)blockIdx.x * MB_NSTAT + t] = sm[t][0];
}

}  // namespace fotg
