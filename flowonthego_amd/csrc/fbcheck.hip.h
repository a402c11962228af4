// fbcheck.hip.h -- forward-backward consistency of a flow pair (Sundaram, Brox & Keutzer, ECCV 2010): the dense analogue of
// kroeger's usefbcon merge.  Per pixel (x, y) of a w x h pair (F, B), f32, separately rounded, in exactly this order:
//   (u, v) = F[y][x]; non-finite                                         -> 3 (unknown)
//   X = (float)x + u, Y = (float)y + v; !(0 <= X <= w-1 && 0 <= Y <= h-1) -> 2 (leaves the frame)
//   x0 = min((int)floorf(X), w-1), x1 = min(x0+1, w-1), ax = X - (float)x0 (y0, y1, ay alike)
//   per channel: r0 = B[y0][x0] (1-ax) + B[y0][x1] ax; r1 = B[y1][x0] (1-ax) + B[y1][x1] ax; b = r0 (1-ay) + r1 ay
//   du = u + bu, dv = v + bv; lhs = du du + dv dv; rhs = alpha1 ((u u + v v) + (bu bu + bv bv)) + alpha2
//   lhs < rhs -> 0 (consistent), else 1 (occluded / inconsistent; a NaN in B lands here)
// tests/fbcheck_ref.py restates it in numpy float32; the build's -ffp-contract=off keeps the two equal bit for bit.
//
// One launch per call: grid (blocks per image, n, 2 directions).  Direction 0 checks F against B into `mask`, direction 1 B
// against F into `mask_bw`.  Thread q of an image covers its pixels 4q .. 4q+3 and writes them as one dword when the image's
// row of bytes is dword aligned (w * h % 4 == 0: every operating-point frame), bytes otherwise.  Per image and direction the
// four code counts are summed per thread, per wave (shuffles) and per workgroup (LDS), then added with one integer atomicAdd
// per workgroup and code: integer sums in any order, so deterministic.
// Sources (flowsrc.hip.h): DenseSrc reads a flow, UpsampleSrc evaluates upsample_crop4_kernel's value at the pixel and at each
// of the four integer neighbours of (X, Y), so the fused form equals the check of fotg_upsample_crop's outputs byte for byte.
// The backward samples land anywhere in the frame; they are gathered through L2.
#pragma once
#include "common.h"
#include "flowsrc.hip.h"

namespace fotg {

enum { FB_NCODE = 4 };

// the bilinear sample of flow B (plane `pair`, first pixel `base`) at (X, Y), 0 <= X <= w-1 and 0 <= Y <= h-1: the four clamped
// taps and the three lerps of the head of this file.  Shared with chain.hip.h, which follows a position through T such samples.
template <class Src>
__device__ __forceinline__ void fb_sample(const Src &B, int pair, long base, float X, float Y, int w, int h, float &bu, float &bv)
{
  int x0 = (int)floorf(X), y0 = (int)floorf(Y);
  x0 = x0 < w - 1 ? x0 : w - 1;
  y0 = y0 < h - 1 ? y0 : h - 1;
  const int x1 = x0 + 1 < w - 1 ? x0 + 1 : w - 1, y1 = y0 + 1 < h - 1 ? y0 + 1 : h - 1;
  const float ax = X - (float)x0, ay = Y - (float)y0;
  float u00, v00, u01, v01, u10, v10, u11, v11;
  B.at(base + (long)y0 * w + x0, pair, x0, y0, u00, v00);
  B.at(base + (long)y0 * w + x1, pair, x1, y0, u01, v01);
  B.at(base + (long)y1 * w + x0, pair, x0, y1, u10, v10);
  B.at(base + (long)y1 * w + x1, pair, x1, y1, u11, v11);
  const float r0u = u00 * (1.f - ax) + u01 * ax, r1u = u10 * (1.f - ax) + u11 * ax;
  const float r0v = v00 * (1.f - ax) + v01 * ax, r1v = v10 * (1.f - ax) + v11 * ax;
  bu = r0u * (1.f - ay) + r1u * ay; bv = r0v * (1.f - ay) + r1v * ay;
}

// the inequality: (u, v) and the vector (bu, bv) sampled at its target agree
__device__ __forceinline__ bool fb_consistent(float u, float v, float bu, float bv, float alpha1, float alpha2)
{
  const float du = u + bu, dv = v + bv;
  const float lhs = du * du + dv * dv;
  const float rhs = alpha1 * ((u * u + v * v) + (bu * bu + bv * bv)) + alpha2;
  return lhs < rhs;
}

template <class Src>
__device__ __forceinline__ unsigned fb_code(const Src &F, const Src &B, int pair, int x, int y, int w, int h, long base,
                                            float alpha1, float alpha2)
{
  float u, v;
  F.at(base + (long)y * w + x, pair, x, y, u, v);
  if (!__builtin_isfinite(u) || !__builtin_isfinite(v)) return 3;
  const float X = (float)x + u, Y = (float)y + v;
  if (!(X >= 0.f && X <= (float)(w - 1) && Y >= 0.f && Y <= (float)(h - 1))) return 2;
  float bu, bv;
  fb_sample(B, pair, base, X, Y, w, h, bu, bv);
  return fb_consistent(u, v, bu, bv, alpha1, alpha2) ? 0u : 1u;
}

// grid (ceil(w h / 1024), n, 2), 256 threads.  counts: n x 2 x 4, zeroed before the launch, or nullptr.  A direction whose mask
// is nullptr and that counts nothing returns at once.
template <class Src>
__global__ __launch_bounds__(256) void fb_check_kernel(Src fw, Src bw, int w, int h, float alpha1, float alpha2,
                                                       unsigned char *__restrict__ mask, unsigned char *__restrict__ mask_bw,
                                                       unsigned *__restrict__ counts)
{
  const int pair = blockIdx.y, dir = blockIdx.z;
  unsigned char *m = dir ? mask_bw : mask;
  if (!m && !counts) return;
  const Src F = dir ? bw : fw, B = dir ? fw : bw;
  const long hw = (long)w * h, base = (long)pair * hw;
  const long r0 = 4 * ((long)blockIdx.x * blockDim.x + threadIdx.x);
  unsigned word = 0, c01 = 0, c23 = 0;           // the four codes as bytes; counts of codes 0 | 1 << 16 and 2 | 3 << 16
  if (r0 < hw) {
    int y = (int)(r0 / w), x = (int)(r0 - (long)y * w);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (r0 + i < hw) {
        const unsigned code = fb_code(F, B, pair, x, y, w, h, base, alpha1, alpha2);
        word |= code << (8 * i);
        const unsigned one = 1u << (16 * (code & 1));
        if (code < 2) c01 += one; else c23 += one;
        if (++x == w) { x = 0; ++y; }
      }
    }
    if (m) {
      unsigned char *o = m + (size_t)base + (size_t)r0;
      if (r0 + 4 <= hw && (((size_t)o) & 3) == 0) {
        __builtin_nontemporal_store(word, reinterpret_cast<unsigned *>(o));
      } else {
        const int nb = (int)(hw - r0 < 4 ? hw - r0 : 4);
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (i < nb) o[i] = (unsigned char)(word >> (8 * i));
      }
    }
  }
  if (!counts) return;
  // (a workgroup counts at most 1024 pixels: every 16-bit field holds its sum)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { c01 += __shfl_xor(c01, o, 64); c23 += __shfl_xor(c23, o, 64); }
  __shared__ unsigned part[256 / FOTG_WAVE][2];
  const int wave = threadIdx.x / FOTG_WAVE, lane = threadIdx.x % FOTG_WAVE;
  if (lane == 0) { part[wave][0] = c01; part[wave][1] = c23; }
  __syncthreads();
  if (threadIdx.x < FB_NCODE) {
    unsigned s = 0;
    for (int i = 0; i < (int)(blockDim.x / FOTG_WAVE); ++i) s += part[i][threadIdx.x >> 1];
    s = (s >> (16 * (threadIdx.x & 1))) & 0xffffu;
    if (s) atomicAdd(counts + ((size_t)pair * 2 + dir) * FB_NCODE + threadIdx.x, s);
  }
}

}  // namespace fotg
