// interp.hip.h -- the frame at time t between two frames, from their bidirectional flow: the interpolation procedure of the
// Middlebury flow benchmark (Baker et al., "A Database and Evaluation Methodology for Optical Flow", section 3.3): project the
// flow forward to t, resolve collisions by photo-consistency, fill what stays empty from the other direction, sample both frames,
// blend with occlusion reasoning.  All arithmetic f32, every operation rounded on its own (the library's -ffp-contract=off), in
// this order.  I0, I1: w x h frames, interleaved channels; F (0 -> 1), B (1 -> 0): full-resolution flows; mF, mB: their masks in
// fotg_fb_check's alphabet; 0 < t < 1; t1 = 1.0f - t.  "taps(S, xx, yy)" and "inside(xx, yy)" are fotg_warp's value (four clamped
// taps, products summed left to right) and its in-frame test (warp.hip.h: the same functions, not a copy).
//
// 1. Candidates, per direction: forward (Isrc, Idst, V, m, s) = (I0, I1, F, mF, t), backward = (I1, I0, B, mB, t1).
//    Per source pixel p = (x, y), linear index i = y w + x:
//      u, v = V[p];  skip unless isfinite(u) && isfinite(v)
//      c = m[p];     skip unless c <= 1                                (codes 2 and 3, and any byte above, never project)
//      val = taps(Idst, (float)x + u, (float)y + v)
//      e = sum over channels, in order, of fabsf(Isrc[p][ch] - val[ch])            (fotg_warp's residual term)
//      q = e * 256 < 16777215 ? (unsigned)floorf(e * 256) : 16777215               (a NaN cost is the largest)
//      tx = floorf(((float)x + s * u) + 0.5f);  ty alike;  skip unless 0 <= tx <= w-1 && 0 <= ty <= h-1
//      key = c << 56 | q << 32 | i                                                 (w h < 2^32)
//      K[ty][tx] = min(K[ty][tx], key)                                             (one 64-bit integer atomicMin)
//    So a consistent candidate beats an inconsistent one, then the lower cost wins, then the lower source index: a minimum, which
//    does not depend on the order of arrival.  K starts as all ones (empty).
// 2. Resolve, per target pixel (x, y):
//      forward key present:  p* = its low 32 bits, (Vu, Vv) = F[p*],  origin 0
//      else backward key:    p* likewise,          (Vu, Vv) = -B[p*], origin 1
//      else:                                       (Vu, Vv) = 0,      origin 2 (a hole)
//      x0 = (float)x - t * Vu;  y0 alike;  x1 = (float)x + t1 * Vu;  y1 alike
//      v0 = taps(I0, x0, y0);  in0 = inside(x0, y0);  v1 = taps(I1, x1, y1);  in1 = inside(x1, y1)
//      o0 = mF[clamp(floorf(y0 + 0.5f), 0, h-1)][clamp(floorf(x0 + 0.5f), 0, w-1)] != 0;  o1 alike from mB at (x1, y1)
//      use0 = in0;  use1 = in1
//      for origin != 2:  if (o1 && !o0) use0 = false   (frame 1's pixel has no match in frame 0, frame 0's pixel has one elsewhere:
//                                                       the content is visible in frame 1 only)
//                        if (o0 && !o1) use1 = false   (the mirror image; both tests use the o0, o1 read above)
//      value = use0 && use1 ? t1 * v0 + t * v1 : use0 ? v0 : use1 ? v1 : t1 * v0 + t * v1
//    (the weighted mean (w0 v0 + w1 v1) / (w0 + w1) with w0 = use0 ? t1 : 0, w1 = use1 ? t : 0, written without the division: the
//    sum of the weights is t1, t or t1 + t)
//      8-bit dst = fotg_warp's rounding (rintf, clamped to [0, 255])
//      code = origin + 4 (use0 && !use1) + 8 (use1 && !use0)
// 3. Statistics per image (6 f64): pixels of origin 0, 1, 2; one-sided pixels (code >= 4); with a comparison frame R
//    sum (double)fabsf(R - value) and sum (double)fabsf(R - (t1 * I0[y][x] + t * I1[y][x])) (the plain blend) over all pixels and
//    channels, the unrounded f32 value.  Reduced by warp.hip.h's warp_block_reduce / warp_fold_kernel: a fixed order, the same
//    bits every run, and the same from the dense and the fused form.
// tests/interp_ref.py restates all of it in numpy float32.
//
// interp_candidate_kernel: grid (ceil(w h / 1024), images, 2 directions), 256 threads, thread q of an image owns source pixels
// 4q .. 4q+3 (warp_kernel's shape and vector loads); the taps of Idst are gathered through L2; one global atomicMin per candidate
// into the key plane of (image, direction).  Nothing is staged in LDS: an LDS-first variant (resolve a tile's own candidates with
// LDS atomics, send winners and strays to memory) is not built.
// interp_resolve_kernel: grid (ceil(w h / 1024), images), thread q owns target pixels 4q .. 4q+3: two 64-bit key loads per pixel,
// one vector of the winning flow (DenseSrc: a gather; UpsampleSrc: the upsampling evaluated at p*), eight taps, two mask bytes;
// stores as warp_kernel's.
#pragma once
#include "common.h"
#include "flowsrc.hip.h"
#include "warp.hip.h"

namespace fotg {

typedef unsigned long long interp_key;
#define FOTG_INTERP_EMPTY (~0ull)

__device__ __forceinline__ unsigned interp_mask4(const unsigned char *__restrict__ o, int nb)
{
  unsigned word = 0;
  if (nb == 4 && (((size_t)o) & 3) == 0) {
    word = *reinterpret_cast<const unsigned *>(o);
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (i < nb) word |= (unsigned)o[i] << (8 * i);
  }
  return word;
}

// fw / bw: the flows; I0 / I1: n x h x w x NOC of T; mF / mB: n x h x w bytes; keys: n x 2 x (w h), all ones before the launch
template <class Src, class T, int NOC>
__global__ __launch_bounds__(WARP_THREADS) void interp_candidate_kernel(Src fw, Src bw, const T *__restrict__ I0, const T *__restrict__ I1,
                                                                        const unsigned char *__restrict__ mF,
                                                                        const unsigned char *__restrict__ mB, int w, int h, float t,
                                                                        interp_key *__restrict__ keys)
{
  const int pair = blockIdx.y, dir = blockIdx.z;
  const long hw = (long)w * h, base = (long)pair * hw;
  const long r0 = 4 * ((long)blockIdx.x * blockDim.x + threadIdx.x);
  if (r0 >= hw) return;
  const Src V = dir ? bw : fw;
  const T *Isrc = (dir ? I1 : I0) + (size_t)base * NOC, *Idst = (dir ? I0 : I1) + (size_t)base * NOC;
  const float s = dir ? 1.0f - t : t;
  interp_key *K = keys + ((size_t)pair * 2 + dir) * (size_t)hw;
  const int nb = (int)(hw - r0 < 4 ? hw - r0 : 4);
  int y = (int)(r0 / w), x = (int)(r0 - (long)y * w);
  float u[4], v[4];
  warp_flow4(V, base + r0, nb, pair, x, y, w, u, v);
  const unsigned mw = interp_mask4((dir ? mB : mF) + (size_t)base + (size_t)r0, nb);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const unsigned c = (mw >> (8 * i)) & 0xffu;
    if (i < nb && c <= 1 && __builtin_isfinite(u[i]) && __builtin_isfinite(v[i])) {
      const float tx = floorf(((float)x + s * u[i]) + 0.5f), ty = floorf(((float)y + s * v[i]) + 0.5f);
      if (tx >= 0.f && tx <= (float)(w - 1) && ty >= 0.f && ty <= (float)(h - 1)) {
        float val[NOC];
        warp_taps<T, NOC>(Idst, w, h, (float)x + u[i], (float)y + v[i], val);
        const size_t p = (size_t)(r0 + i) * NOC;
        float e = fabsf(warp_elem(Isrc, p) - val[0]);
#pragma unroll
        for (int ch = 1; ch < NOC; ++ch) e += fabsf(warp_elem(Isrc, p + ch) - val[ch]);
        const float e256 = e * 256.f;
        const unsigned q = e256 < 16777215.f ? (unsigned)floorf(e256) : 16777215u;
        const interp_key key = (interp_key)c << 56 | (interp_key)q << 32 | (interp_key)(r0 + i);
        atomicMin(K + ((size_t)(int)ty * w + (size_t)(int)tx), key);
      }
    }
    if (++x == w) { x = 0; ++y; }
  }
}

// ref, dst: like I0 (either may be null); code: n x h x w bytes or null; part: (n x gridDim.x) WarpPartial or null
template <class Src, class T, int NOC>
__global__ __launch_bounds__(WARP_THREADS) void interp_resolve_kernel(Src fw, Src bw, const T *__restrict__ I0, const T *__restrict__ I1,
                                                                      const unsigned char *__restrict__ mF,
                                                                      const unsigned char *__restrict__ mB,
                                                                      const interp_key *__restrict__ keys, const T *__restrict__ ref,
                                                                      int w, int h, float t, T *__restrict__ dst,
                                                                      unsigned char *__restrict__ code, WarpPartial *__restrict__ part)
{
  const int pair = blockIdx.y;
  const long hw = (long)w * h, base = (long)pair * hw;
  const long r0 = 4 * ((long)blockIdx.x * blockDim.x + threadIdx.x);
  unsigned c01 = 0, c23 = 0;
  double s_val = 0.0, s_blend = 0.0;
  if (r0 < hw) {
    const int nb = (int)(hw - r0 < 4 ? hw - r0 : 4);
    int y = (int)(r0 / w), x = (int)(r0 - (long)y * w);
    const float t1 = 1.0f - t;
    const T *S0 = I0 + (size_t)base * NOC, *S1 = I1 + (size_t)base * NOC;
    const unsigned char *M0 = mF + (size_t)base, *M1 = mB + (size_t)base;
    const interp_key *KF = keys + (size_t)pair * 2 * (size_t)hw, *KB = KF + hw;
    float val[4 * NOC];
    unsigned word = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int c = 0; c < NOC; ++c) val[i * NOC + c] = 0.f;
      if (i < nb) {
        const interp_key kf = KF[r0 + i], kb = KB[r0 + i];
        unsigned origin = 2;
        float Vu = 0.f, Vv = 0.f;
        if (kf != FOTG_INTERP_EMPTY) {
          const long p = (long)(kf & 0xffffffffull);
          const int py = (int)(p / w);
          fw.at(base + p, pair, (int)(p - (long)py * w), py, Vu, Vv);
          origin = 0;
        } else if (kb != FOTG_INTERP_EMPTY) {
          const long p = (long)(kb & 0xffffffffull);
          const int py = (int)(p / w);
          bw.at(base + p, pair, (int)(p - (long)py * w), py, Vu, Vv);
          Vu = -Vu; Vv = -Vv;
          origin = 1;
        }
        const float x0 = (float)x - t * Vu, y0 = (float)y - t * Vv;
        const float x1 = (float)x + t1 * Vu, y1 = (float)y + t1 * Vv;
        float v0[NOC], v1[NOC];
        warp_taps<T, NOC>(S0, w, h, x0, y0, v0);
        warp_taps<T, NOC>(S1, w, h, x1, y1, v1);
        bool use0 = warp_inside(x0, y0, w, h), use1 = warp_inside(x1, y1, w, h);
        if (origin != 2) {
          const bool o0 = M0[(size_t)clampi(warp_sat(floorf(y0 + 0.5f), h), h) * w + clampi(warp_sat(floorf(x0 + 0.5f), w), w)] != 0;
          const bool o1 = M1[(size_t)clampi(warp_sat(floorf(y1 + 0.5f), h), h) * w + clampi(warp_sat(floorf(x1 + 0.5f), w), w)] != 0;
          if (o1 && !o0) use0 = false;
          if (o0 && !o1) use1 = false;
        }
        const bool only0 = use0 && !use1, only1 = use1 && !use0;
        float value[NOC];
#pragma unroll
        for (int c = 0; c < NOC; ++c) {
          value[c] = only0 ? v0[c] : (only1 ? v1[c] : t1 * v0[c] + t * v1[c]);
          val[i * NOC + c] = value[c];
        }
        const unsigned cd = origin + (only0 ? 4u : 0u) + (only1 ? 8u : 0u);
        word |= cd << (8 * i);
        if (origin < 2) c01 += 1u << (16 * origin); else c23 += 1u;
        if (cd >= 4) c23 += 1u << 16;
        if (part && ref) {
          const size_t q = (size_t)(base + r0 + i) * NOC;
#pragma unroll
          for (int c = 0; c < NOC; ++c) {
            const float r = warp_elem(ref, q + c);
            s_val += (double)fabsf(r - value[c]);
            s_blend += (double)fabsf(r - (t1 * warp_elem(I0, q + c) + t * warp_elem(I1, q + c)));
          }
        }
      }
      if (++x == w) { x = 0; ++y; }
    }
    if (dst) warp_store4<T, NOC>(dst + (size_t)(base + r0) * NOC, val, nb);
    if (code) warp_store_code4(code + (size_t)base + (size_t)r0, word, nb);
  }
  if (part) warp_block_reduce(c01, c23, s_val, s_blend, part + (size_t)pair * gridDim.x + blockIdx.x);
}

}  // namespace fotg
