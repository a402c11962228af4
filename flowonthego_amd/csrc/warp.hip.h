// warp.hip.h -- backward warp of an image along a flow (the reference's image_warp, kroeger/FDF1.0.1/opticalflow_aux.c:18-60),
// with validity codes and photometric residuals.  Per pixel (x, y) of a w x h image, channel c, all arithmetic f32, every
// operation rounded on its own (the library's -ffp-contract=off), in this order:
//
//   u, v = F[y][x]
//   if !isfinite(u) || !isfinite(v):            own = 3; value = fill            (the reference converts NaN to int: undefined)
//   xx = (float)x + u;  yy = (float)y + v
//   fx = floorf(xx);    fy = floorf(yy)         (== (float)(int)floor(xx) wherever the reference's conversion is defined)
//   dx = xx - fx;       dy = yy - fy
//   own = (xx >= 0 && xx <= w-1 && yy >= 0 && yy <= h-1) ? 0 : 2                 (image_warp's mask == (own == 0))
//   xi = fx saturated to [-2, w] as int, yi alike to [-2, h]                     (as prep_values does: x + 1 cannot overflow)
//   x1 = clamp(xi, 0, w-1); x2 = clamp(xi+1, 0, w-1); y1, y2 alike
//   value_c = S[y1][x1][c]*(1-dx)*(1-dy) + S[y1][x2][c]*dx*(1-dy) + S[y2][x1][c]*(1-dx)*dy + S[y2][x2][c]*dx*dy
//                                                                                (four products summed left to right)
//   code = own != 0 ? own : (occ ? occ[y][x] (0, 1 or 3; 2 cannot differ from own) : 0)
//   fill_mode 0 (reference): dst = value wherever own != 3
//   fill_mode 1:             dst = code == 0 ? value : fill
//
// S is the image to warp (frame 1 for a forward flow), interleaved n x h x w x channels, channels 1 or 3, f32 or 8-bit.  8-bit
// taps are converted exactly to f32; an 8-bit destination is rintf(value) clamped to [0, 255] (and fill likewise, a NaN becoming
// 0); the residuals always use the unrounded f32 value.  With fill_mode 0, no occ and a finite flow, dst and code == 0 are the
// reference's dst and mask, bit for bit, for any finite flow however large.  (An occ byte above 3 counts as 3.)
// tests/warp_ref.py restates this in numpy float32.
//
// Optional outputs: code (n x h x w uint8, fotg_fb_check's alphabet) and stats (n x 6 f64 per image: pixels of code 0, 1, 2, 3,
// then, with a comparison image R of S's layout and type, over the code-0 pixels and all channels [4] sum (double)|R - value| and
// [5] sum (double)|R - S[y][x]|, every term the f32 fabsf of the f32 difference).
//
// warp_kernel: grid (ceil(w h / 1024), n), 256 threads, the launch shape of fb_check_kernel: thread q of an image owns its pixels
// 4q .. 4q+3 (64-bit batch offsets).  The dense source reads the thread's four vectors as two 16-byte nontemporal loads where the
// address allows; the fused source (UpsampleSrc) evaluates the upsampling once per pixel.  The taps of S are gathered through L2
// (neighbouring pixels have neighbouring targets for a smooth flow); nothing is staged in LDS.  Stores are 16-byte / dword
// nontemporal stores where the thread's span is whole and aligned, elements otherwise.
// Statistics without floating-point atomics, so the same bits every run: the two residual sums (f64) and the four counts are
// reduced per thread (pixel, then channel order), per wave (xor shuffles 32 .. 1) and per workgroup (waves in index order through
// LDS) into one WarpPartial per workgroup; warp_fold_kernel (one workgroup per image) lets thread t add the partials t, t + 256,
// ... in index order, reduces the 256 sums the same way and writes the six doubles.  Dense and fused launches have the same
// geometry, so they produce the same bits.
#pragma once
#include "common.h"
#include "flowsrc.hip.h"

namespace fotg {

enum { WARP_NSTAT = 6, WARP_THREADS = 256 };

struct WarpPartial {
  double s[2];             // sum |R - value|, sum |R - S| over the workgroup's code-0 pixels
  unsigned c01, c23;       // pixels of code 0 | 1 << 16, of code 2 | 3 << 16 (a workgroup covers at most 1024)
};

__device__ __forceinline__ float warp_elem(const float *s, size_t i) { return s[i]; }
__device__ __forceinline__ float warp_elem(const unsigned char *s, size_t i) { return (float)s[i]; }

// the 8-bit destination: rintf, clamped to [0, 255]; a NaN becomes 0
__device__ __forceinline__ unsigned warp_to_u8(float v)
{
  v = rintf(v);
  return !(v > 0.f) ? 0u : (v > 255.f ? 255u : (unsigned)(int)v);
}

// the flow vectors of the pixels p0 .. p0 + nb - 1 (same image; (x, y) = the first of them)
__device__ __forceinline__ void warp_flow4(const DenseSrc &F, long p0, int nb, int, int, int, int, float (&u)[4], float (&v)[4])
{
  typedef float vf4 __attribute__((ext_vector_type(4)));
  const float *f = F.flow + 2 * p0;
  if (nb == 4 && (((size_t)f) & 15) == 0) {
    const vf4 a = __builtin_nontemporal_load(reinterpret_cast<const vf4 *>(f));
    const vf4 b = __builtin_nontemporal_load(reinterpret_cast<const vf4 *>(f) + 1);
    u[0] = a.x; v[0] = a.y; u[1] = a.z; v[1] = a.w; u[2] = b.x; v[2] = b.y; u[3] = b.z; v[3] = b.w;
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      u[i] = v[i] = 0.f;
      if (i < nb) { u[i] = f[2 * i]; v[i] = f[2 * i + 1]; }
    }
  }
}

__device__ __forceinline__ void warp_flow4(const UpsampleSrc &F, long p0, int nb, int pair, int x, int y, int w, float (&u)[4], float (&v)[4])
{
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    u[i] = v[i] = 0.f;
    if (i < nb) F.at(p0 + i, pair, x, y, u[i], v[i]);
    if (++x == w) { x = 0; ++y; }
  }
}

__device__ __forceinline__ int warp_sat(float f, int n)      // f saturated to [-2, n] as int
{
  return f < -2.f ? -2 : (f > (float)n ? n : (int)f);
}

// image_warp's mask: the sample position lies inside the frame
__device__ __forceinline__ bool warp_inside(float xx, float yy, int w, int h)
{
  return xx >= 0.f && xx <= (float)(w - 1) && yy >= 0.f && yy <= (float)(h - 1);
}

// the value of image S (w x h x NOC) at (xx, yy): the four clamped taps of the head of this file, in its order.  Shared with
// interp.hip.h, whose costs and samples are this arithmetic.
template <class T, int NOC>
__device__ __forceinline__ void warp_taps(const T *__restrict__ S, int w, int h, float xx, float yy, float (&value)[NOC])
{
  const float fx = floorf(xx), fy = floorf(yy);
  const float dx = xx - fx, dy = yy - fy;
  const int xi = warp_sat(fx, w), yi = warp_sat(fy, h);
  const int x1 = clampi(xi, w), x2 = clampi(xi + 1, w), y1 = clampi(yi, h), y2 = clampi(yi + 1, h);
  const size_t a11 = ((size_t)y1 * w + x1) * NOC, a12 = ((size_t)y1 * w + x2) * NOC;
  const size_t a21 = ((size_t)y2 * w + x1) * NOC, a22 = ((size_t)y2 * w + x2) * NOC;
#pragma unroll
  for (int c = 0; c < NOC; ++c)
    value[c] = warp_elem(S, a11 + c) * (1.0f - dx) * (1.0f - dy) + warp_elem(S, a12 + c) * dx * (1.0f - dy) +
               warp_elem(S, a21 + c) * (1.0f - dx) * dy + warp_elem(S, a22 + c) * dx * dy;
}

// the thread's nb (<= 4) pixels val[4 NOC] to o: 16-byte / dword nontemporal stores where the span is whole and aligned
template <class T, int NOC>
__device__ __forceinline__ void warp_store4(T *__restrict__ o, const float (&val)[4 * NOC], int nb)
{
  typedef float vf4 __attribute__((ext_vector_type(4)));
  if constexpr (sizeof(T) == 4) {
    if (nb == 4 && (((size_t)o) & 15) == 0) {
#pragma unroll
      for (int k = 0; k < NOC; ++k)
        __builtin_nontemporal_store(vf4{val[4 * k], val[4 * k + 1], val[4 * k + 2], val[4 * k + 3]}, reinterpret_cast<vf4 *>(o) + k);
    } else {
#pragma unroll
      for (int k = 0; k < 4 * NOC; ++k)
        if (k < nb * NOC) o[k] = val[k];
    }
  } else {
    unsigned b[4 * NOC];
#pragma unroll
    for (int k = 0; k < 4 * NOC; ++k) b[k] = warp_to_u8(val[k]);
    if (nb == 4 && (((size_t)o) & 3) == 0) {
#pragma unroll
      for (int k = 0; k < NOC; ++k)
        __builtin_nontemporal_store(b[4 * k] | b[4 * k + 1] << 8 | b[4 * k + 2] << 16 | b[4 * k + 3] << 24, reinterpret_cast<unsigned *>(o) + k);
    } else {
#pragma unroll
      for (int k = 0; k < 4 * NOC; ++k)
        if (k < nb * NOC) o[k] = (unsigned char)b[k];
    }
  }
}

// the thread's nb (<= 4) code bytes, packed in word, to o
__device__ __forceinline__ void warp_store_code4(unsigned char *__restrict__ o, unsigned word, int nb)
{
  if (nb == 4 && (((size_t)o) & 3) == 0) {
    __builtin_nontemporal_store(word, reinterpret_cast<unsigned *>(o));
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (i < nb) o[i] = (unsigned char)(word >> (8 * i));
  }
}

// the workgroup's statistics in the fixed order of the head of this file (wave: xor shuffles 32 .. 1; workgroup: waves in index
// order through LDS) into *out.  Every thread of the workgroup calls it.
__device__ __forceinline__ void warp_block_reduce(unsigned c01, unsigned c23, double s0, double s1, WarpPartial *__restrict__ out)
{
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    c01 += __shfl_xor(c01, o, 64); c23 += __shfl_xor(c23, o, 64);
    s0 += __shfl_xor(s0, o, 64); s1 += __shfl_xor(s1, o, 64);
  }
  __shared__ WarpPartial wp[WARP_THREADS / FOTG_WAVE];
  const int wave = threadIdx.x / FOTG_WAVE, lane = threadIdx.x % FOTG_WAVE;
  if (lane == 0) { wp[wave].s[0] = s0; wp[wave].s[1] = s1; wp[wave].c01 = c01; wp[wave].c23 = c23; }
  __syncthreads();
  if (threadIdx.x == 0) {
    WarpPartial t = wp[0];
    for (int i = 1; i < WARP_THREADS / FOTG_WAVE; ++i) {
      t.s[0] += wp[i].s[0]; t.s[1] += wp[i].s[1]; t.c01 += wp[i].c01; t.c23 += wp[i].c23;
    }
    *out = t;
  }
}

// flow: the vectors; src / ref / dst: n x h x w x NOC of T (ref, dst may be null); occ / code: n x h x w bytes or null;
// part: (n x gridDim.x) WarpPartial or null.
template <class Src, class T, int NOC>
__global__ __launch_bounds__(WARP_THREADS) void warp_kernel(Src flow, const T *__restrict__ src, const T *__restrict__ ref,
                                                            const unsigned char *__restrict__ occ, int w, int h, int fill_mode,
                                                            float fill, T *__restrict__ dst, unsigned char *__restrict__ code,
                                                            WarpPartial *__restrict__ part)
{
  const int pair = blockIdx.y;
  const long hw = (long)w * h, base = (long)pair * hw;
  const long r0 = 4 * ((long)blockIdx.x * blockDim.x + threadIdx.x);
  unsigned c01 = 0, c23 = 0;
  double s_warp = 0.0, s_unw = 0.0;
  if (r0 < hw) {
    const int nb = (int)(hw - r0 < 4 ? hw - r0 : 4);
    int y = (int)(r0 / w), x = (int)(r0 - (long)y * w);
    float u[4], v[4];
    warp_flow4(flow, base + r0, nb, pair, x, y, w, u, v);
    unsigned occw = 0;
    if (occ) {
      const unsigned char *o = occ + (size_t)base + (size_t)r0;
      if (nb == 4 && (((size_t)o) & 3) == 0) {
        occw = *reinterpret_cast<const unsigned *>(o);
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (i < nb) occw |= (unsigned)o[i] << (8 * i);
      }
    }
    const bool want_value = dst || (part && ref);
    const T *S = src + (size_t)base * NOC;
    float val[4 * NOC];
    unsigned word = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int c = 0; c < NOC; ++c) val[i * NOC + c] = fill;
      if (i < nb) {
        unsigned own = 3;
        float value[NOC];
#pragma unroll
        for (int c = 0; c < NOC; ++c) value[c] = fill;
        if (__builtin_isfinite(u[i]) && __builtin_isfinite(v[i])) {
          const float xx = (float)x + u[i], yy = (float)y + v[i];
          own = warp_inside(xx, yy, w, h) ? 0u : 2u;
          if (want_value) warp_taps<T, NOC>(S, w, h, xx, yy, value);
        }
        unsigned cd = own;
        if (own == 0 && occ) {
          cd = (occw >> (8 * i)) & 0xffu;
          cd = cd > 3 ? 3u : cd;
        }
        word |= cd << (8 * i);
        const unsigned one = 1u << (16 * (cd & 1));
        if (cd < 2) c01 += one; else c23 += one;
        const bool keep = fill_mode == 0 ? own != 3 : cd == 0;
        if (keep) {
#pragma unroll
          for (int c = 0; c < NOC; ++c) val[i * NOC + c] = value[c];
        }
        if (part && ref && cd == 0) {
          const size_t q = (size_t)(base + r0 + i) * NOC;
#pragma unroll
          for (int c = 0; c < NOC; ++c) {
            const float r = warp_elem(ref, q + c);
            s_warp += (double)fabsf(r - value[c]);
            s_unw += (double)fabsf(r - warp_elem(src, q + c));
          }
        }
      }
      if (++x == w) { x = 0; ++y; }
    }
    if (dst) warp_store4<T, NOC>(dst + (size_t)(base + r0) * NOC, val, nb);
    if (code) warp_store_code4(code + (size_t)base + (size_t)r0, word, nb);
  }
  if (part) warp_block_reduce(c01, c23, s_warp, s_unw, part + (size_t)pair * gridDim.x + blockIdx.x);
}

// launches warp_fold_kernel for n images on `stream` (defined in fotg_warp.hip, the one translation unit that compiles the kernel;
// fotg_interp.hip folds its partials through it too)
hipError_t warp_fold(const WarpPartial *part, int blocks, int n, double *stats, hipStream_t stream);

#ifdef FOTG_WARP_FOLD_KERNEL
// grid n, 256 threads: the `blocks` partials of image blockIdx.x, added in a fixed order, into stats[6 blockIdx.x ..]
__global__ __launch_bounds__(WARP_THREADS) void warp_fold_kernel(const WarpPartial *__restrict__ part, int blocks, double *__restrict__ stats)
{
  const WarpPartial *p = part + (size_t)blockIdx.x * blocks;
  double s0 = 0.0, s1 = 0.0;
  unsigned long long c0 = 0, c1 = 0, c2 = 0, c3 = 0;
  for (int j = threadIdx.x; j < blocks; j += WARP_THREADS) {
    const WarpPartial t = p[j];
    s0 += t.s[0]; s1 += t.s[1];
    c0 += t.c01 & 0xffffu; c1 += t.c01 >> 16; c2 += t.c23 & 0xffffu; c3 += t.c23 >> 16;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s0 += __shfl_xor(s0, o, 64); s1 += __shfl_xor(s1, o, 64);
    c0 += __shfl_xor(c0, o, 64); c1 += __shfl_xor(c1, o, 64); c2 += __shfl_xor(c2, o, 64); c3 += __shfl_xor(c3, o, 64);
  }
  __shared__ double sd[WARP_THREADS / FOTG_WAVE][2];
  __shared__ unsigned long long sc[WARP_THREADS / FOTG_WAVE][4];
  const int wave = threadIdx.x / FOTG_WAVE, lane = threadIdx.x % FOTG_WAVE;
  if (lane == 0) { sd[wave][0] = s0; sd[wave][1] = s1; sc[wave][0] = c0; sc[wave][1] = c1; sc[wave][2] = c2; sc[wave][3] = c3; }
  __syncthreads();
  if (threadIdx.x < WARP_NSTAT) {
    const int k = threadIdx.x;
    double r;
    if (k < 4) {
      unsigned long long c = 0;
      for (int i = 0; i < WARP_THREADS / FOTG_WAVE; ++i) c += sc[i][k];
      r = (double)c;
    } else {
      r = sd[0][k - 4];
      for (int i = 1; i < WARP_THREADS / FOTG_WAVE; ++i) r += sd[i][k - 4];
    }
    stats[(size_t)blockIdx.x * WARP_NSTAT + k] = r;
  }
}
#endif  // FOTG_WARP_FOLD_KERNEL

}  // namespace fotg
