// temporal.hip.h -- motion-compensated temporal filtering: the frames around a centre frame pulled onto it along their flows and
// averaged with weights that fall with the local photometric difference (include/fotg.h fotg_temporal_filter has the definition).
// Per output image a centre frame C, K neighbour frames b_1 .. b_K (-1 = absent), a flow F_k (centre -> neighbour) and optionally
// a mask m_k (fotg_fb_check's alphabet) per neighbour.  All arithmetic f32, every operation rounded on its own, in this order; taps,
// own and code are fotg_warp's (warp.hip.h) in its reference fill mode with fill 0, src = frame b_k, flow F_k, occ m_k:
//
//   W_k[q][ch] = own != 3 ? taps(frame b_k, q + F_k[q])[ch] : 0
//   d_k[q]     = fabsf(C[q][0] - W_k[q][0]) (+ fabsf(C[q][1] - W_k[q][1]) + fabsf(C[q][2] - W_k[q][2]), left to right)
//   r_k[x, y]  = (d_k[cl(x-1), y] + d_k[x, y]) + d_k[cl(x+1), y]           (cl clamps to the image: a 3 x 3 box with replicated
//   e_k[x, y]  = (r_k[x, cl(y-1)] + r_k[x, y]) + r_k[x, cl(y+1)]            edges, summed separably)
//   wt         = g_k * (1.0f - e_k * scale)                                  (scale = 1.0f / (tau * (float)(9 channels)), host f32)
//   use_k      = code_k == 0 && wt > 0                                       (a NaN fails)
//   num[ch] = C[ch]; den = 1; used = 0;  for k ascending with use_k: num[ch] = num[ch] + wt * W_k[ch]; den = den + wt; ++used
//   value[ch] = num[ch] / den                                                (correctly rounded; den >= 1)
//
// temporal_kernel: one pass.  grid (ceil(w / 64), ceil(h / 16), n), 256 threads; a workgroup owns a 64 x 16 tile of one output image,
// thread t the four pixels 4 (t % 16) .. + 3 of tile row t / 16, so a thread's flow vectors, its centre pixels and its outputs are
// 16-byte runs (warp_flow4 / warp_store4 / warp_store_code4) and a wave covers four full tile rows.  The centre pixels, num, den
// and used stay in registers across the loop over the neighbours.  Per neighbour every thread computes W_k and d_k of its pixels
// and writes d_k into a 66 x 18 LDS plane; the 164 pixels of the one-pixel halo are computed (d_k only, from their own flow vector,
// at the position clamped to the image) by the first 164 threads.  After a barrier the 18 x 64 row sums r_k go to a second LDS
// plane, after another barrier each thread adds three of them per pixel.  A plane entry outside the image holds the value of the
// clamped position, which is what cl asks for.  The taps are gathered through L2 as in warp_kernel.  Nothing but dst and used is
// written, once.
// Statistics (per image four doubles: sum of used, pixels with used == 0, sum |ref - value|, sum |ref - C| over all pixels and
// channels) without floating-point atomics: per thread (pixel, then channel order), then warp_block_reduce into one WarpPartial
// per workgroup (c01 = sum of used, c23 = pixels with used == 0), then temporal_fold_kernel, one workgroup per image, adds the
// partials in index order as warp_fold_kernel does.  Dense and fused launches share the geometry, so they produce the same bits.
#pragma once
#include "common.h"
#include "flowsrc.hip.h"
#include "warp.hip.h"

namespace fotg {

enum { TEMPORAL_NSTAT = 4, TEMPORAL_MAXK = 8, TEMPORAL_TW = 64, TEMPORAL_TH = 16,
       TEMPORAL_HALO = 2 * (TEMPORAL_TW + 2) + 2 * TEMPORAL_TH };

struct TemporalGains { float g[TEMPORAL_MAXK]; };

template <class Src> struct FlowIsDense { static constexpr bool value = false; };
template <> struct FlowIsDense<DenseSrc> { static constexpr bool value = true; };

// W_k (fotg_warp's reference-mode value with fill 0) and d_k of pixel (x, y) with centre value c and flow vector (u, v); own as
// in warp_kernel
template <class T, int NOC>
__device__ __forceinline__ float temporal_diff(const T *__restrict__ S, int w, int h, int x, int y, float u, float v,
                                               const float (&c)[NOC], float (&W)[NOC], unsigned &own)
{
  own = 3;
#pragma unroll
  for (int ch = 0; ch < NOC; ++ch) W[ch] = 0.f;
  if (__builtin_isfinite(u) && __builtin_isfinite(v)) {
    const float xx = (float)x + u, yy = (float)y + v;
    own = warp_inside(xx, yy, w, h) ? 0u : 2u;
    warp_taps<T, NOC>(S, w, h, xx, yy, W);
  }
  float d = fabsf(c[0] - W[0]);
#pragma unroll
  for (int ch = 1; ch < NOC; ++ch) d = d + fabsf(c[ch] - W[ch]);
  return d;
}

// flow: the vectors of the n K (image, neighbour) pairs; frames: the stack, T x h x w x NOC; ref / dst: n x h x w x NOC or null;
// masks: n x K x h x w bytes or null; idx: per image K + 1 ints, the centre's frame index and the K neighbours' (-1 = absent),
// validated by the host; used: n x h x w bytes or null; part: (n x gridDim.y x gridDim.x) WarpPartial or null.
template <class Src, class T, int NOC>
__global__ __launch_bounds__(WARP_THREADS) void temporal_kernel(Src flow, const T *__restrict__ frames, const T *__restrict__ ref,
                                                                const unsigned char *__restrict__ masks, const int *__restrict__ idx,
                                                                int K, int w, int h, float scale, TemporalGains gains,
                                                                T *__restrict__ dst, unsigned char *__restrict__ used,
                                                                WarpPartial *__restrict__ part)
{
  __shared__ float sd[TEMPORAL_TH + 2][TEMPORAL_TW + 2];
  __shared__ float sr[TEMPORAL_TH + 2][TEMPORAL_TW];
  const int img = blockIdx.z, t = threadIdx.x;
  const int tx = t % (TEMPORAL_TW / 4), ty = t / (TEMPORAL_TW / 4);
  const int bx = blockIdx.x * TEMPORAL_TW, by = blockIdx.y * TEMPORAL_TH;
  const int x0 = bx + 4 * tx, y = by + ty;
  const long hw = (long)w * h;
  const size_t fstride = (size_t)hw * NOC;
  const int *__restrict__ ix = idx + (size_t)img * (K + 1);
  const T *__restrict__ Cf = frames + (size_t)ix[0] * fstride;
  const bool whole = y < h && x0 + 3 < w;                       // the thread's four pixels are four pixels of the image

  // the thread's pixels (clamped to the image), their centre values and accumulators
  const int cy = y < h ? y : h - 1;
  int cx[4];
  float c[4 * NOC], num[4 * NOC], den[4];
  unsigned usedw = 0;                                           // used of pixel i in byte i
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    cx[i] = x0 + i < w ? x0 + i : w - 1;
    const size_t q = ((size_t)cy * w + cx[i]) * NOC;
#pragma unroll
    for (int ch = 0; ch < NOC; ++ch) num[i * NOC + ch] = c[i * NOC + ch] = warp_elem(Cf, q + ch);
    den[i] = 1.0f;
  }
  // the thread's halo pixel: top row, bottom row, left column, right column of the 66 x 18 plane
  int lx = 0, ly = 0, hx = 0, hy = 0;
  float hc[NOC];
  if (t < TEMPORAL_HALO) {
    if (t < 2 * (TEMPORAL_TW + 2)) { lx = t % (TEMPORAL_TW + 2); ly = t < TEMPORAL_TW + 2 ? 0 : TEMPORAL_TH + 1; }
    else { const int s = t - 2 * (TEMPORAL_TW + 2); lx = s < TEMPORAL_TH ? 0 : TEMPORAL_TW + 1; ly = 1 + s % TEMPORAL_TH; }
    hx = clampi(bx - 1 + lx, w); hy = clampi(by - 1 + ly, h);
    const size_t q = ((size_t)hy * w + hx) * NOC;
#pragma unroll
    for (int ch = 0; ch < NOC; ++ch) hc[ch] = warp_elem(Cf, q + ch);
  }

  for (int k = 0; k < K; ++k) {
    const int b = ix[1 + k];
    const float g = gains.g[k];
    if (b < 0 || g == 0.f) continue;                            // (uniform over the workgroup) absent, or a weight that is never > 0
    const T *__restrict__ S = frames + (size_t)b * fstride;
    const int pair = img * K + k;
    const long pbase = (long)pair * hw;
    float u[4], v[4];
    if constexpr (FlowIsDense<Src>::value) {                    // four dense vectors are two 16-byte loads
      if (whole) {
        warp_flow4(flow, pbase + (long)y * w + x0, 4, pair, x0, y, w, u, v);
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) flow.at(pbase + (long)cy * w + cx[i], pair, cx[i], cy, u[i], v[i]);
      }
    }
    float W[4 * NOC];
    unsigned ok = 0;                                            // bit i: code_k == 0 at pixel i
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float ci[NOC], Wi[NOC];
      unsigned own;
#pragma unroll
      for (int ch = 0; ch < NOC; ++ch) ci[ch] = c[i * NOC + ch];
      if constexpr (!FlowIsDense<Src>::value)                   // an upsampled vector right before its use: fewer live registers
        flow.at(pbase + (long)cy * w + cx[i], pair, cx[i], cy, u[i], v[i]);
      sd[ty + 1][1 + 4 * tx + i] = temporal_diff<T, NOC>(S, w, h, cx[i], cy, u[i], v[i], ci, Wi, own);
#pragma unroll
      for (int ch = 0; ch < NOC; ++ch) W[i * NOC + ch] = Wi[ch];
      ok |= (own == 0 ? 1u : 0u) << i;
    }
    if (masks && ok) {
      const unsigned char *__restrict__ m = masks + (size_t)pbase;
      if (whole && (((size_t)(m + (size_t)y * w + x0)) & 3) == 0) {
        const unsigned mw = *reinterpret_cast<const unsigned *>(m + (size_t)y * w + x0);
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if ((mw >> (8 * i)) & 0xffu) ok &= ~(1u << i);
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (m[(size_t)cy * w + cx[i]]) ok &= ~(1u << i);
      }
    }
    if (t < TEMPORAL_HALO) {
      float hu, hv, Wh[NOC];
      unsigned own;
      flow.at(pbase + (long)hy * w + hx, pair, hx, hy, hu, hv);
      sd[ly][lx] = temporal_diff<T, NOC>(S, w, h, hx, hy, hu, hv, hc, Wh, own);
    }
    __syncthreads();
    for (int j = t; j < (TEMPORAL_TH + 2) * TEMPORAL_TW; j += WARP_THREADS) {
      const int ry = j / TEMPORAL_TW, rx = j % TEMPORAL_TW;
      sr[ry][rx] = (sd[ry][rx] + sd[ry][rx + 1]) + sd[ry][rx + 2];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float e = (sr[ty][4 * tx + i] + sr[ty + 1][4 * tx + i]) + sr[ty + 2][4 * tx + i];
      const float wt = g * (1.0f - e * scale);
      if (((ok >> i) & 1u) && wt > 0.f) {
#pragma unroll
        for (int ch = 0; ch < NOC; ++ch) num[i * NOC + ch] = num[i * NOC + ch] + wt * W[i * NOC + ch];
        den[i] = den[i] + wt;
        usedw += 1u << (8 * i);
      }
    }
  }

  unsigned n_used = 0, n_zero = 0;
  double s_val = 0.0, s_ctr = 0.0;
  if (y < h && x0 < w) {
    const int nb = w - x0 < 4 ? w - x0 : 4;
    const size_t p0 = (size_t)img * hw + (size_t)y * w + x0;
    float val[4 * NOC];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int ch = 0; ch < NOC; ++ch) val[i * NOC + ch] = num[i * NOC + ch] / den[i];
      if (i < nb && part) {
        const unsigned cnt = (usedw >> (8 * i)) & 0xffu;
        n_used += cnt;
        n_zero += cnt == 0 ? 1u : 0u;
        if (ref) {
#pragma unroll
          for (int ch = 0; ch < NOC; ++ch) {
            const float r = warp_elem(ref, (p0 + i) * NOC + ch);
            s_val += (double)fabsf(r - val[i * NOC + ch]);
            s_ctr += (double)fabsf(r - c[i * NOC + ch]);
          }
        }
      }
    }
    if (dst) warp_store4<T, NOC>(dst + p0 * NOC, val, nb);
    if (used) warp_store_code4(used + p0, usedw, nb);
  }
  if (part)
    warp_block_reduce(n_used, n_zero, s_val, s_ctr,
                      part + ((size_t)img * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x);
}

// grid n, 256 threads: the `blocks` partials of image blockIdx.x, added in a fixed order, into stats[4 blockIdx.x ..]
__global__ __launch_bounds__(WARP_THREADS) void temporal_fold_kernel(const WarpPartial *__restrict__ part, int blocks,
                                                                     double *__restrict__ stats)
{
  const WarpPartial *p = part + (size_t)blockIdx.x * blocks;
  double s0 = 0.0, s1 = 0.0;
  unsigned long long c0 = 0, c1 = 0;
  for (int j = threadIdx.x; j < blocks; j += WARP_THREADS) {
    const WarpPartial q = p[j];
    s0 += q.s[0]; s1 += q.s[1];
    c0 += q.c01; c1 += q.c23;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s0 += __shfl_xor(s0, o, 64); s1 += __shfl_xor(s1, o, 64);
    c0 += __shfl_xor(c0, o, 64); c1 += __shfl_xor(c1, o, 64);
  }
  __shared__ double sd[WARP_THREADS / FOTG_WAVE][2];
  __shared__ unsigned long long sc[WARP_THREADS / FOTG_WAVE][2];
  const int wave = threadIdx.x / FOTG_WAVE, lane = threadIdx.x % FOTG_WAVE;
  if (lane == 0) { sd[wave][0] = s0; sd[wave][1] = s1; sc[wave][0] = c0; sc[wave][1] = c1; }
  __syncthreads();
  if (threadIdx.x < TEMPORAL_NSTAT) {
    const int k = threadIdx.x;
    double r;
    if (k < 2) {
      unsigned long long c = 0;
      for (int i = 0; i < WARP_THREADS / FOTG_WAVE; ++i) c += sc[i][k];
      r = (double)c;
    } else {
      r = sd[0][k - 2];
      for (int i = 1; i < WARP_THREADS / FOTG_WAVE; ++i) r += sd[i][k - 2];
    }
    stats[(size_t)blockIdx.x * TEMPORAL_NSTAT + k] = r;
  }
}

}  // namespace fotg
