// flowfilter.hip.h -- edge- and occlusion-aware filtering of a flow: a joint (cross) bilateral filter of the vectors, guided by the
// frame the flow belongs to, that leaves out the vectors a consistency mask rejects and fills rejected pixels from the consistent
// vectors around them (include/fotg.h fotg_flow_filter has the definition).  Per image of w x h: the flow F (h x w x 2 f32), a guide
// G (h x w x channels, channels 1 or 3, f32 or 8-bit converted exactly to f32), optionally a mask M (h x w bytes, fotg_fb_check's
// alphabet), a radius 1 <= R <= 7, a table s[0 .. R] with every entry in [0, 1] and s[0] > 0, tau > 0 and
// scale = 1.0f / (tau * (float)channels) (host f32).  All arithmetic f32, every operation rounded on its own, in this order:
//
//   valid(q) = q inside the image && isfinite(F(q).u) && isfinite(F(q).v) && (no mask || M(q) == 0)
//   one pass, pixel p:
//     nu = nv = den = 0
//     for dy = -R .. R ascending, inside it dx = -R .. R ascending, q = p + (dx, dy); a q outside the image is skipped:
//       d   = |G(p)[0] - G(q)[0]| (+ |G(p)[1] - G(q)[1]| + |G(p)[2] - G(q)[2]|, left to right)
//       wt  = (s[|dy|] * s[|dx|]) * (1.0f - d * scale)
//       use = valid(q) && wt > 0                                        (a NaN fails)
//       if use: nu = nu + wt * F(q).u;  nv = nv + wt * F(q).v;  den = den + wt
//     den > 0:   out = (nu / den, nv / den);  code = valid(p) ? 0 : 1     (1 = filled from the neighbours)
//     otherwise: out = F(p) bit for bit;      code = 3                    (no support)
//   pass k >= 2 is pass 1 on the previous output with the mask (code_{k-1} == 3) and the same guide; the final code is 3 where the
//   last pass says 3, otherwise 0 where pass 1 said 0, otherwise 1.
//
// flowfilter_kernel: one pass.  grid (ceil(w / 64), ceil(h / 16), n), 256 threads; a workgroup owns a 64 x 16 tile of one image,
// thread t the four pixels 4 (t % 16) .. + 3 of tile row t / 16 (the temporal filter's shape), so its stores are 16-byte runs.
//   1. The tile plus a halo of R, (64 + 2R) x (16 + 2R) entries, goes into LDS once: a plane of u, a plane of v, the guide (one
//      plane per f32 channel; an 8-bit guide, gray or RGB, packed into the bytes of one word) and a plane of bytes, bit 0 = valid,
//      bit 7 = "pass 1 said 0" carried through the passes.  An entry outside the image is marked invalid and nothing of it is read
//      from memory.  This is the only place the vectors are read (the only place UpsampleSrc::at is evaluated for the filter).
//   2. One barrier.
//   3. A thread walks the 2R + 1 window rows; of a row it reads the 4 + 2R entries once, each from LDS into registers, and uses
//      an entry for every one of its four pixels whose window holds it.  The weight of column offset dx comes from a 4 + 2R entry
//      table in LDS, c[j] = s[|j - R|] for j <= 2R and 0 beyond, read once per entry (a broadcast) and passed from pixel to pixel
//      through a four-stage shift register: pixel i uses c[j - i], for 0 <= j - i <= 2R.  nu, nv, den stay in registers.
//   4. out and code are stored with warp_store4 / warp_store_code4.
// The planes have a pitch of 65 + 2R words: odd, so the four tile rows of a wave (lanes 4 words apart within a row) fall on 64
// distinct banks.  The LDS of a launch is sized by its R (flowfilter_lds_bytes): 30.9 KB (gray, 8-bit RGB) to 49.9 KB (f32 RGB)
// at R = 7, 20.4 to 32.9 KB at R = 3, which with the 160 KiB of a CU allows 5 to 3 and 8 to 4 workgroups (waves per SIMD).
// Several passes ping-pong between `out` and stream-ordered memory of the call (fotg_flowfilter.hip); a pass k >= 2 stages the
// previous pass's vectors (prev) and its code bytes, and evaluates the original source again only for the change statistic, at
// the thread's own four pixels.
// Statistics (per image four doubles: pixels of final code 0, 1, 3, and over the pixels of final code 0 the sum of
// (double)fabsf(out.u - F.u) and (double)fabsf(out.v - F.v), F the input of pass 1, terms that are not finite left out) without
// floating-point atomics: per thread (pixel, then u, v), then warp_block_reduce into one WarpPartial per workgroup, then
// flowfilter_fold_kernel, one workgroup per image, adds the partials in index order as warp_fold_kernel does.  Dense and fused
// launches share the geometry, so they produce the same bits.
#pragma once
#include "common.h"
#include "flowsrc.hip.h"
#include "warp.hip.h"

namespace fotg {

enum { FLOWFILTER_NSTAT = 4, FLOWFILTER_MAXR = 7, FLOWFILTER_MAXITERS = 4, FLOWFILTER_TW = 64, FLOWFILTER_TH = 16,
       FLOWFILTER_TAB = 4 + 2 * FLOWFILTER_MAXR };
// what a pass reads as its mask and writes as its code
enum { FLOWFILTER_MASK_USER = 0,      // a mask of fotg_fb_check: any non-zero byte is invalid
       FLOWFILTER_MASK_PASS = 1 };    // the code bytes of the previous pass: (byte & 3) == 3 is invalid, bit 7 is carried
enum { FLOWFILTER_CODE_FINAL = 0,     // the final code: 3, or 0 where pass 1 said 0 (this pass, if it is the first), or 1
       FLOWFILTER_CODE_PASS = 1 };    // this pass's own code in bits 0..1, "pass 1 said 0" in bit 7

struct FlowFilterSpatial { float s[FLOWFILTER_MAXR + 1]; };

__host__ __device__ inline int flowfilter_pitch(int R) { return FLOWFILTER_TW + 2 * R + 1; }
// words of guide per LDS entry: one per f32 channel, one for an 8-bit pixel
template <class T, int NOC> struct FlowFilterGuide { static constexpr int words = sizeof(T) == 1 ? 1 : NOC; };
template <class T, int NOC> inline size_t flowfilter_lds_bytes(int R)
{
  const size_t plane = (size_t)flowfilter_pitch(R) * (FLOWFILTER_TH + 2 * R);
  return FLOWFILTER_TAB * sizeof(float) + plane * (2 + FlowFilterGuide<T, NOC>::words) * sizeof(float) + ((plane + 3) & ~(size_t)3);
}

// the guide pixel at element index q NOC of G as LDS words
template <int NOC> __device__ __forceinline__ void flowfilter_guide_load(const float *__restrict__ G, size_t q, float (&g)[NOC])
{
#pragma unroll
  for (int ch = 0; ch < NOC; ++ch) g[ch] = G[q * NOC + ch];
}
template <int NOC> __device__ __forceinline__ void flowfilter_guide_load(const unsigned char *__restrict__ G, size_t q, float (&g)[1])
{
  unsigned wd = G[q * NOC];
  if constexpr (NOC == 3) wd |= (unsigned)G[q * NOC + 1] << 8 | (unsigned)G[q * NOC + 2] << 16;
  g[0] = __uint_as_float(wd);
}
// LDS words -> the NOC channels as f32
template <class T, int NOC> __device__ __forceinline__ void flowfilter_guide_decode(const float (&g)[FlowFilterGuide<T, NOC>::words], float (&c)[NOC])
{
  if constexpr (sizeof(T) == 1) {
    const unsigned wd = __float_as_uint(g[0]);
#pragma unroll
    for (int ch = 0; ch < NOC; ++ch) c[ch] = (float)((wd >> (8 * ch)) & 0xffu);
  } else {
#pragma unroll
    for (int ch = 0; ch < NOC; ++ch) c[ch] = g[ch];
  }
}

// flow: the input of pass 1 (dense or the coarse flow of a context); prev: null in pass 1, otherwise the previous pass's vectors
// (n x h x w x 2); guide: n x h x w x NOC of T; mask: n x h x w bytes or null, read as mask_mode says; out: n x h x w x 2 or null;
// code: n x h x w bytes or null, written as code_mode says; part: (n x gridDim.y x gridDim.x) WarpPartial or null (the last pass).
// Dynamic LDS: flowfilter_lds_bytes<T, NOC>(R).
template <class Src, class T, int NOC>
__global__ __launch_bounds__(WARP_THREADS) void flowfilter_kernel(Src flow, const float *__restrict__ prev, const T *__restrict__ guide,
                                                                  const unsigned char *__restrict__ mask, int mask_mode, int w, int h,
                                                                  int R, float scale, FlowFilterSpatial sp, float *__restrict__ out,
                                                                  unsigned char *__restrict__ code, int code_mode,
                                                                  WarpPartial *__restrict__ part)
{
  constexpr int GW = FlowFilterGuide<T, NOC>::words;
  extern __shared__ float ff_lds[];
  const int P = flowfilter_pitch(R), HW = FLOWFILTER_TW + 2 * R, HH = FLOWFILTER_TH + 2 * R;
  const int plane = P * HH;
  float *__restrict__ ctab = ff_lds;                               // FLOWFILTER_TAB column weights
  float *__restrict__ su = ff_lds + FLOWFILTER_TAB;
  float *__restrict__ sv = su + plane;
  float *__restrict__ sg = sv + plane;                             // GW planes
  unsigned char *__restrict__ sk = reinterpret_cast<unsigned char *>(sg + (size_t)GW * plane);

  const int img = blockIdx.z, t = threadIdx.x;
  const int tx = t % (FLOWFILTER_TW / 4), ty = t / (FLOWFILTER_TW / 4);
  const int bx = blockIdx.x * FLOWFILTER_TW, by = blockIdx.y * FLOWFILTER_TH;
  const int x0 = bx + 4 * tx, y = by + ty;
  const long hw = (long)w * h, ibase = (long)img * hw;

  // 1. the tile and its halo
  if (t < FLOWFILTER_TAB) {
    const int a = t < R ? R - t : t - R;
    float c = sp.s[0];
#pragma unroll
    for (int k = 1; k <= FLOWFILTER_MAXR; ++k) c = a == k ? sp.s[k] : c;
    ctab[t] = t <= 2 * R ? c : 0.f;
  }
  for (int e = t; e < HW * HH; e += WARP_THREADS) {
    const int ly = e / HW, lx = e - ly * HW;
    const int gx = bx - R + lx, gy = by - R + ly;
    float u = 0.f, v = 0.f, g[GW];
#pragma unroll
    for (int k = 0; k < GW; ++k) g[k] = 0.f;
    unsigned kb = 0;
    if (gx >= 0 && gx < w && gy >= 0 && gy < h) {
      const long p = ibase + (long)gy * w + gx;
      if (prev) { u = prev[2 * p]; v = prev[2 * p + 1]; }
      else flow.at(p, img, gx, gy, u, v);
      flowfilter_guide_load<NOC>(guide, (size_t)p, g);
      bool ok = __builtin_isfinite(u) && __builtin_isfinite(v);
      if (mask) {
        const unsigned m = mask[p];
        if (mask_mode == FLOWFILTER_MASK_PASS) { ok = ok && (m & 3u) != 3u; kb = m & 0x80u; }
        else ok = ok && m == 0;
      }
      kb |= ok ? 1u : 0u;
    }
    const int o = ly * P + lx;
    su[o] = u; sv[o] = v;
#pragma unroll
    for (int k = 0; k < GW; ++k) sg[k * plane + o] = g[k];
    sk[o] = (unsigned char)kb;
  }
  __syncthreads();

  // 2. the window: rows dy ascending, of a row the entries j = 0 .. 3 + 2R ascending, entry j being dx = j - i - R of pixel i
  const int ctr = (ty + R) * P + 4 * tx + R;                        // the thread's first pixel
  float gp[4][NOC], nu[4], nv[4], den[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float gw[GW];
#pragma unroll
    for (int k = 0; k < GW; ++k) gw[k] = sg[k * plane + ctr + i];
    flowfilter_guide_decode<T, NOC>(gw, gp[i]);
    nu[i] = nv[i] = den[i] = 0.f;
  }
  for (int dy = -R; dy <= R; ++dy) {
    const float sy = ctab[dy + R];                                  // s[|dy|]
    const int row = ctr + dy * P - R;
    float c1 = 0.f, c2 = 0.f, c3 = 0.f;                             // sy * s[|dx|] of the pixels 1, 2, 3 at this entry
    for (int j = 0; j < 4 + 2 * R; ++j) {
      const float c0 = sy * ctab[j];
      float gw[GW], gq[NOC];
#pragma unroll
      for (int k = 0; k < GW; ++k) gw[k] = sg[k * plane + row + j];
      flowfilter_guide_decode<T, NOC>(gw, gq);
      const unsigned kq = sk[row + j] & 1u, keep = 0u - kq;         // an invalid vector may be anything: it becomes +0 (all five
      const bool okq = kq != 0;                                     // LDS reads of an entry are issued together, none depends on
      const float uq = __uint_as_float(__float_as_uint(su[row + j]) & keep);       // the validity byte)
      const float vq = __uint_as_float(__float_as_uint(sv[row + j]) & keep);
      const float cw[4] = {c0, c1, c2, c3};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if ((unsigned)(j - i) <= (unsigned)(2 * R)) {               // (uniform) entry j lies in pixel i's window: dx = j - i - R
          float d = fabsf(gp[i][0] - gq[0]);
#pragma unroll
          for (int ch = 1; ch < NOC; ++ch) d = d + fabsf(gp[i][ch] - gq[ch]);
          float wt = cw[i] * (1.0f - d * scale);
          wt = okq && wt > 0.f ? wt : 0.f;                          // unused: + 0 * (a finite vector) changes no bit of the sums
          nu[i] = nu[i] + wt * uq;
          nv[i] = nv[i] + wt * vq;
          den[i] = den[i] + wt;
        }
      }
      c3 = c2; c2 = c1; c1 = c0;
    }
  }

  // 3. the results
  unsigned c01 = 0, c23 = 0;
  double s_chg = 0.0;
  if (y < h && x0 < w) {
    const int nb = w - x0 < 4 ? w - x0 : 4;
    const size_t p0 = (size_t)ibase + (size_t)y * w + x0;
    float val[8];
    unsigned word = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const unsigned kb = sk[ctr + i];
      const float fu = su[ctr + i], fv = sv[ctr + i];
      unsigned own, fin;                                            // this pass's code, the final code
      if (den[i] > 0.f) {
        val[2 * i] = nu[i] / den[i]; val[2 * i + 1] = nv[i] / den[i];
        own = (kb & 1u) ? 0u : 1u;
      } else {
        val[2 * i] = fu; val[2 * i + 1] = fv;
        own = 3u;
      }
      const bool first0 = mask_mode == FLOWFILTER_MASK_PASS ? (kb & 0x80u) != 0 : own == 0;
      fin = own == 3u ? 3u : (first0 ? 0u : 1u);
      word |= (code_mode == FLOWFILTER_CODE_PASS ? own | (first0 ? 0x80u : 0u) : fin) << (8 * i);
      if (part && i < nb) {
        if (fin == 0) {
          c01 += 1u;
          float ou = fu, ov = fv;                                   // the input of pass 1
          if (prev) flow.at((long)p0 + i, img, x0 + i, y, ou, ov);
          const float du = fabsf(val[2 * i] - ou), dv = fabsf(val[2 * i + 1] - ov);
          if (__builtin_isfinite(du)) s_chg += (double)du;
          if (__builtin_isfinite(dv)) s_chg += (double)dv;
        } else if (fin == 1) {
          c01 += 1u << 16;
        } else {
          c23 += 1u << 16;
        }
      }
    }
    if (out) warp_store4<float, 2>(out + 2 * p0, val, nb);
    if (code) warp_store_code4(code + p0, word, nb);
  }
  if (part)
    warp_block_reduce(c01, c23, s_chg, 0.0, part + ((size_t)img * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x);
}

// grid n, 256 threads: the `blocks` partials of image blockIdx.x, added in a fixed order, into stats[4 blockIdx.x ..]
__global__ __launch_bounds__(WARP_THREADS) void flowfilter_fold_kernel(const WarpPartial *__restrict__ part, int blocks,
                                                                       double *__restrict__ stats)
{
  const WarpPartial *p = part + (size_t)blockIdx.x * blocks;
  double s0 = 0.0;
  unsigned long long c0 = 0, c1 = 0, c3 = 0;
  for (int j = threadIdx.x; j < blocks; j += WARP_THREADS) {
    const WarpPartial q = p[j];
    s0 += q.s[0];
    c0 += q.c01 & 0xffffu; c1 += q.c01 >> 16; c3 += q.c23 >> 16;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s0 += __shfl_xor(s0, o, 64);
    c0 += __shfl_xor(c0, o, 64); c1 += __shfl_xor(c1, o, 64); c3 += __shfl_xor(c3, o, 64);
  }
  __shared__ double sd[WARP_THREADS / FOTG_WAVE];
  __shared__ unsigned long long sc[WARP_THREADS / FOTG_WAVE][3];
  const int wave = threadIdx.x / FOTG_WAVE, lane = threadIdx.x % FOTG_WAVE;
  if (lane == 0) { sd[wave] = s0; sc[wave][0] = c0; sc[wave][1] = c1; sc[wave][2] = c3; }
  __syncthreads();
  if (threadIdx.x < FLOWFILTER_NSTAT) {
    const int k = threadIdx.x;
    double r;
    if (k < 3) {
      unsigned long long c = 0;
      for (int i = 0; i < WARP_THREADS / FOTG_WAVE; ++i) c += sc[i][k];
      r = (double)c;
    } else {
      r = sd[0];
      for (int i = 1; i < WARP_THREADS / FOTG_WAVE; ++i) r += sd[i];
    }
    stats[(size_t)blockIdx.x * FLOWFILTER_NSTAT + k] = r;
  }
}

}  // namespace fotg
