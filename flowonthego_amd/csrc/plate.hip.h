// plate.hip.h -- background plates and mosaics: the frames of a shot pulled into one coordinate system along their motion and
// reduced per pixel by a median (or a mean) over the frames that see the pixel (include/fotg.h fotg_plate has the definition).
// Per plate i K samples (frame index b_k, -1 = absent) on a W x H canvas whose pixel (X, Y) is the reference coordinate
// (x, y) = (X - ox, Y - oy).  All arithmetic f32, every operation rounded on its own, in this order; taps, warp_inside and the
// 8-bit rounding are fotg_warp's (warp.hip.h), the frame is w x h:
//
//   (u, v)_k  = the sample's vector at the canvas pixel: flows[i][k][Y][X] (dense), the fused source's value at (X, Y), or
//               motion_predict(motion_coef(P_ik, w, h), 2x - (w-1), 2y - (h-1)) (motion source; fotg_motion_flow's arithmetic at a
//               reference coordinate that may lie outside the frame)
//   for k ascending, b_k >= 0; a sample is admitted by these tests, in this order:
//     1. u and v are finite
//     2. xx = (float)x + u, yy = (float)y + v satisfy warp_inside(xx, yy, w, h)          (otherwise own = 2);  ++coverage
//     3. occ == NULL || occ[i][k][Y][X] == 0
//     4. exclude == NULL || exclude[b_k] is zero at (x1, y1), (x2, y1), (x1, y2), (x2, y2), the four clamped tap pixels of fotg_warp
//     5. no channel of s = taps(frame b_k, xx, yy) is NaN;                                 s_m = s; ++m
//   mode 0 (median), per channel: the admitted values ordered by f32 <, ties keeping the k order;
//             m odd: est = s[(m-1)/2];  m even: est = (s[m/2 - 1] + s[m/2]) * 0.5f
//   mode 1 (mean), per channel:   sum = s_0; sum = sum + s_j (j = 1 .. m-1, the k order); est = sum / (float)m  (correctly rounded)
//   code = m >= min_count ? 0 : (coverage < min_count ? 2 : 1);   dst = code == 0 ? est : fill;   count = m
//
// plate_kernel: one launch.  grid (ceil(W / 64), ceil(H / rows), n), 64 rows threads (rows = 1, 2 or 4, fotg_plate_rows): a wave
// owns 64 consecutive pixels of one canvas row, a lane one pixel.  The admitted samples of a lane live in its own column of the
// dynamic LDS, value j of channel ch at float (j NOC + ch) blockDim.x + threadIdx.x: consecutive lanes hit consecutive banks, so
// every access is conflict-free, and since no lane reads another's column the kernel has no barrier.  LDS of a launch:
// 4 K NOC blockDim.x bytes (plate_lds_bytes), 96 KB at K = 32, three channels and 256 threads.  The median is selected by rank
// counting: value j has rank #{i: s_i < s_j || (s_i == s_j && i < j)}, m reads per value; the ranks (m-1)/2 and m/2 are picked
// out on the way, so nothing is ever moved.  A sample that is absent is skipped by the whole workgroup (its index is uniform).
// The taps are gathered through L2 as in warp_kernel; dst, count and code are written once.
// Statistics (per plate six doubles: pixels of code 0, 1, 2, sum of count, and with a comparison image ref over the code-0 pixels
// and all channels sum |ref - est| and sum |ref - s_0|, each term the f32 fabsf of the f32 difference of the unrounded values)
// without floating-point atomics: per lane (channel order), per wave (xor shuffles 32 .. 1) into one WarpPartial per wave -- the
// partial of canvas row Y and column tile bx at index Y gridDim.x + bx, whatever rows is -- then warp_fold_kernel (warp.hip.h) adds
// them in index order.  So every run, every source and every launch shape gives the same bits.
#pragma once
#include "common.h"
#include "flowsrc.hip.h"
#include "motion_model.hip.h"
#include "warp.hip.h"

namespace fotg {

enum { PLATE_MAXK = 32, PLATE_MAX_DIM = 16384, PLATE_MAX_ORIGIN = 1 << 20, PLATE_TW = 64, PLATE_MAX_ROWS = 4 };

// A camera motion per sample: params n K x 6 f64 in fit_motion's pixel-frame convention for the w x h frame; (x, y) is the
// reference coordinate of the canvas pixel.
struct MotionSrc {
  const double *params;
  int w, h;
  __device__ __forceinline__ void at(long /*p*/, int pair, int x, int y, float &u, float &v) const
  {
    motion_predict(motion_coef(params + 6 * (size_t)pair, w, h), 2 * x - (w - 1), 2 * y - (h - 1), u, v);
  }
};

inline size_t plate_lds_bytes(int K, int channels, int threads) { return (size_t)K * channels * threads * sizeof(float); }

// flow: the vectors of the n K samples on the canvas; frames: T x h x w x NOC; idx: n x K frame indices (-1 = absent), validated by
// the host; occ: n x K x H x W bytes or null; exclude: T x h x w bytes or null; ref / dst: n x H x W x NOC or null; count / code:
// n x H x W bytes or null; part: n x H x gridDim.x WarpPartial or null.
template <class Src, class T, int NOC>
__global__ __launch_bounds__(PLATE_TW * PLATE_MAX_ROWS) void plate_kernel(Src flow, const T *__restrict__ frames, const T *__restrict__ ref,
                                                                         const unsigned char *__restrict__ occ,
                                                                         const unsigned char *__restrict__ exclude,
                                                                         const int *__restrict__ idx, int K, int w, int h, int W, int H,
                                                                         int ox, int oy, int mode, int min_count, float fill,
                                                                         T *__restrict__ dst, unsigned char *__restrict__ count,
                                                                         unsigned char *__restrict__ code, WarpPartial *__restrict__ part)
{
  extern __shared__ float plate_lds[];
  const int img = blockIdx.z, nt = blockDim.x, t = threadIdx.x;
  const int X = blockIdx.x * PLATE_TW + t % PLATE_TW, Y = blockIdx.y * (nt / PLATE_TW) + t / PLATE_TW;
  if (Y >= H) return;                                           // (a whole wave; there is no barrier below)
  const bool live = X < W;
  const int x = X - ox, y = Y - oy;
  const long HW = (long)W * H, q = (long)Y * W + X;
  const size_t fpix = (size_t)w * h;
  const int *__restrict__ ix = idx + (size_t)img * K;
  float *col = plate_lds + t;
  const size_t cs = (size_t)nt;                                 // floats between two entries of a column

  int m = 0, cover = 0;
  float first[NOC];
#pragma unroll
  for (int ch = 0; ch < NOC; ++ch) first[ch] = 0.f;
  for (int k = 0; k < K; ++k) {
    const int b = ix[k];
    if (b < 0 || !live) continue;                               // absent: uniform over the workgroup
    const int pair = img * K + k;
    float u, v;
    flow.at((long)pair * HW + q, pair, x, y, u, v);
    if (!(__builtin_isfinite(u) && __builtin_isfinite(v))) continue;
    const float xx = (float)x + u, yy = (float)y + v;
    if (!warp_inside(xx, yy, w, h)) continue;
    ++cover;
    if (occ && occ[(size_t)pair * HW + q]) continue;
    if (exclude) {
      const int xi = warp_sat(floorf(xx), w), yi = warp_sat(floorf(yy), h);
      const int x1 = clampi(xi, w), x2 = clampi(xi + 1, w), y1 = clampi(yi, h), y2 = clampi(yi + 1, h);
      const unsigned char *__restrict__ e = exclude + (size_t)b * fpix;
      if (e[(size_t)y1 * w + x1] | e[(size_t)y1 * w + x2] | e[(size_t)y2 * w + x1] | e[(size_t)y2 * w + x2]) continue;
    }
    float s[NOC];
    warp_taps<T, NOC>(frames + (size_t)b * fpix * NOC, w, h, xx, yy, s);
    bool nan = false;
#pragma unroll
    for (int ch = 0; ch < NOC; ++ch) nan = nan || s[ch] != s[ch];
    if (nan) continue;
#pragma unroll
    for (int ch = 0; ch < NOC; ++ch) {
      col[(size_t)(m * NOC + ch) * cs] = s[ch];
      if (m == 0) first[ch] = s[ch];
    }
    ++m;
  }

  const unsigned cd = m >= min_count ? 0u : (cover < min_count ? 2u : 1u);
  float est[NOC];
#pragma unroll
  for (int ch = 0; ch < NOC; ++ch) est[ch] = fill;
  if (live && cd == 0) {
    if (mode == 0) {
      const int lo = (m - 1) >> 1, hi = m >> 1;
#pragma unroll
      for (int ch = 0; ch < NOC; ++ch) {
        const float *c = col + (size_t)ch * cs;
        float vlo = 0.f, vhi = 0.f;
        for (int j = 0; j < m; ++j) {
          const float sj = c[(size_t)(j * NOC) * cs];
          int r = 0;
          for (int i = 0; i < m; ++i) {
            const float si = c[(size_t)(i * NOC) * cs];
            r += (si < sj || (si == sj && i < j)) ? 1 : 0;
          }
          if (r == lo) vlo = sj;
          if (r == hi) vhi = sj;
        }
        est[ch] = lo == hi ? vlo : (vlo + vhi) * 0.5f;
      }
    } else {
#pragma unroll
      for (int ch = 0; ch < NOC; ++ch) {
        const float *c = col + (size_t)ch * cs;
        float sum = c[0];
        for (int j = 1; j < m; ++j) sum = sum + c[(size_t)(j * NOC) * cs];
        est[ch] = sum / (float)m;
      }
    }
  }

  unsigned c01 = 0, c23 = 0;
  double s_est = 0.0, s_first = 0.0;
  if (live) {
    const size_t p = (size_t)img * HW + (size_t)q;
    if (dst) {
#pragma unroll
      for (int ch = 0; ch < NOC; ++ch) {
        if constexpr (sizeof(T) == 4) dst[p * NOC + ch] = est[ch];
        else dst[p * NOC + ch] = (unsigned char)warp_to_u8(est[ch]);
      }
    }
    if (count) count[p] = (unsigned char)m;
    if (code) code[p] = (unsigned char)cd;
    if (part) {
      if (cd == 0) c01 = 1u; else if (cd == 1) c01 = 1u << 16; else c23 = 1u;
      c23 += (unsigned)m << 16;
      if (ref && cd == 0) {
#pragma unroll
        for (int ch = 0; ch < NOC; ++ch) {
          const float r = warp_elem(ref, p * NOC + ch);
          s_est += (double)fabsf(r - est[ch]);
          s_first += (double)fabsf(r - first[ch]);
        }
      }
    }
  }
  if (part) {                                                   // (uniform)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      c01 += __shfl_xor(c01, o, 64); c23 += __shfl_xor(c23, o, 64);
      s_est += __shfl_xor(s_est, o, 64); s_first += __shfl_xor(s_first, o, 64);
    }
    if (t % PLATE_TW == 0) {
      WarpPartial wp;
      wp.s[0] = s_est; wp.s[1] = s_first; wp.c01 = c01; wp.c23 = c23;
      part[((size_t)img * H + Y) * gridDim.x + blockIdx.x] = wp;
    }
  }
}

}  // namespace fotg
