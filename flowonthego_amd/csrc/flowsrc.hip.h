// flowsrc.hip.h -- where the per-pixel passes over a flow (flowcolor.hip.h, fbcheck.hip.h) read their vectors from: a dense
// n x h x w x 2 flow, or the engine's coarse flow upsampled and cropped on the fly with exactly upsample_crop4_kernel's arithmetic
// (same source coordinate, same x 2^sc_l per tap, same three lerps in the same order), so a fused pass equals the pass over
// fotg_upsample_crop's output bit for bit.
#pragma once
#include "common.h"

namespace fotg {

// A dense flow: pixel p of the batch (linear, n x h x w) at flow[2 p].
struct DenseSrc {
  const float *flow;
  __device__ __forceinline__ void at(long p, int /*pair*/, int /*x*/, int /*y*/, float &u, float &v) const
  {
    u = flow[2 * p]; v = flow[2 * p + 1];
  }
};

// The coarse flow of a context (n x hl x wl x 2): upsample_crop4_kernel's value at output pixel (x, y) of the pair.
struct UpsampleSrc {
  const float *flow;
  long in_stride;          // floats per pair: wl * hl * 2
  int wl, hl, sc_l, x0, y0;
  __device__ __forceinline__ void coord(int d, int n, int &s0, int &s1, float &fr) const
  {
    const int N = 2 * d + 1 - (1 << sc_l);
    float fc = (float)N * __builtin_ldexpf(1.0f, -(sc_l + 1));
    int si = (int)floorf(fc); fc -= si;
    if (si < 0) { fc = 0; si = 0; }
    if (si >= n - 1) { fc = 0; si = n - 1; }
    s0 = si; s1 = si + 1 < n ? si + 1 : n - 1; fr = fc;
  }
  __device__ __forceinline__ void at(long /*p*/, int pair, int x, int y, float &u, float &v) const
  {
    int sy, sy1, sx, sx1; float fy, fx;
    coord(y + y0, hl, sy, sy1, fy);
    coord(x + x0, wl, sx, sx1, fx);
    const float *f = flow + (size_t)pair * in_stride;
    const float scf = (float)(1 << sc_l);
    float r[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      float v00 = f[2 * ((size_t)sy * wl + sx) + c], v01 = f[2 * ((size_t)sy * wl + sx1) + c];
      float v10 = f[2 * ((size_t)sy1 * wl + sx) + c], v11 = f[2 * ((size_t)sy1 * wl + sx1) + c];
      if (sc_l != 0) { v00 *= scf; v01 *= scf; v10 *= scf; v11 *= scf; }
      const float a0 = v00 * (1.f - fx) + v01 * fx;
      const float a1 = v10 * (1.f - fx) + v11 * fx;
      r[c] = a0 * (1.f - fy) + a1 * fy;
    }
    u = r[0]; v = r[1];
  }
};

}  // namespace fotg
