// motion_model.hip.h -- the motion model as a flow, for every pass that evaluates it per pixel (motion.hip.h fits and classifies with
// it, histograms.hip.h subtracts it): the f32 coefficients of the six pixel-frame parameters, the prediction at a pixel, and which
// vectors count as known.  The arithmetic is defined at the head of motion.hip.h ("Classification and residual").
#pragma once
#include "common.h"

namespace fotg {

struct MotionCoef { float k[6]; };

// the f32 coefficients of the prediction in the centred frame from the six pixel-frame parameters P
__host__ __device__ inline MotionCoef motion_coef(const double *P, int w, int h)
{
  const double wx = (double)(w - 1), hy = (double)(h - 1);
  MotionCoef m;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const double h0 = P[3 * r] * 0.5, h1 = P[3 * r + 1] * 0.5;
    m.k[3 * r] = (float)h0;
    m.k[3 * r + 1] = (float)h1;
    m.k[3 * r + 2] = (float)((P[3 * r + 2] + h0 * wx) + h1 * hy);
  }
  return m;
}

__host__ __device__ inline void motion_predict(const MotionCoef &m, int X, int Y, float &pu, float &pv)
{
  const float Xf = (float)X, Yf = (float)Y;
  pu = (m.k[0] * Xf + m.k[1] * Yf) + m.k[2];
  pv = (m.k[3] * Xf + m.k[4] * Yf) + m.k[5];
}

__host__ __device__ inline bool motion_known(float u, float v) { return fabsf(u) <= 4096.f && fabsf(v) <= 4096.f; }

}  // namespace fotg
