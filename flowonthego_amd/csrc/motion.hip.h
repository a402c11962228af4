// motion.hip.h -- the single camera motion that explains a flow field, and the pixels that do not follow it: a robust least-squares
// fit of u = a00 x + a01 y + tx, v = a10 x + a11 y + ty (x, y in pixels of the w x h image) to the n x h x w x 2 flow F.
// model 0 translation (A = 0), 1 similarity (a00 = a11, a01 = -a10), 2 affine.  The definition, in order:
//
// Per pixel (x, y), integers and f32:
//   X = 2x - (w-1);  Y = 2y - (h-1)                 (centred, doubled: integers, |X| < w, |Y| < h)
//   u, v = F[y][x];  known = |u| <= 4096 && |v| <= 4096        (false for a NaN or an infinity)
//   U = (int)rintf(u * 256);  V = (int)rintf(v * 256)          (exact in f32 for a known pixel; |U|, |V| <= 2^20)
//   admissible = known && (no mask || mask[y][x] == 0)         (mask: the alphabet of the consistency check, 0 = valid)
// Round r = 0 .. iters selects the admissible pixels (r = 0) or those of them within thresh of the previous round's parameters
// (r > 0; "within" as in the classification below) and reduces twelve int64 sums over them, S[0 .. 11] =
//   n, sum X, sum Y, sum XX, sum XY, sum YY, sum U, sum XU, sum YU, sum V, sum XV, sum YV.
// For w, h <= 16384 (MOTION_MAX_DIM; beyond it the C-ABI returns FOTG_ERR_ARG) none can overflow: the largest, |sum XU|, is at
// most 2^28 pixels x 2^14 x 2^20 = 2^62.  Integer addition is associative, so the sums are the same bits whatever the reduction
// tree, the launch shape or the ending (one 64-bit integer atomic add per workgroup and sum, or per-workgroup partials folded by a
// second launch).  There are no floating-point atomics.
//
// Solve (motion_solve; f64, every operation rounded on its own, each S[k] converted to f64 first), c[0 .. 5] with
// U ~ c0 X + c1 Y + c2, V ~ c3 X + c4 Y + c5:
//   translation (needs n >= 1):  c2 = SU / n;  c5 = SV / n;  the rest 0
//   similarity  (needs n >= 2):  D = n (SXX + SYY) - (SX SX + SY SY), needs D > 0
//                                a = (n (SXU + SYV) - (SX SU + SY SV)) / D;   b = (n (SXV - SYU) - (SX SV - SY SU)) / D
//                                c0 = a; c1 = -b; c2 = ((SU - a SX) + b SY) / n;  c3 = b; c4 = a; c5 = ((SV - b SX) - a SY) / n
//   affine      (needs n >= 3):  the adjugate of [[SXX SXY SX] [SXY SYY SY] [SX SY n]]:
//                                A00 = SYY n - SY SY;  A01 = SX SY - SXY n;  A02 = SXY SY - SYY SX
//                                A11 = SXX n - SX SX;  A12 = SX SXY - SXX SY;  A22 = SXX SYY - SXY SXY
//                                det = (SXX A00 + SXY A01) + SX A02, needs det > 0
//                                c0 = ((A00 SXU + A01 SYU) + A02 SU) / det;  c1 = ((A01 SXU + A11 SYU) + A12 SU) / det
//                                c2 = ((A02 SXU + A12 SYU) + A22 SU) / det;  c3 .. c5 alike with SXV, SYV, SV
// then to the pixel frame, per row (c0 c1 c2) and (c3 c4 c5):
//   q_i = c_i / 256 (exact);  a_0 = 2 q0;  a_1 = 2 q1;  t = (q2 - q0 (double)(w-1)) - q1 (double)(h-1)
// params = [a00 a01 tx a10 a11 ty].  A round whose system is unusable (too few pixels, D or det not > 0) keeps the previous
// parameters (zeros before round 0) and clears the image's `fitted` flag for good; other images are unaffected.
//
// Classification and residual (motion_coef + motion_predict; f32, every operation rounded on its own), from the six f64 parameters:
//   per row: h0 = a_0 / 2;  h1 = a_1 / 2;  k0 = (float)h0;  k1 = (float)h1;  k2 = (float)((t + h0 (double)(w-1)) + h1 (double)(h-1))
//   pu = (k0 (float)X + k1 (float)Y) + k2;  pv alike;  du = u - pu;  dv = v - pv
//   follows = du du + dv dv <= thresh thresh          (thresh thresh: one f32 product)
// code = 3 for a pixel that is not known, else 2 for one the mask excludes, else 0 (follows the model) or 1 (does not: independent
// motion).  residual = (du, dv) at every pixel.  fotg_motion_flow writes (pu, pv): flow - motion_flow(params) is the residual bit
// for bit.  tests/motion_ref.py restates all of this in numpy.
//
// motion_pass_kernel<Src, PASS>: the launch shape of warp_kernel -- grid (ceil(w h / 1024), n), 256 threads, thread q of an image
// owns its pixels 4q .. 4q+3, the dense source read as two 16-byte loads where the address allows (warp_flow4), the fused source
// (UpsampleSrc) evaluated per pixel.  PASS: round 0, a later round, or the final pass that writes code / residual and counts the
// codes.  The twelve sums are reduced per thread (24 VGPRs), per wave (four DPP stages inside rows of 16 lanes, then xor shuffles by 16
// and 32, the twelve sums of a stage in flight together; a 64-bit value crosses lanes as its two halves and is added as 64 bits)
// and per workgroup (through LDS); threads 0 .. 11 then store them as the workgroup's partial for motion_fold_kernel (the default,
// which measured faster) or add them to the image's accumulators with one 64-bit atomic each.  motion_solve_kernel: one thread per image,
// reads and clears the accumulators, solves, writes the parameters: they never leave the device between rounds.
#pragma once
#include "common.h"
#include "flowsrc.hip.h"
#include "warp.hip.h"
#include "motion_model.hip.h"

namespace fotg {

enum { MOTION_THREADS = 256, MOTION_NSUM = 12, MOTION_NSTAT = 6, MOTION_MAX_DIM = 16384, MOTION_MAX_ITERS = 64 };
enum { MOTION_ROUND0 = 0, MOTION_ROUND = 1, MOTION_FINAL = 2 };

// the solve of the head of this file: false (c untouched) where the system is unusable
__host__ __device__ inline bool motion_solve(const long long (&S)[MOTION_NSUM], int model, double (&c)[6])
{
  const double n = (double)S[0], sx = (double)S[1], sy = (double)S[2], sxx = (double)S[3], sxy = (double)S[4], syy = (double)S[5];
  const double su = (double)S[6], sxu = (double)S[7], syu = (double)S[8], sv = (double)S[9], sxv = (double)S[10], syv = (double)S[11];
  if (model == 0) {
    if (S[0] < 1) return false;
    c[0] = 0.0; c[1] = 0.0; c[2] = su / n;
    c[3] = 0.0; c[4] = 0.0; c[5] = sv / n;
    return true;
  }
  if (model == 1) {
    if (S[0] < 2) return false;
    const double D = n * (sxx + syy) - (sx * sx + sy * sy);
    if (!(D > 0.0)) return false;
    const double a = (n * (sxu + syv) - (sx * su + sy * sv)) / D;
    const double b = (n * (sxv - syu) - (sx * sv - sy * su)) / D;
    c[0] = a; c[1] = -b; c[2] = ((su - a * sx) + b * sy) / n;
    c[3] = b; c[4] = a;  c[5] = ((sv - b * sx) - a * sy) / n;
    return true;
  }
  if (S[0] < 3) return false;
  const double A00 = syy * n - sy * sy, A01 = sx * sy - sxy * n, A02 = sxy * sy - syy * sx;
  const double A11 = sxx * n - sx * sx, A12 = sx * sxy - sxx * sy, A22 = sxx * syy - sxy * sxy;
  const double det = (sxx * A00 + sxy * A01) + sx * A02;
  if (!(det > 0.0)) return false;
  c[0] = ((A00 * sxu + A01 * syu) + A02 * su) / det;
  c[1] = ((A01 * sxu + A11 * syu) + A12 * su) / det;
  c[2] = ((A02 * sxu + A12 * syu) + A22 * su) / det;
  c[3] = ((A00 * sxv + A01 * syv) + A02 * sv) / det;
  c[4] = ((A01 * sxv + A11 * syv) + A12 * sv) / det;
  c[5] = ((A02 * sxv + A12 * syv) + A22 * sv) / det;
  return true;
}

// c (fixed point, centred, doubled) to the six pixel-frame parameters P
__host__ __device__ inline void motion_to_pixel_frame(const double (&c)[6], int w, int h, double *P)
{
  const double wx = (double)(w - 1), hy = (double)(h - 1);
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const double q0 = c[3 * r] * 0.00390625, q1 = c[3 * r + 1] * 0.00390625, q2 = c[3 * r + 2] * 0.00390625;
    P[3 * r] = q0 * 2.0;
    P[3 * r + 1] = q1 * 2.0;
    P[3 * r + 2] = (q2 - q0 * wx) - q1 * hy;
  }
}

// one stage of the wave's reduction inside rows of 16 lanes: every sum gets the value of the lane that the DPP control CTRL pairs
// its lane with (an involution, all lanes of the wave active), both halves moved, then one 64-bit add
template <int CTRL, int K>
__device__ __forceinline__ void motion_dpp_stage(long long (&s)[K])
{
  long long t[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(unsigned long long)s[k], CTRL, 0xf, 0xf, false);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)((unsigned long long)s[k] >> 32), CTRL, 0xf, 0xf, false);
    t[k] = (long long)(((unsigned long long)hi << 32) | lo);
  }
#pragma unroll
  for (int k = 0; k < K; ++k) s[k] += t[k];
}

// a selected pixel joins the twelve sums of the head of this file
__device__ __forceinline__ void motion_add12(long long (&s)[12], int X, int Y, float u, float v)
{
  const long long U = (int)rintf(u * 256.f), V = (int)rintf(v * 256.f);
  const long long Xl = X, Yl = Y;
  s[0] += 1;       s[1] += Xl;      s[2] += Yl;
  s[3] += Xl * Xl; s[4] += Xl * Yl; s[5] += Yl * Yl;
  s[6] += U;       s[7] += Xl * U;  s[8] += Yl * U;
  s[9] += V;       s[10] += Xl * V; s[11] += Yl * V;
}

// the mask bytes of a thread's nb (<= 4) pixels at o, byte i in bits 8i .. 8i+7: one 4-byte load where the address allows
__device__ __forceinline__ unsigned motion_mask4(const unsigned char *__restrict__ o, int nb)
{
  if (nb == 4 && (((size_t)o) & 3) == 0) return *reinterpret_cast<const unsigned *>(o);
  unsigned maskw = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (i < nb) maskw |= (unsigned)o[i] << (8 * i);
  return maskw;
}

// the wave's K sums in every lane, stage by stage, the K sums of a stage side by side: their lane crossings are independent and
// in flight together.  Within a row of 16 lanes the crossings are DPP moves (lane ^ 1, lane ^ 2, then the mirrors of 8 and of 16
// lanes: every lane of a row ends with the row's sum); across rows, xor shuffles by 16 and 32.  All lanes of the wave active.
template <int K>
__device__ __forceinline__ void motion_wave_reduce(long long (&s)[K])
{
  motion_dpp_stage<0xB1>(s);      // quad_perm [1 0 3 2]
  motion_dpp_stage<0x4E>(s);      // quad_perm [2 3 0 1]
  motion_dpp_stage<0x141>(s);     // row_half_mirror
  motion_dpp_stage<0x140>(s);     // row_mirror
#pragma unroll
  for (int o = 16; o <= 32; o <<= 1) {
    long long t[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)(unsigned long long)s[k], o, 64);
      const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)((unsigned long long)s[k] >> 32), o, 64);
      t[k] = (long long)(((unsigned long long)hi << 32) | lo);
    }
#pragma unroll
    for (int k = 0; k < K; ++k) s[k] += t[k];
  }
}

// the workgroup's K sums: per wave by lane crossings of the two halves, per workgroup through LDS; thread k < K then stores sum k
// to part[k] (part != null) or adds it to acc[k] with one 64-bit integer atomic.  Every thread of the workgroup calls it.
template <int K>
__device__ __forceinline__ void motion_block_reduce(long long (&s)[K], long long *__restrict__ acc, long long *__restrict__ part)
{
  motion_wave_reduce<K>(s);
  __shared__ long long ws[MOTION_THREADS / FOTG_WAVE][K];
  const int wave = threadIdx.x / FOTG_WAVE, lane = threadIdx.x % FOTG_WAVE;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) ws[wave][k] = s[k];
  }
  __syncthreads();
  if (threadIdx.x < K) {
    long long t = ws[0][threadIdx.x];
    for (int i = 1; i < MOTION_THREADS / FOTG_WAVE; ++i) t += ws[i][threadIdx.x];
    if (part) part[threadIdx.x] = t;
    else if (t != 0) atomicAdd(reinterpret_cast<unsigned long long *>(acc) + threadIdx.x, (unsigned long long)t);
  }
}

// flow: the vectors; mask: n x h x w bytes or null; params: n x 6 (PASS != MOTION_ROUND0).  The K sums (twelve, or the four code
// counts of the final pass) of image p go to acc[p acc_stride ..] by atomics, or, with part != null, to the workgroup's partial
// part[(p gridDim.x + blockIdx.x) K ..]; with both null nothing is counted.  code / residual: outputs of the final pass or null.
template <class Src, int PASS>
__global__ __launch_bounds__(MOTION_THREADS) void motion_pass_kernel(Src flow, const unsigned char *__restrict__ mask, int w, int h,
                                                                     const double *__restrict__ params, float thresh2,
                                                                     long long *__restrict__ acc, int acc_stride,
                                                                     long long *__restrict__ part, unsigned char *__restrict__ code,
                                                                     float *__restrict__ residual)
{
  constexpr int K = PASS == MOTION_FINAL ? 4 : MOTION_NSUM;
  const int pair = blockIdx.y;
  const long hw = (long)w * h, base = (long)pair * hw;
  const long r0 = 4 * ((long)blockIdx.x * blockDim.x + threadIdx.x);
  long long s[K];
#pragma unroll
  for (int k = 0; k < K; ++k) s[k] = 0;
  if (r0 < hw) {
    MotionCoef m = {};
    if (PASS != MOTION_ROUND0) m = motion_coef(params + 6 * (size_t)pair, w, h);
    const int nb = (int)(hw - r0 < 4 ? hw - r0 : 4);
    int y = (int)(r0 / w), x = (int)(r0 - (long)y * w);
    float u[4], v[4];
    warp_flow4(flow, base + r0, nb, pair, x, y, w, u, v);
    const unsigned maskw = mask ? motion_mask4(mask + (size_t)base + (size_t)r0, nb) : 0u;
    float res[8];
    unsigned word = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      res[2 * i] = res[2 * i + 1] = 0.f;
      if (i < nb) {
        const int X = 2 * x - (w - 1), Y = 2 * y - (h - 1);
        const bool known = motion_known(u[i], v[i]);
        unsigned cd = !known ? 3u : (((maskw >> (8 * i)) & 0xffu) != 0 ? 2u : 0u);
        if (PASS != MOTION_ROUND0) {
          float pu, pv;
          motion_predict(m, X, Y, pu, pv);
          const float du = u[i] - pu, dv = v[i] - pv;
          if (cd == 0 && !(du * du + dv * dv <= thresh2)) cd = 1;
          res[2 * i] = du; res[2 * i + 1] = dv;
        }
        if constexpr (PASS == MOTION_FINAL) {
          word |= cd << (8 * i);
          s[0] += cd == 0; s[1] += cd == 1; s[2] += cd == 2; s[3] += cd == 3;
        } else {
          if (cd == 0) motion_add12(s, X, Y, u[i], v[i]);
        }
      }
      if (++x == w) { x = 0; ++y; }
    }
    if (PASS == MOTION_FINAL) {
      if (residual) warp_store4<float, 2>(residual + 2 * (size_t)(base + r0), res, nb);
      if (code) warp_store_code4(code + (size_t)base + (size_t)r0, word, nb);
    }
  }
  if (acc || part)
    motion_block_reduce<K>(s, acc ? acc + (size_t)pair * acc_stride : nullptr, part ? part + ((size_t)pair * gridDim.x + blockIdx.x) * K : nullptr);
}

// grid n, 256 threads: the `blocks` partials (K sums each) of image blockIdx.x, added, into out[blockIdx.x out_stride ..]
template <int K>
__global__ __launch_bounds__(MOTION_THREADS) void motion_fold_kernel(const long long *__restrict__ part, int blocks,
                                                                     long long *__restrict__ out, int out_stride)
{
  const long long *p = part + (size_t)blockIdx.x * blocks * K;
  long long s[K];
#pragma unroll
  for (int k = 0; k < K; ++k) s[k] = 0;
  for (int j = threadIdx.x; j < blocks; j += MOTION_THREADS) {
#pragma unroll
    for (int k = 0; k < K; ++k) s[k] += p[(size_t)j * K + k];
  }
  motion_block_reduce<K>(s, nullptr, out + (size_t)blockIdx.x * out_stride);
}

#ifndef FOTG_MOTION_NO_PLAIN_KERNELS     // (layers.hip.h shares the templates and helpers above; these two are compiled once, by fotg_motion.hip)
// one thread per image: reads and clears the twelve accumulators, solves, writes the parameters (or keeps them and sets bad[i]).
// sums_out (n x 12) and stats (n x 6: [4] the pixels in this fit, [5] fitted) are written where given -- the last round's.
__global__ void motion_solve_kernel(long long *__restrict__ acc, int n, int model, int w, int h, double *__restrict__ params,
                                    long long *__restrict__ bad, long long *__restrict__ sums_out, long long *__restrict__ stats)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  long long S[MOTION_NSUM];
#pragma unroll
  for (int k = 0; k < MOTION_NSUM; ++k) {
    S[k] = acc[(size_t)i * MOTION_NSUM + k];
    acc[(size_t)i * MOTION_NSUM + k] = 0;
    if (sums_out) sums_out[(size_t)i * MOTION_NSUM + k] = S[k];
  }
  double c[6];
  long long b = bad[i];
  if (motion_solve(S, model, c)) {
    motion_to_pixel_frame(c, w, h, params + 6 * (size_t)i);
  } else {
    b = 1;
    bad[i] = 1;
  }
  if (stats) {
    stats[(size_t)i * MOTION_NSTAT + 4] = S[0];
    stats[(size_t)i * MOTION_NSTAT + 5] = b ? 0 : 1;
  }
}

// the model as a flow: (pu, pv) of the head of this file at every pixel.  The launch shape of motion_pass_kernel.
__global__ __launch_bounds__(MOTION_THREADS) void motion_flow_kernel(const double *__restrict__ params, int w, int h, float *__restrict__ flow)
{
  const int pair = blockIdx.y;
  const long hw = (long)w * h, base = (long)pair * hw;
  const long r0 = 4 * ((long)blockIdx.x * blockDim.x + threadIdx.x);
  if (r0 >= hw) return;
  const MotionCoef m = motion_coef(params + 6 * (size_t)pair, w, h);
  const int nb = (int)(hw - r0 < 4 ? hw - r0 : 4);
  int y = (int)(r0 / w), x = (int)(r0 - (long)y * w);
  float val[8];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    motion_predict(m, 2 * x - (w - 1), 2 * y - (h - 1), val[2 * i], val[2 * i + 1]);
    if (++x == w) { x = 0; ++y; }
  }
  warp_store4<float, 2>(flow + 2 * (size_t)(base + r0), val, nb);
}

#endif

}  // namespace fotg
