// chain.hip.h -- flow chaining: a position followed through the T flows of a sequence (long-range flow, point tracks), with the
// codes of fbcheck.hip.h / warp.hip.h (0 valid, 1 occluded, 2 leaves the frame, 3 unknown) telling where a chain got lost.
//
// A chain has a start position (X0, Y0), T forward flows F_0 .. F_{T-1} of one w x h sequence (F_k: frame k -> k+1) and optionally
// T backward flows B_k (frame k+1 -> k).  Its state is a displacement (Dx, Dy) = (0, 0), steps = 0 and code = 0.  All arithmetic
// f32, every operation rounded on its own (the library's -ffp-contract=off), in exactly this order:
//
//   start:  !isfinite(X0) || !isfinite(Y0) -> code 3;  else !warp_inside(X0, Y0, w, h) -> code 2
//   for k = 0 .. T-1 while code == 0:
//     X = X0 + Dx;  Y = Y0 + Dy
//     (u, v) = bilerp(F_k, X, Y)        fb_code's taps and lerp order (fb_sample of fbcheck.hip.h):
//                                       x0 = min((int)floorf(X), w-1), x1 = min(x0+1, w-1), ax = X - (float)x0 (y0, y1, ay alike),
//                                       per channel r0 = a (1-ax) + b ax, r1 likewise, value = r0 (1-ay) + r1 ay
//     !isfinite(u) || !isfinite(v)                 -> code 3, stop
//     Ex = Dx + u;  Ey = Dy + v;  Xn = X0 + Ex;  Yn = Y0 + Ey
//     !warp_inside(Xn, Yn, w, h)                   -> code 2, stop
//     if B:  (bu, bv) = bilerp(B_k, Xn, Yn)
//            du = u + bu, dv = v + bv;  lhs = du du + dv dv;  rhs = alpha1 ((u u + v v) + (bu bu + bv bv)) + alpha2
//            !(lhs < rhs)                          -> code 1, stop      (fb_consistent; a NaN in B lands here, as in fb_check)
//     Dx = Ex;  Dy = Ey;  steps = k + 1
//
// A stopped chain keeps its last accepted displacement.  Every tap index is derived from a position that has passed warp_inside
// (the start, or the Xn of the step before: X0 + Dx of step k+1 is the same f32 sum as Xn of step k) and is clamped, so no input
// value (NaN, +-inf, 1e30) can produce an out-of-range address; a chain that is not live samples position (0, 0) and discards it.
// Consequences, for T = 1 and integer starts: ax = ay = 0, so where all four taps of F_0 are finite (u, v) == F_0[y][x] and the
// displacement at the code-0 pixels is F_0 (compared with ==: a -0 becomes +0); with B, code is fb_check's forward mask byte for
// byte.  A non-finite vector in the tap to the right of, below or diagonally below a pixel makes the lerp (tap * 0 = NaN) and so
// the chain's code 3 where fb_check, which reads F_0[y][x] alone, still judges the pixel.
// tests/chain_ref.py restates all of this in numpy float32.
//
// chain_dense_kernel: grid (ceil(w h / 1024), n_seq), 256 threads, the launch shape of warp_kernel and fb_check_kernel: thread q
// owns the chains that start at pixels 4q .. 4q+3 of frame 0.  The loop over k is inside the kernel and the position lives in
// registers: nothing but the outputs goes to HBM.  chain_step is written without branches (a stopped chain reads the taps of
// pixel (0, 0), one broadcast address, and discards them), so the four chains of a thread are independent straight-line code and
// their gathers are in flight together; a thread leaves the loop when all four have stopped.  The taps are gathered through L2
// (neighbouring chains stay neighbours under a smooth flow); nothing is staged in LDS.  Outputs, each may be null: total
// (n_seq x h x w x 2 f32, the displacement), code (u8), steps (i32), stored as 16-byte / dword nontemporal stores where the
// thread's span is whole and aligned, elements otherwise.
// chain_points_kernel: one thread per point, grid (ceil(P / 256), n_seq); pts n_seq x P x 2 (x, y); traj n_seq x (T+1) x P x 2
// holds X0 + D after every step (traj[0] the start; the frozen position repeated once a chain has stopped).
// Sources (flowsrc.hip.h): DenseSrc reads n_seq x T flows, plane s T + k; UpsampleSrc evaluates upsample_crop4_kernel's value at
// each tap from the coarse flow k of a context, so the fused form equals the chain over fotg_upsample_crop's outputs byte for byte.
// Statistics, per sequence five unsigned 64-bit integers: chains ending with code 0, 1, 2, 3 and the sum of steps (beyond 32 bits
// at 1080p for T > 2071), reduced per thread, per wave (shuffles) and per workgroup (LDS), then one integer atomicAdd per
// workgroup and counter into a buffer the call has zeroed: integer sums in any order, so the same bits every run.
#pragma once
#include "common.h"
#include "fbcheck.hip.h"
#include "warp.hip.h"

namespace fotg {

enum { CHAIN_NSTAT = 5, CHAIN_THREADS = 256 };

struct ChainState {
  float dx, dy;            // the last accepted displacement
  int steps;               // accepted steps
  unsigned code;           // 0 while live
};

__device__ __forceinline__ ChainState chain_start(float X0, float Y0, int w, int h)
{
  ChainState s = {0.f, 0.f, 0, 0u};
  if (!__builtin_isfinite(X0) || !__builtin_isfinite(Y0)) s.code = 3;
  else if (!warp_inside(X0, Y0, w, h)) s.code = 2;
  return s;
}

// step k of the chain that started at (X0, Y0): flows F and (BW) B, plane `pair` whose first pixel is `base`
template <class Src, bool BW>
__device__ __forceinline__ void chain_step(const Src &F, const Src &B, int pair, long base, int k, float X0, float Y0, int w, int h,
                                           float alpha1, float alpha2, ChainState &s)
{
  const bool live = s.code == 0;
  const float X = live ? X0 + s.dx : 0.f, Y = live ? Y0 + s.dy : 0.f;
  float u, v;
  fb_sample(F, pair, base, X, Y, w, h, u, v);
  const bool known = __builtin_isfinite(u) && __builtin_isfinite(v);
  const float ex = s.dx + u, ey = s.dy + v;
  const float xn = X0 + ex, yn = Y0 + ey;
  const bool in = known && warp_inside(xn, yn, w, h);
  unsigned code = !known ? 3u : (!in ? 2u : 0u);
  if constexpr (BW) {
    const bool go = live && in;
    float bu, bv;
    fb_sample(B, pair, base, go ? xn : X, go ? yn : Y, w, h, bu, bv);
    if (in && !fb_consistent(u, v, bu, bv, alpha1, alpha2)) code = 1u;
  }
  if (live) {
    s.code = code;
    if (code == 0) { s.dx = ex; s.dy = ey; s.steps = k + 1; }
  }
}

// the workgroup's counts (c01: codes 0 | 1 << 16, c23: codes 2 | 3 << 16; at most 1024 chains) and its sum of steps, added to the
// five counters of the sequence.  Every thread of the workgroup calls it.
__device__ __forceinline__ void chain_block_stats(unsigned c01, unsigned c23, unsigned long long nsteps, unsigned long long *__restrict__ st)
{
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    c01 += __shfl_xor(c01, o, 64); c23 += __shfl_xor(c23, o, 64);
    nsteps += __shfl_xor(nsteps, o, 64);
  }
  __shared__ unsigned pc[CHAIN_THREADS / FOTG_WAVE][2];
  __shared__ unsigned long long ps[CHAIN_THREADS / FOTG_WAVE];
  const int wave = threadIdx.x / FOTG_WAVE, lane = threadIdx.x % FOTG_WAVE;
  if (lane == 0) { pc[wave][0] = c01; pc[wave][1] = c23; ps[wave] = nsteps; }
  __syncthreads();
  if (threadIdx.x < CHAIN_NSTAT) {
    unsigned long long r = 0;
    if (threadIdx.x < 4) {
      unsigned c = 0;
      for (int i = 0; i < CHAIN_THREADS / FOTG_WAVE; ++i) c += pc[i][threadIdx.x >> 1];
      r = (c >> (16 * (threadIdx.x & 1))) & 0xffffu;
    } else {
      for (int i = 0; i < CHAIN_THREADS / FOTG_WAVE; ++i) r += ps[i];
    }
    if (r) atomicAdd(st + threadIdx.x, r);
  }
}

// the thread's nb (<= 4) step counts to o: one 16-byte nontemporal store where the span is whole and aligned
__device__ __forceinline__ void chain_store_steps4(int *__restrict__ o, const int (&st)[4], int nb)
{
  typedef int vi4 __attribute__((ext_vector_type(4)));
  if (nb == 4 && (((size_t)o) & 15) == 0) {
    __builtin_nontemporal_store(vi4{st[0], st[1], st[2], st[3]}, reinterpret_cast<vi4 *>(o));
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (i < nb) o[i] = st[i];
  }
}

// fw, bw: the flows (bw unused without BW); total / code / steps: the outputs or null; stats: n_seq x 5, zeroed, or null
template <class Src, bool BW>
__global__ __launch_bounds__(CHAIN_THREADS) void chain_dense_kernel(Src fw, Src bw, int T, int w, int h, float alpha1, float alpha2,
                                                                    float *__restrict__ total, unsigned char *__restrict__ code,
                                                                    int *__restrict__ steps, unsigned long long *__restrict__ stats)
{
  const int seq = blockIdx.y;
  const long hw = (long)w * h, obase = (long)seq * hw;
  const long r0 = 4 * ((long)blockIdx.x * blockDim.x + threadIdx.x);
  unsigned c01 = 0, c23 = 0;
  unsigned long long nsteps = 0;
  if (r0 < hw) {
    const int nb = (int)(hw - r0 < 4 ? hw - r0 : 4);
    int y = (int)(r0 / w), x = (int)(r0 - (long)y * w);
    float X0[4], Y0[4];
    ChainState s[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      X0[i] = (float)x; Y0[i] = (float)y;
      s[i] = chain_start(X0[i], Y0[i], w, h);
      if (i >= nb) { X0[i] = Y0[i] = 0.f; s[i].code = 2; }        // (no such pixel: never live, never stored or counted)
      if (++x == w) { x = 0; ++y; }
    }
    for (int k = 0; k < T; ++k) {
      if (s[0].code != 0 && s[1].code != 0 && s[2].code != 0 && s[3].code != 0) break;
      const int pair = seq * T + k;
      const long base = (long)pair * hw;
#pragma unroll
      for (int i = 0; i < 4; ++i) chain_step<Src, BW>(fw, bw, pair, base, k, X0[i], Y0[i], w, h, alpha1, alpha2, s[i]);
    }
    float val[8];
    int st[4];
    unsigned word = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      val[2 * i] = s[i].dx; val[2 * i + 1] = s[i].dy; st[i] = s[i].steps;
      if (i < nb) {
        word |= s[i].code << (8 * i);
        const unsigned one = 1u << (16 * (s[i].code & 1));
        if (s[i].code < 2) c01 += one; else c23 += one;
        nsteps += (unsigned)s[i].steps;
      }
    }
    if (total) warp_store4<float, 2>(total + 2 * (size_t)(obase + r0), val, nb);
    if (code) warp_store_code4(code + (size_t)(obase + r0), word, nb);
    if (steps) chain_store_steps4(steps + (size_t)(obase + r0), st, nb);
  }
  if (stats) chain_block_stats(c01, c23, nsteps, stats + (size_t)seq * CHAIN_NSTAT);
}

// pts: n_seq x P x 2; traj: n_seq x (T+1) x P x 2 or null; code, steps: n_seq x P or null; stats as above
template <class Src, bool BW>
__global__ __launch_bounds__(CHAIN_THREADS) void chain_points_kernel(Src fw, Src bw, int T, int w, int h, float alpha1, float alpha2,
                                                                     int P, const float *__restrict__ pts, float *__restrict__ traj,
                                                                     unsigned char *__restrict__ code, int *__restrict__ steps,
                                                                     unsigned long long *__restrict__ stats)
{
  const int seq = blockIdx.y;
  const long hw = (long)w * h;
  const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
  unsigned c01 = 0, c23 = 0;
  unsigned long long nsteps = 0;
  if (p < P) {
    const size_t q = (size_t)seq * P + (size_t)p;
    const float X0 = pts[2 * q], Y0 = pts[2 * q + 1];
    ChainState s = chain_start(X0, Y0, w, h);
    float *tr = traj ? traj + 2 * ((size_t)seq * ((size_t)T + 1) * P + (size_t)p) : nullptr;
    if (tr) { tr[0] = X0; tr[1] = Y0; }
    for (int k = 0; k < T; ++k) {
      if (s.code == 0) {
        const int pair = seq * T + k;
        chain_step<Src, BW>(fw, bw, pair, (long)pair * hw, k, X0, Y0, w, h, alpha1, alpha2, s);
      } else if (!tr) {
        break;
      }
      if (tr) {
        tr += 2 * (size_t)P;
        tr[0] = X0 + s.dx; tr[1] = Y0 + s.dy;
      }
    }
    if (code) code[q] = (unsigned char)s.code;
    if (steps) steps[q] = s.steps;
    const unsigned one = 1u << (16 * (s.code & 1));
    if (s.code < 2) c01 = one; else c23 = one;
    nsteps = (unsigned)s.steps;
  }
  if (stats) chain_block_stats(c01, c23, nsteps, stats + (size_t)seq * CHAIN_NSTAT);
}

}  // namespace fotg
