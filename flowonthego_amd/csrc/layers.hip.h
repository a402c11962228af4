// layers.hip.h -- motion layers: up to eight parametric motions fitted to one flow, every pixel given to the nearest of them (the
// layered decomposition of Wang and Adelson on the pieces of motion.hip.h).  Inputs: the n x h x w x 2 flow F, an optional mask in
// the alphabet of the consistency check, `layers` K in 1 .. 8, `model` as in the motion fit, iters 0 .. 64, rounds 0 .. 64,
// thresh >= 0, an optional init n x K x 6 f64.  The definition, in order:
//
// Per pixel: X, Y, known, U, V and admissible exactly as at the head of motion.hip.h.  For a layer with parameters P,
//   (du, dv) = (u, v) - motion_predict(motion_coef(P, w, h), X, Y);  r(P) = du du + dv dv         (f32, every operation on its own)
//   within(P) = r(P) <= thresh thresh                                                             (thresh thresh: one f32 product)
// Every layer has parameters (zeros at first), a `live` and a `fitted` flag (0 at first), a seed tile (-1 at first), the twelve
// sums of its last fit and their pixel count (zeros at first).
//
// Seeding, layer by layer, k = 0 .. K-1 (skipped with init: every layer is then live and fitted with the caller's parameters, seed -2):
//   candidates = the admissible pixels that are within() of no live layer j < k             (a dead layer removes nothing)
//   k = 0:  no seed tile (its seed stays -1); rounds r = 0 .. iters select the candidates (r = 0) or the candidates within the
//           layer's parameters (r > 0), reduce the twelve sums, solve with `model`: the motion fit's procedure, params[0] equals
//           fotg_fit_motion's byte for byte
//   k >= 1: over tiles of 32 x 32 pixels (LAYERS_TILE; edge tiles partial; tile index = tile row x tiles per row + tile column)
//           count the candidates per tile.  The seed tile is the one with the most, the lowest index among equals; with no
//           candidate at all the layer is dead and keeps its zeros and seed -1.  The first parameters are the translation solve
//           (motion_solve, model 0) of the seed tile's n, sum U, sum V over its candidates.  Then iters + 1 rounds, each selecting
//           the candidates within the layer's current parameters, reducing the twelve sums and solving with `model`.
//   A round whose system is unusable keeps the previous parameters and clears `fitted`; the later rounds still run.  After the
//   last round live = fitted: a layer one of whose rounds was unusable is dead (its parameters stay as they are).
// Refinement, `rounds` times:
//   assign: best = none, rb = +infinity, (db) = (u, v); for the live layers j in ascending order: less = r_j < rb; if best is none
//           or less: best = j, db = (du_j, dv_j); if less: rb = r_j.  (The first live layer is taken as it comes, a later one only
//           where strictly nearer: ties go to the lower index, a NaN never displaces a value.)
//           joined = admissible and best is a layer and db.u db.u + db.v db.v <= thresh thresh
//   every live layer's twelve sums run over the pixels joined to it; it is solved with `model`; an unusable system keeps the
//   parameters and clears `fitted`, the layer stays live.
// Final pass: assign as above.  labels uint8: best where joined; 253 where admissible but not joined (within thresh of no layer, or
// no layer live); 254 where the mask excludes the pixel; 255 where it is unknown (unknown wins over masked).  residual = db (the
// flow itself when no layer is live).  records n x K x 8 int64: pixels labelled, pixels in the last fit, live, fitted, seed tile
// (-1: none, -2: init), then sum X, sum Y, sum U over the labelled pixels.  stats n x 4 int64: pixels of label 253, 254, 255 and
// the number of live layers.  sums n x K x 12: each layer's last fit.  Layers are not reordered.
// Integer sums are the same bits whatever the reduction tree, so every output has one value per input; tests/layers_ref.py
// restates all of this in numpy on tests/motion_ref.py.
//
// Kernels (256 threads; nothing waits between workgroups, no floating-point atomics, no private memory):
//   layers_tile_kernel<Src>      grid (tiles, n): one workgroup per tile, thread t its row t / 8, columns 4 (t % 8) .. + 3; the
//                                candidate test against the earlier live layers; n, sum U, sum V of the tile.
//   layers_select_kernel         grid n: the largest key (count << 32 | ~index) over the image's tiles, then the translation solve.
//   layers_pass_kernel<Src, M>   the launch shape of motion_pass_kernel (thread q owns pixels 4q .. 4q+3).  The layers' f32
//                                coefficients and live flags sit in LDS (wave-uniform reads).  M = LAYERS_ROUND: the twelve sums of
//                                one layer's seeding round, reduced by motion_block_reduce.  M = LAYERS_ASSIGN / LAYERS_FINAL: per
//                                layer *present in the wave* (ballot) the predicated sums (twelve; or count, X, Y, U, and the three
//                                label counts as a pseudo-layer K) are reduced across the wave with motion_wave_reduce (DPP stages and two xor
//                                shuffles), lane 0 stores them in the wave's row of an LDS table, and after one barrier the table
//                                leaves as the workgroup's partial.  No per-thread array is indexed by the layer.
//   layers_fold_kernel<NS>       grid (layers, n): the workgroups' partials added (motion_fold_kernel's shape, a layer per block).
//   layers_solve_kernel          one thread per (image, layer): motion_solve + motion_to_pixel_frame; the parameters and flags
//                                never leave the device between passes.
//   layers_records_kernel        one thread per (image, layer): records and stats.
#pragma once
#define FOTG_MOTION_NO_PLAIN_KERNELS            // motion.hip.h's two non-template kernels are compiled by fotg_motion.hip alone
#include "motion.hip.h"

namespace fotg {

enum { LAYERS_MAX = 8, LAYERS_TILE = 32, LAYERS_NREC = 8, LAYERS_NSTAT = 4, LAYERS_NST = 4, LAYERS_MAX_ROUNDS = 64 };
enum { LAYERS_ROUND = 0, LAYERS_ASSIGN = 1, LAYERS_FINAL = 2 };
enum { LAYERS_UNASSIGNED = 253, LAYERS_MASKED = 254, LAYERS_UNKNOWN = 255 };
// a layer's state on the device, LAYERS_NST int64 each
enum { LAYERS_ST_LIVE = 0, LAYERS_ST_FITTED = 1, LAYERS_ST_SEED = 2, LAYERS_ST_IN_FIT = 3 };

// the coefficients and live flags of an image's K layers into LDS; every thread of the workgroup calls it
__device__ __forceinline__ void layers_load(const double *__restrict__ params, const long long *__restrict__ st, int K, int w, int h,
                                            float (&coef)[LAYERS_MAX][6], int (&live)[LAYERS_MAX])
{
  if ((int)threadIdx.x < K) {
    const MotionCoef m = motion_coef(params + 6 * (size_t)threadIdx.x, w, h);
#pragma unroll
    for (int c = 0; c < 6; ++c) coef[threadIdx.x][c] = m.k[c];
    live[threadIdx.x] = st[(size_t)threadIdx.x * LAYERS_NST + LAYERS_ST_LIVE] != 0;
  }
  __syncthreads();
}

__device__ __forceinline__ MotionCoef layers_coef(const float (&coef)[LAYERS_MAX][6], int j)
{
  MotionCoef m;
#pragma unroll
  for (int c = 0; c < 6; ++c) m.k[c] = coef[j][c];
  return m;
}

// r(P) of the head of this file and its (du, dv)
__device__ __forceinline__ float layers_r(const MotionCoef &m, int X, int Y, float u, float v, float &du, float &dv)
{
  float pu, pv;
  motion_predict(m, X, Y, pu, pv);
  du = u - pu; dv = v - pv;
  return du * du + dv * dv;
}

// grid (tiles, n), tiles = tx ty: the candidates of layer k (admissible, within no live layer j < k) of one tile: their n, sum U,
// sum V to tiles_out[(image tiles + tile) 3 ..]
template <class Src>
__global__ __launch_bounds__(MOTION_THREADS) void layers_tile_kernel(Src flow, const unsigned char *__restrict__ mask, int w, int h, int tx,
                                                                     const double *__restrict__ params, const long long *__restrict__ st,
                                                                     int K, int k, float thresh2, long long *__restrict__ tiles_out)
{
  __shared__ float coef[LAYERS_MAX][6];
  __shared__ int live[LAYERS_MAX];
  const int pair = blockIdx.y;
  layers_load(params + 6 * (size_t)pair * K, st + (size_t)pair * K * LAYERS_NST, K, w, h, coef, live);
  const long base = (long)pair * w * h;
  const int y = (int)(blockIdx.x / tx) * LAYERS_TILE + (int)threadIdx.x / 8;
  const int x0 = (int)(blockIdx.x % tx) * LAYERS_TILE + 4 * ((int)threadIdx.x % 8);
  long long s[3] = {0, 0, 0};
  if (y < h) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int x = x0 + i;
      if (x < w) {
        const long p = base + (long)y * w + x;
        float u, v;
        flow.at(p, pair, x, y, u, v);
        bool cand = motion_known(u, v) && (!mask || mask[p] == 0);
        const int X = 2 * x - (w - 1), Y = 2 * y - (h - 1);
        for (int j = 0; j < k; ++j) {
          if (live[j]) {
            float du, dv;
            if (layers_r(layers_coef(coef, j), X, Y, u, v, du, dv) <= thresh2) cand = false;
          }
        }
        if (cand) {
          s[0] += 1; s[1] += (int)rintf(u * 256.f); s[2] += (int)rintf(v * 256.f);
        }
      }
    }
  }
  motion_block_reduce<3>(s, nullptr, tiles_out + ((size_t)pair * gridDim.x + blockIdx.x) * 3);
}

// grid n: the seed tile of layer k of image blockIdx.x among its `tiles` tiles, and the layer's first parameters
__global__ __launch_bounds__(MOTION_THREADS) void layers_select_kernel(const long long *__restrict__ tile_sums, int tiles, int w, int h,
                                                                       int K, int k, double *__restrict__ params, long long *__restrict__ st)
{
  const long long *t = tile_sums + (size_t)blockIdx.x * tiles * 3;
  unsigned long long key = 0;                   // (count, ~index): the most candidates, the lowest index among equals
  for (int j = threadIdx.x; j < tiles; j += MOTION_THREADS) {
    const unsigned long long c = ((unsigned long long)t[(size_t)j * 3] << 32) | (0xffffffffu - (unsigned)j);
    key = c > key ? c : key;
  }
  __shared__ unsigned long long keys[MOTION_THREADS];
  keys[threadIdx.x] = key;
  __syncthreads();
  for (int o = MOTION_THREADS / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o && keys[threadIdx.x + o] > keys[threadIdx.x]) keys[threadIdx.x] = keys[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  key = keys[0];
  long long *s = st + ((size_t)blockIdx.x * K + k) * LAYERS_NST;
  if ((key >> 32) == 0) return;                 // no candidate: dead, zeros, seed -1 (as layers_init_kernel left it)
  const int tile = (int)(0xffffffffu - (unsigned)key);
  long long S[MOTION_NSUM] = {};
  S[0] = t[(size_t)tile * 3]; S[6] = t[(size_t)tile * 3 + 1]; S[9] = t[(size_t)tile * 3 + 2];
  double c[6];
  motion_solve(S, 0, c);
  motion_to_pixel_frame(c, w, h, params + 6 * ((size_t)blockIdx.x * K + k));
  s[LAYERS_ST_LIVE] = 1; s[LAYERS_ST_FITTED] = 1; s[LAYERS_ST_SEED] = tile;
}

// The launch shape of motion_pass_kernel.  MODE LAYERS_ROUND: a seeding round of layer k (first: layer 0's round 0, without the
// test against its own parameters), the workgroup's twelve sums to part[(image gridDim.x + block) 12 ..].  LAYERS_ASSIGN: K x 12
// sums to part[(image gridDim.x + block) K 12 ..].  LAYERS_FINAL: labels and residual (each may be null) and (K + 1) x 4 sums to
// part[(image gridDim.x + block) (K + 1) 4 ..]: per layer count, X, Y, U of its labelled pixels, then the counts of 253, 254, 255.
template <class Src, int MODE>
__global__ __launch_bounds__(MOTION_THREADS) void layers_pass_kernel(Src flow, const unsigned char *__restrict__ mask, int w, int h,
                                                                     const double *__restrict__ params, const long long *__restrict__ st,
                                                                     int K, int k, int first, float thresh2, long long *__restrict__ part,
                                                                     unsigned char *__restrict__ labels, float *__restrict__ residual)
{
  constexpr int NS = MODE == LAYERS_FINAL ? 4 : MOTION_NSUM;
  constexpr int WAVES = MOTION_THREADS / FOTG_WAVE;
  __shared__ float coef[LAYERS_MAX][6];
  __shared__ int live[LAYERS_MAX];
  __shared__ long long tab[MODE == LAYERS_ROUND ? 1 : WAVES][LAYERS_MAX + 1][NS];
  const int pair = blockIdx.y;
  const int KL = MODE == LAYERS_FINAL ? K + 1 : K;
  if (MODE != LAYERS_ROUND) {
    for (int t = threadIdx.x; t < WAVES * (LAYERS_MAX + 1) * NS; t += MOTION_THREADS) (&tab[0][0][0])[t] = 0;
  }
  layers_load(params + 6 * (size_t)pair * K, st + (size_t)pair * K * LAYERS_NST, K, w, h, coef, live);
  const long hw = (long)w * h, base = (long)pair * hw;
  const long r0 = 4 * ((long)blockIdx.x * blockDim.x + threadIdx.x);
  const int nb = r0 < hw ? (int)(hw - r0 < 4 ? hw - r0 : 4) : 0;
  float u[4] = {0.f, 0.f, 0.f, 0.f}, v[4] = {0.f, 0.f, 0.f, 0.f};
  int X[4], Y[4];
  bool adm[4], known[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) { X[i] = Y[i] = 0; adm[i] = known[i] = false; }
  if (nb > 0) {
    int y = (int)(r0 / w), x = (int)(r0 - (long)y * w);
    warp_flow4(flow, base + r0, nb, pair, x, y, w, u, v);
    const unsigned maskw = mask ? motion_mask4(mask + (size_t)base + (size_t)r0, nb) : 0u;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      X[i] = 2 * x - (w - 1); Y[i] = 2 * y - (h - 1);
      known[i] = i < nb && motion_known(u[i], v[i]);
      adm[i] = known[i] && ((maskw >> (8 * i)) & 0xffu) == 0;
      if (++x == w) { x = 0; ++y; }
    }
  }
  if constexpr (MODE == LAYERS_ROUND) {
    long long s[NS];
#pragma unroll
    for (int q = 0; q < NS; ++q) s[q] = 0;
    bool sel[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) sel[i] = adm[i] && live[k];
    for (int j = 0; j <= k; ++j) {
      if (j < k ? live[j] != 0 : !first) {
        const MotionCoef m = layers_coef(coef, j);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          float du, dv;
          const bool in = layers_r(m, X[i], Y[i], u[i], v[i], du, dv) <= thresh2;
          sel[i] = sel[i] && (j < k ? !in : in);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (sel[i]) motion_add12(s, X[i], Y[i], u[i], v[i]);
    motion_block_reduce<NS>(s, nullptr, part + ((size_t)pair * gridDim.x + blockIdx.x) * NS);
  } else {
    int best[4];
    float rb[4], dub[4], dvb[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { best[i] = -1; rb[i] = __builtin_inff(); dub[i] = u[i]; dvb[i] = v[i]; }
    for (int j = 0; j < K; ++j) {
      if (live[j]) {
        const MotionCoef m = layers_coef(coef, j);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          float du, dv;
          const float r = layers_r(m, X[i], Y[i], u[i], v[i], du, dv);
          const bool less = r < rb[i];
          if (best[i] < 0 || less) { best[i] = j; dub[i] = du; dvb[i] = dv; }
          if (less) rb[i] = r;
        }
      }
    }
    int lab[4];                                   // the label, or 256 for a pixel past the image's end
    unsigned mine = 0;                            // the rows of the table this thread adds to
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bool joined = adm[i] && best[i] >= 0 && dub[i] * dub[i] + dvb[i] * dvb[i] <= thresh2;
      lab[i] = i >= nb ? 256 : (joined ? best[i] : (adm[i] ? (int)LAYERS_UNASSIGNED : (known[i] ? (int)LAYERS_MASKED : (int)LAYERS_UNKNOWN)));
      if (MODE == LAYERS_FINAL) {
        if (lab[i] < 256) mine |= 1u << (lab[i] < LAYERS_UNASSIGNED ? lab[i] : K);
      } else if (joined) {
        mine |= 1u << best[i];
      }
    }
    if constexpr (MODE == LAYERS_FINAL) {
      if (nb > 0) {
        if (residual) {
          float res[8];
#pragma unroll
          for (int i = 0; i < 4; ++i) { res[2 * i] = dub[i]; res[2 * i + 1] = dvb[i]; }
          warp_store4<float, 2>(residual + 2 * (size_t)(base + r0), res, nb);
        }
        if (labels) {
          unsigned word = 0;
#pragma unroll
          for (int i = 0; i < 4; ++i) word |= ((unsigned)lab[i] & 0xffu) << (8 * i);
          warp_store_code4(labels + (size_t)base + (size_t)r0, word, nb);
        }
      }
    }
    const int wave = threadIdx.x / FOTG_WAVE, lane = threadIdx.x % FOTG_WAVE;
#pragma unroll 1
    for (int L = 0; L < KL; ++L) {
      if (__ballot((mine >> L) & 1u) == 0) continue;          // wave-uniform: every lane of the wave reduces, or none
      long long s[NS];
#pragma unroll
      for (int q = 0; q < NS; ++q) s[q] = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        // (the pixel's products are formed here, per present layer: kept out of the loop they cost 88 registers and the occupancy)
        asm volatile("" : "+v"(X[i]), "+v"(Y[i]));
        if constexpr (MODE == LAYERS_FINAL) {
          if (L < K) {
            if (lab[i] == L) { s[0] += 1; s[1] += X[i]; s[2] += Y[i]; s[3] += (int)rintf(u[i] * 256.f); }
          } else {
            s[0] += lab[i] == LAYERS_UNASSIGNED; s[1] += lab[i] == LAYERS_MASKED; s[2] += lab[i] == LAYERS_UNKNOWN;
          }
        } else {
          if (lab[i] == L) motion_add12(s, X[i], Y[i], u[i], v[i]);
        }
      }
      motion_wave_reduce<NS>(s);
      if (lane == 0) {
#pragma unroll
        for (int q = 0; q < NS; ++q) tab[wave][L][q] = s[q];
      }
    }
    __syncthreads();
    long long *out = part + ((size_t)pair * gridDim.x + blockIdx.x) * KL * NS;
    for (int t = threadIdx.x; t < KL * NS; t += MOTION_THREADS) {
      long long a = 0;
#pragma unroll
      for (int wv = 0; wv < WAVES; ++wv) a += tab[wv][t / NS][t % NS];
      out[t] = a;
    }
  }
}

// grid (KL, n): the `blocks` partials (KL x NS sums each) of image blockIdx.y, row blockIdx.x, added into
// out[blockIdx.y out_stride + (k0 + blockIdx.x) NS ..]
template <int NS>
__global__ __launch_bounds__(MOTION_THREADS) void layers_fold_kernel(const long long *__restrict__ part, int blocks, long long *__restrict__ out,
                                                                     int out_stride, int k0)
{
  const int KL = gridDim.x;
  const long long *p = part + ((size_t)blockIdx.y * blocks * KL + blockIdx.x) * NS;
  long long s[NS];
#pragma unroll
  for (int q = 0; q < NS; ++q) s[q] = 0;
  for (int j = threadIdx.x; j < blocks; j += MOTION_THREADS) {
#pragma unroll
    for (int q = 0; q < NS; ++q) s[q] += p[(size_t)j * KL * NS + q];
  }
  motion_block_reduce<NS>(s, nullptr, out + (size_t)blockIdx.y * out_stride + (size_t)(k0 + blockIdx.x) * NS);
}

// one thread per (image, layer): the state before seeding (or the caller's init), the parameters zeroed (or init's)
__global__ void layers_init_kernel(int total, const double *__restrict__ init, double *__restrict__ params, long long *__restrict__ st,
                                   int K)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
#pragma unroll
  for (int c = 0; c < 6; ++c) params[6 * (size_t)i + c] = init ? init[6 * (size_t)i + c] : 0.0;
  long long *s = st + (size_t)i * LAYERS_NST;
  const bool start = init || i % K == 0;          // layer 0 needs no seed tile: its rounds always run
  s[LAYERS_ST_LIVE] = start; s[LAYERS_ST_FITTED] = start; s[LAYERS_ST_SEED] = init ? -2 : -1; s[LAYERS_ST_IN_FIT] = 0;
}

// one thread per (image, layer k0 <= k < k1): a live layer is solved from acc[(image (K + 1) + k) 12 ..]; close: the last seeding
// round, after which live = fitted.  sums_out (n x K x 12) where given.
__global__ void layers_solve_kernel(const long long *__restrict__ acc, int n, int K, int k0, int k1, int close, int model, int w, int h,
                                    double *__restrict__ params, long long *__restrict__ st, long long *__restrict__ sums_out)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * (k1 - k0)) return;
  const int img = i / (k1 - k0), k = k0 + i % (k1 - k0);
  long long *s = st + ((size_t)img * K + k) * LAYERS_NST;
  if (!s[LAYERS_ST_LIVE]) return;
  long long S[MOTION_NSUM];
#pragma unroll
  for (int q = 0; q < MOTION_NSUM; ++q) {
    S[q] = acc[((size_t)img * (K + 1) + k) * MOTION_NSUM + q];
    if (sums_out) sums_out[((size_t)img * K + k) * MOTION_NSUM + q] = S[q];
  }
  s[LAYERS_ST_IN_FIT] = S[0];
  double c[6];
  if (motion_solve(S, model, c)) motion_to_pixel_frame(c, w, h, params + 6 * ((size_t)img * K + k));
  else s[LAYERS_ST_FITTED] = 0;
  if (close) s[LAYERS_ST_LIVE] = s[LAYERS_ST_FITTED];
}

// one thread per (image, layer): the layer's record from the final pass's sums acc4[(image (K + 1) + k) 4 ..] and its state; the
// thread of layer 0 writes the image's stats as well.  records and stats may each be null.
__global__ void layers_records_kernel(const long long *__restrict__ acc4, const long long *__restrict__ st, int n, int K,
                                      long long *__restrict__ records, long long *__restrict__ stats)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * K) return;
  const int img = i / K, k = i % K;
  const long long *a = acc4 + ((size_t)img * (K + 1) + k) * 4, *s = st + (size_t)i * LAYERS_NST;
  if (records) {
    long long *r = records + (size_t)i * LAYERS_NREC;
    r[0] = a[0]; r[1] = s[LAYERS_ST_IN_FIT]; r[2] = s[LAYERS_ST_LIVE]; r[3] = s[LAYERS_ST_FITTED]; r[4] = s[LAYERS_ST_SEED];
    r[5] = a[1]; r[6] = a[2]; r[7] = a[3];
  }
  if (stats && k == 0) {
    const long long *c = acc4 + ((size_t)img * (K + 1) + K) * 4;
    long long nlive = 0;
    for (int j = 0; j < K; ++j) nlive += s[(size_t)j * LAYERS_NST + LAYERS_ST_LIVE] != 0;
    stats[(size_t)img * LAYERS_NSTAT] = c[0]; stats[(size_t)img * LAYERS_NSTAT + 1] = c[1]; stats[(size_t)img * LAYERS_NSTAT + 2] = c[2];
    stats[(size_t)img * LAYERS_NSTAT + 3] = nlive;
  }
}

}  // namespace fotg
