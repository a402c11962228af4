// blockmotion.hip.h -- block motion vectors from a dense flow, for a video encoder: one quarter-pel vector per B x B block of the
// frame, chosen among a few vectors the flow proposes because it makes the motion-compensated prediction cheap, with its SAD.
// Integer arithmetic from the first step to the last, so any reduction order gives the same bytes.  The definition, in order:
//
// Inputs: cur, ref uint8 frames n x h x w x c, c in {1, 3}; flow n x h x w x 2 f32 from cur to ref, cur(x) ~ ref(x + flow(x)); mask
// null or n x h x w bytes in the alphabet of the consistency check (only 0 is valid); B in {8, 16, 32}; refine in {0, 1, 2, 3};
// 1 <= w, h <= 16384 (BM_MAX_DIM).
//
// Per pixel:
//   known = |u| <= 4096 && |v| <= 4096                       (false for a NaN or an infinity)
//   Qx = (int)rintf(u * 4);  Qy = (int)rintf(v * 4)          (quarter pixels; the product is exact, to nearest even, |Q| <= 16384)
//   admissible = known && (no mask || mask == 0)
// Block grid: bw = ceil(w / B), bh = ceil(h / B); block (bx, by) covers x in [bx B, min(bx B + B, w)) and y alike.  Pixels beyond
// the frame do not exist: they add nothing to any sum.
//
// Prediction of pixel (x, y), channel k, by the vector (mx, my):
//   ix = 4 x + mx;  X0 = ix >> 2 (floor);  fx = ix & 3;  iy, Y0, fy alike
//   a, b, c, d = ref at (X0, Y0), (X0 + 1, Y0), (X0, Y0 + 1), (X0 + 1, Y0 + 1), every coordinate clamped on its own to the frame
//   pred = ((4 - fx)(4 - fy) a + fx (4 - fy) b + (4 - fx) fy c + fx fy d + 8) >> 4
// SAD(m) = sum |cur - pred| over the block's pixels and channels (at most 32 32 3 255).
//
// Candidates, in this order; one with nothing to compute from is absent:
//   0  the zero vector (always present)
//   1  the block mean: with S = sum Q over the block's admissible pixels and m their count, floor((2 S + m) / (2 m)) per component
//   2  Q of the pixel (min(bx B + B/2, w - 1), min(by B + B/2, h - 1)), if it is admissible
//   3 .. 6  the means, by the same rule, of the four B/2 x B/2 quadrants clipped to the frame (top-left, top-right, bottom-left,
//      bottom-right), each a candidate for the whole block
// The winner is the lowest SAD, the lowest index among equals (a duplicate vector is skipped: it cannot win).
//
// Refinement: the steps are the last `refine` entries of (4, 2, 1).  Per step s the eight vectors m + s (dx, dy), (dx, dy) in the
// order (-1,-1) (0,-1) (1,-1) (-1,0) (1,0) (-1,1) (0,1) (1,1), without those with a component beyond +-16384; the vector moves to
// the lowest SAD only if that is strictly lower than the current one, to the earliest among equals.  moved = any step moved it.
//
// Outputs per block: mv int16 x 2 (quarter pixels), cost uint32 x 2 = [SAD of the final vector, SAD of the zero vector], kind uint8 =
// the winning candidate | (8 if moved).  Optional: pred, shaped like cur, the prediction by each block's final vector; stats int64
// x 11 per image = sum SAD, sum zero-vector SAD, sum (cur - pred)^2, blocks moved, blocks per winning candidate 0 .. 6.
// tests/blockmotion_ref.py restates all of this in numpy.
//
// blockmv_kernel<Src, NOC, B>: one wave64 per block, four blocks per 256-thread workgroup, grid (ceil(bw bh / 4), n).  A lane
// owns 1 (B = 8), 4 (B = 16) or 4 x 4 (B = 32: four adjacent pixels in the rows lr, lr + 8, lr + 16, lr + 24) pixels of cur, held in
// registers for the whole block.  The vector sums of the four quadrants (the block's are their sum) are reduced by the DPP +
// xor-shuffle ladder that motion.hip.h uses; lanes 0 .. 13 then each hold one component of one candidate (the ten divisions run
// side by side) and the candidate loop reads them back with v_readlane.  Per candidate the wave stages the (B + 1)^2 x c window of
// ref the vector needs in its own slice of LDS, clamped as it loads; per refinement step one (B + 3)^2 window, which serves the current
// vector and all eight neighbours, so the byte gathers from global memory happen once per window, not once per tap.  A SAD is a
// per-lane sum over LDS taps and one wave reduction; the decisions are wave-uniform (v_readfirstlane).  A wave never waits for
// another wave: there is no workgroup barrier.  pred leaves as dwords where the address allows (B >= 16), bytes otherwise.  The
// statistics are folded from cost, kind and a per-block squared-error plane by blockmv_fold_kernel, one workgroup per image.
// (blockmv_*, not blockmotion_*: the resource-table test of the motion fit counts every kernel whose name contains "motion_".)
#pragma once
#include "common.h"
#include "flowsrc.hip.h"

namespace fotg {

enum { BM_THREADS = 256, BM_WAVES = BM_THREADS / FOTG_WAVE, BM_NSTAT = 11, BM_QMAX = 16384, BM_MAX_DIM = 16384 };

template <int NOC, int B>
struct BmGeom {
  static constexpr int W4 = B == 8 ? 1 : 4;                 // adjacent pixels a lane owns in a row
  static constexpr int LPR = B / W4;                        // lanes per block row: 8, 4, 8
  static constexpr int LROWS = FOTG_WAVE / LPR;             // block rows one pass of the wave covers: 8, 16, 8
  static constexpr int ROWS = B / LROWS;                    // rows a lane owns: 1, 1, 4
  static constexpr int NB = W4 * NOC;                       // bytes a lane owns per row
  static constexpr int WMAX = B + 3;                        // the widest window
  static constexpr int STRIDE = (WMAX * NOC + 3) & ~3;      // bytes per window row in LDS
  static constexpr int LDS_WAVE = STRIDE * WMAX;
};

__device__ __forceinline__ bool bm_known(float u, float v) { return fabsf(u) <= 4096.f && fabsf(v) <= 4096.f; }

// the K sums over the wave, in every lane (all 64 lanes active): motion.hip.h's ladder on 32-bit values
template <int K>
__device__ __forceinline__ void bm_wave_sum(int (&s)[K])
{
#define BM_STAGE(CTRL)                                                                                                   \
  {                                                                                                                      \
    int t[K];                                                                                                            \
    _Pragma("unroll") for (int k = 0; k < K; ++k) t[k] = __builtin_amdgcn_update_dpp(0, s[k], CTRL, 0xf, 0xf, false);    \
    _Pragma("unroll") for (int k = 0; k < K; ++k) s[k] += t[k];                                                          \
  }
  BM_STAGE(0xB1)       // quad_perm [1 0 3 2]
  BM_STAGE(0x4E)       // quad_perm [2 3 0 1]
  BM_STAGE(0x141)      // row_half_mirror
  BM_STAGE(0x140)      // row_mirror
#undef BM_STAGE
#pragma unroll
  for (int o = 16; o <= 32; o <<= 1) {
    int t[K];
#pragma unroll
    for (int k = 0; k < K; ++k) t[k] = __shfl_xor(s[k], o, 64);
#pragma unroll
    for (int k = 0; k < K; ++k) s[k] += t[k];
  }
}

// one sum over the wave as a wave-uniform value
__device__ __forceinline__ int bm_wave_sum1(int v)
{
  int s[1] = {v};
  bm_wave_sum<1>(s);
  return __builtin_amdgcn_readfirstlane(s[0]);
}

// the wave's LDS slice is written and read by the wave alone: order its own accesses, wait for nobody else
__device__ __forceinline__ void bm_wave_sync()
{
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

// the first nb of NBYTES bytes at p into v (the rest 0): dwords where the address allows
template <int NBYTES>
__device__ __forceinline__ void bm_load(const unsigned char *__restrict__ p, int nb, int (&v)[NBYTES])
{
#pragma unroll
  for (int i = 0; i < NBYTES; ++i) v[i] = 0;
  if (nb <= 0) return;
  if (NBYTES % 4 == 0 && nb == NBYTES && (((size_t)p) & 3) == 0) {
#pragma unroll
    for (int i = 0; i < NBYTES / 4; ++i) {
      const unsigned t = reinterpret_cast<const unsigned *>(p)[i];
#pragma unroll
      for (int j = 0; j < 4; ++j) v[4 * i + j] = (int)((t >> (8 * j)) & 0xffu);
    }
  } else {
#pragma unroll
    for (int i = 0; i < NBYTES; ++i)
      if (i < nb) v[i] = p[i];
  }
}

template <int NBYTES>
__device__ __forceinline__ void bm_store(unsigned char *__restrict__ p, int nb, const int (&v)[NBYTES])
{
  if (nb <= 0) return;
  if (NBYTES % 4 == 0 && nb == NBYTES && (((size_t)p) & 3) == 0) {
#pragma unroll
    for (int i = 0; i < NBYTES / 4; ++i)
      reinterpret_cast<unsigned *>(p)[i] = (unsigned)v[4 * i] | ((unsigned)v[4 * i + 1] << 8) | ((unsigned)v[4 * i + 2] << 16) |
                                           ((unsigned)v[4 * i + 3] << 24);
  } else {
#pragma unroll
    for (int i = 0; i < NBYTES; ++i)
      if (i < nb) p[i] = (unsigned char)v[i];
  }
}

// the (B + 1 + 2 M)^2 x NOC window of the image `ref` (w x h x NOC) whose first tap is (X0, Y0), every coordinate clamped to the
// frame, into the wave's slice: row r at win + r STRIDE
template <int NOC, int B, int M>
__device__ __forceinline__ void bm_stage(unsigned char *win, const unsigned char *__restrict__ ref, int w, int h, int X0, int Y0,
                                         int lane)
{
  using G = BmGeom<NOC, B>;
  constexpr int WW = B + 1 + 2 * M, RL = WW * NOC, TOTAL = RL * WW;
  bm_wave_sync();                                            // the reads of the previous window are done
#pragma unroll 4
  for (int e = lane; e < TOTAL; e += FOTG_WAVE) {
    const int r = e / RL, j = e - r * RL, c = j / NOC, ch = j - c * NOC;
    const int y = clampi(Y0 + r, h), x = clampi(X0 + c, w);
    win[r * G::STRIDE + j] = ref[((size_t)y * w + x) * NOC + ch];
  }
  bm_wave_sync();
}

// the lane's share of SAD (OUT = false) or of the squared error (OUT = true, which also returns the predictions in pr) of the
// vector whose first tap is (ox, oy) of the staged window, with the fractions (fx, fy).  nv[r]: the lane's valid bytes in row r.
template <int NOC, int B, bool OUT>
__device__ __forceinline__ int bm_eval(const unsigned char *win, int ox, int oy, int fx, int fy, int px0, int lr,
                                       const int (&cu)[BmGeom<NOC, B>::ROWS][BmGeom<NOC, B>::NB], const int (&nv)[BmGeom<NOC, B>::ROWS],
                                       int (&pr)[BmGeom<NOC, B>::ROWS][BmGeom<NOC, B>::NB])
{
  using G = BmGeom<NOC, B>;
  const int w00 = (4 - fx) * (4 - fy), w01 = fx * (4 - fy), w10 = (4 - fx) * fy, w11 = fx * fy;
  int s = 0;
#pragma unroll
  for (int r = 0; r < G::ROWS; ++r) {
    const unsigned char *p0 = win + (oy + lr + r * G::LROWS) * G::STRIDE + (ox + px0) * NOC, *p1 = p0 + G::STRIDE;
    int t0[G::NB + NOC], t1[G::NB + NOC];
#pragma unroll
    for (int i = 0; i < G::NB + NOC; ++i) { t0[i] = p0[i]; t1[i] = p1[i]; }
#pragma unroll
    for (int i = 0; i < G::NB; ++i) {
      const int p = (w00 * t0[i] + w01 * t0[i + NOC] + w10 * t1[i] + w11 * t1[i + NOC] + 8) >> 4;
      const int d = cu[r][i] - p;
      if (OUT) pr[r][i] = p;
      s += i < nv[r] ? (OUT ? d * d : (d < 0 ? -d : d)) : 0;
    }
  }
  return s;
}

// flow: the vectors; cur, ref: n x h x w x NOC bytes; mask: n x h x w bytes or null; bw x bh: the block grid.  mv (n x bh x bw x 2),
// cost (n x bh x bw x 2), kind (n x bh x bw): outputs; pred (like cur) and sse (n x bh x bw, the block's squared error for the
// statistics): outputs or null.
template <class Src, int NOC, int B>
__global__ __launch_bounds__(BM_THREADS) void blockmv_kernel(Src flow, const unsigned char *__restrict__ cur,
                                                                 const unsigned char *__restrict__ ref,
                                                                 const unsigned char *__restrict__ mask, int w, int h, int bw, int bh,
                                                                 int refine, short *__restrict__ mv, unsigned *__restrict__ cost,
                                                                 unsigned char *__restrict__ kind, unsigned char *__restrict__ pred,
                                                                 unsigned *__restrict__ sse)
{
  using G = BmGeom<NOC, B>;
  __shared__ __attribute__((aligned(16))) unsigned char lds[BM_WAVES][G::LDS_WAVE];
  const int wave = threadIdx.x / FOTG_WAVE, lane = threadIdx.x % FOTG_WAVE;
  const int pair = blockIdx.y, nblk = bw * bh;
  const int blk = __builtin_amdgcn_readfirstlane((int)blockIdx.x * BM_WAVES + wave);
  if (blk >= nblk) return;                                   // whole waves leave: no barrier follows
  unsigned char *win = lds[wave];
  const int by = blk / bw, bx = blk - by * bw, x0 = bx * B, y0 = by * B;
  const int px0 = (lane % G::LPR) * G::W4, lr = lane / G::LPR;
  const size_t img = (size_t)pair * w * h;
  const unsigned char *refi = ref + img * NOC;
  const int nvx = min(max(w - (x0 + px0), 0), G::W4);        // the lane's pixels inside the frame, per row

  // the lane's pixels of cur, and its share of the quadrants' vector sums: s[3 q + 0 .. 2] = sum Qx, sum Qy, count of quadrant q
  int cu[G::ROWS][G::NB], nv[G::ROWS], s[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) s[k] = 0;
#pragma unroll
  for (int r = 0; r < G::ROWS; ++r) {
    const int py = lr + r * G::LROWS, y = y0 + py, x = x0 + px0;
    const int np = y < h ? nvx : 0;
    nv[r] = np * NOC;
    const size_t p = img + (size_t)y * w + x;
    bm_load<G::NB>(cur + p * NOC, nv[r], cu[r]);
    int sx = 0, sy = 0, sm = 0;
#pragma unroll
    for (int i = 0; i < G::W4; ++i) {
      if (i < np) {
        float u, v;
        flow.at((long)(p + i), pair, x + i, y, u, v);
        if (bm_known(u, v) && (!mask || mask[p + i] == 0)) {
          sx += (int)rintf(u * 4.f); sy += (int)rintf(v * 4.f); sm += 1;
        }
      }
    }
    const int ql = 2 * (py >= B / 2) + (px0 >= B / 2);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      s[3 * q] += ql == q ? sx : 0; s[3 * q + 1] += ql == q ? sy : 0; s[3 * q + 2] += ql == q ? sm : 0;
    }
  }
  bm_wave_sum<12>(s);

  // lane 2 k + comp holds component comp of candidate k (cv) and whether the candidate is present (cp)
  int cv = 0, cp = 0;
  {
    const int cxp = min(x0 + B / 2, w - 1), cyp = min(y0 + B / 2, h - 1);
    const size_t pc = img + (size_t)cyp * w + cxp;
    float uc, vc;
    flow.at((long)pc, pair, cxp, cyp, uc, vc);
    const bool cadm = bm_known(uc, vc) && (!mask || mask[pc] == 0);
    const int k = lane >> 1, comp = lane & 1;
    int S = 0, m = 0;
    if (k == 1) {
      S = s[comp] + s[3 + comp] + s[6 + comp] + s[9 + comp];
      m = s[2] + s[5] + s[8] + s[11];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (k == 3 + q) { S = s[3 * q + comp]; m = s[3 * q + 2]; }
    if (m > 0) {
      const int a = 2 * S + m, b = 2 * m;
      int q = a / b;
      if (a - q * b < 0) --q;                                // the floor: / truncates
      cv = q; cp = 1;
    }
    if (k == 0) cp = 1;
    if (k == 2 && cadm) { cv = (int)rintf((comp ? vc : uc) * 4.f); cp = 1; }
  }

  int none[G::ROWS][G::NB];
  int bmx = 0, bmy = 0, bk = 0, bs = 0, zs = 0;
  for (int k = 0; k < 7; ++k) {
    const int mx = __builtin_amdgcn_readlane(cv, 2 * k), my = __builtin_amdgcn_readlane(cv, 2 * k + 1);
    if (!__builtin_amdgcn_readlane(cp, 2 * k) || (k > 0 && mx == bmx && my == bmy)) continue;
    bm_stage<NOC, B, 0>(win, refi, w, h, x0 + (mx >> 2), y0 + (my >> 2), lane);
    const int sad = bm_wave_sum1(bm_eval<NOC, B, false>(win, 0, 0, mx & 3, my & 3, px0, lr, cu, nv, none));
    if (k == 0) { zs = bs = sad; }
    else if (sad < bs) { bs = sad; bmx = mx; bmy = my; bk = k; }
  }

  bool moved = false;
  for (int t = 3 - refine; t < 3; ++t) {
    const int step = 4 >> t, ox0 = (bmx >> 2) - 1, oy0 = (bmy >> 2) - 1;
    bm_stage<NOC, B, 1>(win, refi, w, h, x0 + ox0, y0 + oy0, lane);
    int nmx = bmx, nmy = bmy, ns = bs;
    for (int i = 0; i < 8; ++i) {
      const int j = i + (i >= 4), dy = j / 3 - 1, dx = j - 3 * (dy + 1) - 1;
      const int mx = bmx + step * dx, my = bmy + step * dy;
      if (mx < -BM_QMAX || mx > BM_QMAX || my < -BM_QMAX || my > BM_QMAX) continue;
      const int sad = bm_wave_sum1(bm_eval<NOC, B, false>(win, (mx >> 2) - ox0, (my >> 2) - oy0, mx & 3, my & 3, px0, lr, cu, nv, none));
      if (sad < ns) { ns = sad; nmx = mx; nmy = my; }
    }
    if (ns < bs) { bs = ns; bmx = nmx; bmy = nmy; moved = true; }
  }

  const size_t ob = (size_t)pair * nblk + blk;
  if (lane == 0) {
    mv[2 * ob] = (short)bmx; mv[2 * ob + 1] = (short)bmy;
    cost[2 * ob] = (unsigned)bs; cost[2 * ob + 1] = (unsigned)zs;
    kind[ob] = (unsigned char)(bk | (moved ? 8 : 0));
  }
  if (pred || sse) {
    int pr[G::ROWS][G::NB];
    bm_stage<NOC, B, 0>(win, refi, w, h, x0 + (bmx >> 2), y0 + (bmy >> 2), lane);
    const int se = bm_wave_sum1(bm_eval<NOC, B, true>(win, 0, 0, bmx & 3, bmy & 3, px0, lr, cu, nv, pr));
    if (sse && lane == 0) sse[ob] = (unsigned)se;
    if (pred) {
#pragma unroll
      for (int r = 0; r < G::ROWS; ++r)
        bm_store<G::NB>(pred + (img + (size_t)(y0 + lr + r * G::LROWS) * w + x0 + px0) * NOC, nv[r], pr[r]);
    }
  }
}

// grid n, 256 threads: the eleven statistics of image blockIdx.x from its nblk blocks (64-bit integer sums, a tree through LDS)
__global__ __launch_bounds__(BM_THREADS) void blockmv_fold_kernel(const unsigned *__restrict__ cost,
                                                                      const unsigned char *__restrict__ kind,
                                                                      const unsigned *__restrict__ sse, int nblk,
                                                                      long long *__restrict__ stats)
{
  __shared__ long long sh[BM_NSTAT][BM_THREADS];
  const size_t base = (size_t)blockIdx.x * nblk;
  long long s[BM_NSTAT];
#pragma unroll
  for (int k = 0; k < BM_NSTAT; ++k) s[k] = 0;
  for (int j = threadIdx.x; j < nblk; j += BM_THREADS) {
    const int kd = kind[base + j];
    s[0] += cost[2 * (base + j)]; s[1] += cost[2 * (base + j) + 1]; s[2] += sse[base + j]; s[3] += (kd >> 3) & 1;
#pragma unroll
    for (int q = 0; q < 7; ++q) s[4 + q] += (kd & 7) == q;
  }
#pragma unroll
  for (int k = 0; k < BM_NSTAT; ++k) sh[k][threadIdx.x] = s[k];
  for (int o = BM_THREADS / 2; o > 0; o >>= 1) {
    __syncthreads();
    if ((int)threadIdx.x < o) {
#pragma unroll
      for (int k = 0; k < BM_NSTAT; ++k) sh[k][threadIdx.x] += sh[k][threadIdx.x + o];
    }
  }
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < BM_NSTAT; ++k) stats[(size_t)blockIdx.x * BM_NSTAT + k] = sh[k][0];
  }
}

}  // namespace fotg
