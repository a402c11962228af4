// histograms.hip.h -- motion histograms: a flow turned into features, the histogram of optical flow (HOF) and the two motion-boundary
// histograms (MBHx, MBHy) of the dense-trajectories family, per cell of a regular grid and/or per object of an `ids` map.  Integer
// arithmetic after the first step, so any order of accumulation gives the same bytes.  The definition, in order:
//
// 1. Residual.  (u, v) = F[y][x] must be motion_known (motion_model.hip.h: |u|, |v| <= 4096, false for a NaN or an infinity).  With params
//    (n x 6 f64, the pixel-frame parameters of fotg_fit_motion): (pu, pv) = motion_predict(motion_coef(P, w, h), 2x-(w-1), 2y-(h-1)),
//    ru = u - pu, rv = v - pv (one f32 subtraction each), and (ru, rv) must be motion_known again.  Without params ru = u, rv = v.
// 2. A pixel is admissible iff step 1 passes and (no mask || mask[y][x] == 0).  U = (int)rintf(256 ru), V = (int)rintf(256 rv).
// 3. M(a, b) = floor(sqrt(a a + b b)), the exact integer square root of the 64-bit sum.
// 4. A(a, b) in [0, 2048), in units of 45/256 degrees, for (a, b) != (0, 0): ax = |a|, ay = |b|;
//      phi = ax >= ay ? T[(ay << 8) / ax] : 512 - T[(ax << 8) / ay]                       (integer division; T = MH_ATAN below)
//      a >= 0, b >= 0: A = phi;  a < 0, b >= 0: A = 1024 - phi;  a < 0, b < 0: A = 1024 + phi;  a >= 0, b < 0: A = (2048 - phi) mod 2048
//    T[k] = rint(256 atan(k / 256) / (pi / 4)), k = 0 .. 256: monotone, T[0] = 0, T[128] = 151, T[256] = 256; the entry nearest to a
//    rounding tie is 0.0077 away from it, so every libm gives this table.
// 5. Soft binning of a weight m at angle A: b0 = A >> 8, f = A & 255, w1 = (m f) >> 8, w0 = m - w1; bin b0 += w0, bin (b0 + 1) & 7 += w1.
//    Eight bins centred on the multiples of 45 degrees, linear interpolation between neighbours.
// 6. HOF of an admissible pixel, m = M(U, V): m < thresh256 counts one in the zero-bin column; otherwise m is soft-binned at A(U, V)
//    (nothing for U = V = 0, which can only get here with thresh256 = 0).
// 7. MBH.  Ux = U[y][min(x+1, w-1)] - U[y][max(x-1, 0)], Uy = U[min(y+1, h-1)][x] - U[max(y-1, 0)][x]; Vx, Vy alike (clamped
//    coordinates: one-sided at the border).  A pixel takes part iff it and its four clamped neighbours are admissible.  MBHx soft-bins
//    M(Ux, Uy) at A(Ux, Uy), MBHy M(Vx, Vy) at A(Vx, Vy); a zero gradient counts in n_mbh and adds nothing.
// 8. The record, 32 int64: [0..7] HOF, [8] zero-bin pixels, [9..16] MBHx, [17..24] MBHy, [25] admissible pixels, [26] pixels in MBH,
//    [27] pixels that are not admissible, [28] sum of m, [29] sum of U, [30] sum of V over the admissible pixels, [31] 0.
// 9. cells: n x ceil(h / cell) x ceil(w / cell) x 32, cell in {8, 16, 32}, edge cells partial.  objects: n x rows x 32; a pixel with
//    i = ids[y][x] in [0, rows) adds to row i, every other id is background; its MBH goes to its own row whatever its neighbours' ids.
// tests/histograms_ref.py restates all of this in numpy.
//
// mh_kernel<Src>: grid (ceil(w / 64), ceil(h / 32), n), 256 threads; a workgroup owns a tile of 64 x 32 pixels, which holds whole
// cells of every allowed size, so every cell belongs to one workgroup and is written by plain stores, once.
//   Staging: thread (tx, ty) = (t % 8, t / 8) owns the eight adjacent pixels 8 tx .. 8 tx + 7 of tile row ty: a dense flow leaves in
//   four 16-byte loads, the mask in two 4-byte and the ids in two 16-byte loads where the address allows, one by one otherwise; the
//   fused source evaluates its four taps per pixel.  196 threads add the one-pixel halo.  Every position holds the value of the pixel
//   at its clamped coordinates, as (U, V) or (MH_BAD, 0) for an inadmissible one: this is the only place flow, mask and params are read.
//   Histograms: lane l of wave k owns the eight vertically adjacent pixels (l, 8 k .. 8 k + 7) -- one cell, adjacent lanes read
//   adjacent LDS words -- and keeps the 31 columns as 32-bit counters: the seven counts and sums in registers, the 24 bins, whose
//   index is known at run time only, in a column of LDS that is the thread's alone (two integer adds per soft-binned weight, no
//   conflicts: the bank is the thread's, whatever the bin), read back into registers when the pixels are done; nothing is private
//   memory.  A cell of 32 x 32 fits 32 bits (MBH: 1024 floor(sqrt(2) 2^21) ~ 3.04e9); the sums of U and V fit a signed 32 bits.
//   Cells: the eight lanes of an 8 x 8 block add their registers with three DPP stages; one lane per block adds the non-zero columns to
//   the tile's table in LDS; after a barrier the table leaves as int64.
//   Objects: the wave walks the distinct ids of its 512 pixels (readlane of a live id, as objtracks.hip.h walks its keys); the lanes'
//   partials of one id are added over the whole wave (DPP inside rows of 16, two xor shuffles across) while they still fit 32 bits
//   (512 pixels), one lane adds the non-zero columns to a 64-bit table of MH_SLOTS objects in LDS, and after the barrier one thread per
//   slot and column issues one 64-bit integer atomic: a tile of one object costs at most 31 atomics for 2048 pixels.  (A ninth
//   object in a tile sends its wave partials straight to memory.)
#pragma once
#include <type_traits>
#include "common.h"
#include "flowsrc.hip.h"
#include "motion_model.hip.h"

namespace fotg {

enum { MH_THREADS = 256, MH_TW = 64, MH_TH = 32, MH_PW = MH_TW + 2, MH_PH = MH_TH + 2, MH_NREC = 32, MH_NACC = 31, MH_SLOTS = 8,
       MH_MAX_ROWS = 1024, MH_MAX_DIM = 16384, MH_HALO = 2 * MH_PW + 2 * MH_TH, MH_BAD = -2147483647 - 1 };
enum { MH_HOF = 0, MH_ZERO = 8, MH_MBHX = 9, MH_MBHY = 17, MH_N = 25, MH_NMBH = 26, MH_NBAD = 27, MH_SM = 28, MH_SU = 29, MH_SV = 30 };

// T[k] = rint(256 atan(k / 256) / (pi / 4))
__device__ const unsigned short MH_ATAN[257] = {
    0,   1,   3,   4,   5,   6,   8,   9,  10,  11,  13,  14,  15,  17,  18,  19,  20,  22,  23,  24,
   25,  27,  28,  29,  30,  32,  33,  34,  36,  37,  38,  39,  41,  42,  43,  44,  46,  47,  48,  49,
   51,  52,  53,  54,  55,  57,  58,  59,  60,  62,  63,  64,  65,  67,  68,  69,  70,  71,  73,  74,
   75,  76,  77,  79,  80,  81,  82,  83,  85,  86,  87,  88,  89,  91,  92,  93,  94,  95,  96,  98,
   99, 100, 101, 102, 103, 104, 106, 107, 108, 109, 110, 111, 112, 114, 115, 116, 117, 118, 119, 120,
  121, 122, 124, 125, 126, 127, 128, 129, 130, 131, 132, 133, 134, 135, 137, 138, 139, 140, 141, 142,
  143, 144, 145, 146, 147, 148, 149, 150, 151, 152, 153, 154, 155, 156, 157, 158, 159, 160, 161, 162,
  163, 164, 165, 166, 167, 168, 169, 170, 171, 172, 173, 174, 175, 176, 177, 177, 178, 179, 180, 181,
  182, 183, 184, 185, 186, 187, 188, 188, 189, 190, 191, 192, 193, 194, 195, 195, 196, 197, 198, 199,
  200, 201, 201, 202, 203, 204, 205, 206, 206, 207, 208, 209, 210, 211, 211, 212, 213, 214, 215, 215,
  216, 217, 218, 219, 219, 220, 221, 222, 222, 223, 224, 225, 225, 226, 227, 228, 228, 229, 230, 231,
  231, 232, 233, 234, 234, 235, 236, 236, 237, 238, 239, 239, 240, 241, 241, 242, 243, 243, 244, 245,
  245, 246, 247, 248, 248, 249, 250, 250, 251, 251, 252, 253, 253, 254, 255, 255, 256,
};

// floor(sqrt(a a + b b)) for |a|, |b| <= 2^22: the f32 root is an estimate, the exact integer products decide.  Vectors below 128
// pixels (a, b < 2^15: the sum fits 32 bits, every product is a 24-bit one) take the short path.
__device__ __forceinline__ unsigned mh_mag(int a, int b)
{
  const unsigned ax = (unsigned)(a < 0 ? -a : a), ay = (unsigned)(b < 0 ? -b : b);
  if ((ax | ay) < 32768u) {
    const unsigned n = __umul24(ax, ax) + __umul24(ay, ay);
    // n < 2^31: the conversion (2^-24) and the root (one ulp) are off by less than 0.01 in all, so the truncated estimate is the
    // root or one beside it, and one step either way settles it
    unsigned s = (unsigned)__builtin_amdgcn_sqrtf((float)n);
    s -= __umul24(s, s) > n ? 1u : 0u;
    s += __umul24(s + 1, s + 1) <= n ? 1u : 0u;
    return s;
  }
  const unsigned long long n = (unsigned long long)ax * ax + (unsigned long long)ay * ay;
  unsigned s = (unsigned)sqrtf((float)n);
  while ((unsigned long long)s * s > n) --s;
  while ((unsigned long long)(s + 1) * (s + 1) <= n) ++s;
  return s;
}

// step 4 for (a, b) != (0, 0); tab: the table (in LDS)
__device__ __forceinline__ unsigned mh_angle(int a, int b, const unsigned short *tab)
{
  const unsigned ax = (unsigned)(a < 0 ? -a : a), ay = (unsigned)(b < 0 ? -b : b);
  const unsigned lo = ax >= ay ? ay : ax, hi = ax >= ay ? ax : ay;
  // (lo << 8) / hi, at most 256, hi < 2^23: the f32 quotient is within one of it, the exact 24-bit product decides
  const unsigned num = lo << 8;
  unsigned q = (unsigned)((float)num * __builtin_amdgcn_rcpf((float)hi));
  const int r = (int)(num - __umul24(q, hi));
  q = r < 0 ? q - 1 : ((unsigned)r >= hi ? q + 1 : q);
  const unsigned t = tab[q];
  const unsigned phi = ax >= ay ? t : 512u - t;
  return a >= 0 ? (b >= 0 ? phi : (2048u - phi) & 2047u) : (b >= 0 ? 1024u - phi : 1024u + phi);
}

// step 5 into the lane's eight bins in LDS (bin k at col[k MH_THREADS]): a run-time bin is an LDS address, never a register index
__device__ __forceinline__ void mh_soft(unsigned *col, unsigned m, int a, int b, const unsigned short *tab)
{
  if (m == 0) return;
  const unsigned A = mh_angle(a, b, tab);
  const unsigned b0 = A >> 8, b1 = (b0 + 1) & 7, w1 = (m * (A & 255u)) >> 8, w0 = m - w1;
  atomicAdd(col + b0 * MH_THREADS, w0);
  if (w1 != 0) atomicAdd(col + b1 * MH_THREADS, w1);
}

// steps 1 and 2 for the pixel (cx, cy): (U, V), or (MH_BAD, 0) for an inadmissible one
__device__ __forceinline__ int2 mh_fixed(float u, float v, unsigned mk, bool has, const MotionCoef &m, int cx, int cy, int w, int h)
{
  bool ok = mk == 0 && motion_known(u, v);
  float ru = u, rv = v;
  if (has) {
    float pu, pv;
    motion_predict(m, 2 * cx - (w - 1), 2 * cy - (h - 1), pu, pv);
    ru = u - pu; rv = v - pv;
    ok = ok && motion_known(ru, rv);
  }
  int2 r;
  r.x = ok ? (int)rintf(ru * 256.f) : (int)MH_BAD;
  r.y = ok ? (int)rintf(rv * 256.f) : 0;
  return r;
}

// one stage of a reduction over lanes: every column gets the value of the lane the DPP control CTRL pairs its lane with
template <int CTRL>
__device__ __forceinline__ void mh_dpp_stage(unsigned (&s)[MH_NACC])
{
  unsigned t[MH_NACC];
#pragma unroll
  for (int k = 0; k < MH_NACC; ++k) t[k] = (unsigned)__builtin_amdgcn_update_dpp(0, (int)s[k], CTRL, 0xf, 0xf, false);
#pragma unroll
  for (int k = 0; k < MH_NACC; ++k) s[k] += t[k];
}

// the sums of U and V are signed
__device__ __forceinline__ unsigned long long mh_wide(unsigned v, int col)
{
  return (col == MH_SU || col == MH_SV) ? (unsigned long long)(long long)(int)v : (unsigned long long)v;
}

// flow: the vectors; mask: n x h x w bytes or null; params: n x 6 or null; ids: n x h x w or null (then objects is null);
// cells: n x ceil(h / cell) x ceil(w / cell) x 32 or null; objects: n x rows x 32 or null, cleared before the launch.
// vec: bit 0 a dense flow is aligned for 16-byte loads, bit 1 the mask for 4-byte loads, bit 2 the ids for 16-byte loads.
template <class Src>
__global__ __launch_bounds__(MH_THREADS) void mh_kernel(Src flow, const unsigned char *__restrict__ mask, const double *__restrict__ params,
                                                        const int *__restrict__ ids, int w, int h, int cell, int thresh, int rows, int vec,
                                                        long long *__restrict__ cells, long long *__restrict__ objects)
{
  __shared__ int2 suv[MH_PH][MH_PW];                          // position (lx, ly): the pixel (X0 + lx - 1, Y0 + ly - 1), clamped
  __shared__ short sid[MH_TH][MH_TW];                         // the pixel's row of objects (below 1024), -1 for background
  __shared__ unsigned ctab[32][MH_NREC];                      // the tile's cells (32 of them at cell 8)
  __shared__ unsigned long long otab[MH_SLOTS][MH_NREC];      // the tile's objects
  __shared__ int okey[MH_SLOTS];
  __shared__ unsigned short tab[257];
  __shared__ unsigned lbin[3 * 8][MH_THREADS];                // the lane's HOF, MBHx and MBHy bins of the turn: column t is thread t's alone
  const int t = threadIdx.x, pair = blockIdx.z;
  const int X0 = (int)blockIdx.x * MH_TW, Y0 = (int)blockIdx.y * MH_TH;
  const size_t img = (size_t)pair * w * h;
  const bool has = params != nullptr, obj = objects != nullptr;
  MotionCoef mc = {};
  if (has) mc = motion_coef(params + 6 * (size_t)pair, w, h);

  for (int i = t; i < 32 * MH_NREC; i += MH_THREADS) (&ctab[0][0])[i] = 0;
  (&otab[0][0])[t] = 0;                                      // MH_SLOTS * MH_NREC == MH_THREADS
  if (t < MH_SLOTS) okey[t] = -1;
  for (int i = t; i < 257; i += MH_THREADS) tab[i] = MH_ATAN[i];
#pragma unroll
  for (int k = 0; k < 3 * 8; ++k) lbin[k][t] = 0;

  {                                                          // the interior: eight adjacent pixels of one row
    const int tx = t % 8, ty = t / 8, gx0 = X0 + 8 * tx, gy = Y0 + ty;
    if (gy <= h && gx0 <= w) {                               // (row h and column w are read as clamped neighbours)
      const int cy = gy < h ? gy : h - 1;
      const size_t row = img + (size_t)cy * w;
      const bool whole = gx0 + 8 <= w;
      float u[8], v[8];
      bool got = false;
      if constexpr (std::is_same<Src, DenseSrc>::value) {
        if (whole && (vec & 1) && ((row + gx0) & 1) == 0) {
          const float4 *f = reinterpret_cast<const float4 *>(flow.flow + 2 * (row + gx0));
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const float4 f4 = f[q];
            u[2 * q] = f4.x; v[2 * q] = f4.y; u[2 * q + 1] = f4.z; v[2 * q + 1] = f4.w;
          }
          got = true;
        }
      }
      if (!got) {
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const int cx = gx0 + q < w ? gx0 + q : w - 1;
          flow.at((long)(row + cx), pair, cx, cy, u[q], v[q]);
        }
      }
      const bool quad = whole && ((row + gx0) & 3) == 0;
      unsigned mk[2] = {0, 0};
      if (mask) {
        if (quad && (vec & 2)) {
          mk[0] = *reinterpret_cast<const unsigned *>(mask + row + gx0);
          mk[1] = *reinterpret_cast<const unsigned *>(mask + row + gx0 + 4);
        } else {
#pragma unroll
          for (int q = 0; q < 8; ++q) {
            const int cx = gx0 + q < w ? gx0 + q : w - 1;
            mk[q / 4] |= (unsigned)mask[row + cx] << (8 * (q % 4));
          }
        }
      }
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int cx = gx0 + q < w ? gx0 + q : w - 1;
        suv[ty + 1][8 * tx + q + 1] = mh_fixed(u[q], v[q], (mk[q / 4] >> (8 * (q % 4))) & 0xffu, has, mc, cx, cy, w, h);
      }
      if (obj && gy < h) {
        int id[8];
        if (quad && (vec & 4)) {
          const int4 a = *reinterpret_cast<const int4 *>(ids + row + gx0), b = *reinterpret_cast<const int4 *>(ids + row + gx0 + 4);
          id[0] = a.x; id[1] = a.y; id[2] = a.z; id[3] = a.w; id[4] = b.x; id[5] = b.y; id[6] = b.z; id[7] = b.w;
        } else {
#pragma unroll
          for (int q = 0; q < 8; ++q) id[q] = gx0 + q < w ? ids[row + gx0 + q] : -1;
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) sid[ty][8 * tx + q] = (unsigned)id[q] < (unsigned)rows ? (short)id[q] : (short)-1;
      }
    }
  }
  if (t < MH_HALO) {                                         // the halo: top row, bottom row, left column, right column
    int lx, ly;
    if (t < MH_PW) { lx = t; ly = 0; }
    else if (t < 2 * MH_PW) { lx = t - MH_PW; ly = MH_PH - 1; }
    else if (t < 2 * MH_PW + MH_TH) { lx = 0; ly = t - 2 * MH_PW + 1; }
    else { lx = MH_PW - 1; ly = t - 2 * MH_PW - MH_TH + 1; }
    const int gx = X0 + lx - 1, gy = Y0 + ly - 1;
    if (gx <= w && gy <= h) {
      const int cx = gx < 0 ? 0 : gx < w ? gx : w - 1, cy = gy < 0 ? 0 : gy < h ? gy : h - 1;
      const size_t p = img + (size_t)cy * w + cx;
      float u, v;
      flow.at((long)p, pair, cx, cy, u, v);
      suv[ly][lx] = mh_fixed(u, v, mask ? (unsigned)mask[p] : 0u, has, mc, cx, cy, w, h);
    }
  }
  __syncthreads();

  const int lane = t % FOTG_WAVE, ly0 = (t / FOTG_WAVE) * 8;  // the lane's pixels: tile column `lane`, tile rows ly0 .. ly0 + 7
  unsigned live = 0;                                         // bit q: pixel q is inside the image and not yet counted
  if (X0 + lane < w) {
    const int left = h - (Y0 + ly0);
    live = left >= 8 ? 0xffu : left > 0 ? (1u << left) - 1u : 0u;
  }
  unsigned ca[MH_NACC];                                      // the lane's part of its cell
#pragma unroll
  for (int k = 0; k < MH_NACC; ++k) ca[k] = 0;
  for (;;) {                                                 // one turn per distinct id of the wave (one turn without objects)
    const unsigned long long any = __ballot(live != 0);
    if (any == 0) break;
    int key = -1;
    if (obj) {
      const int mine = live ? sid[ly0 + __ffs((int)live) - 1][lane] : -1;
      key = __builtin_amdgcn_readlane(mine, __builtin_amdgcn_readfirstlane(__ffsll((long long)any) - 1));
    }
    const bool need = cells != nullptr || key >= 0;          // wave-uniform: background pixels matter to the cells only
    unsigned a[MH_NACC];
#pragma unroll
    for (int k = 0; k < MH_NACC; ++k) a[k] = 0;
#pragma unroll 1
    for (int q = 0; q < 8; ++q) {
      if (!((live >> q) & 1)) continue;
      if (obj && sid[ly0 + q][lane] != key) continue;
      live &= ~(1u << q);
      if (!need) continue;
      const int2 c = suv[ly0 + q + 1][lane + 1];
      if (c.x == MH_BAD) { a[MH_NBAD] += 1; continue; }
      const unsigned m = mh_mag(c.x, c.y);
      a[MH_N] += 1; a[MH_SM] += m; a[MH_SU] += (unsigned)c.x; a[MH_SV] += (unsigned)c.y;
      if (m < (unsigned)thresh) a[MH_ZERO] += 1;
      else mh_soft(&lbin[0][t], m, c.x, c.y, tab);
      const int2 l = suv[ly0 + q + 1][lane], r = suv[ly0 + q + 1][lane + 2], up = suv[ly0 + q][lane + 1], dn = suv[ly0 + q + 2][lane + 1];
      if (l.x == MH_BAD || r.x == MH_BAD || up.x == MH_BAD || dn.x == MH_BAD) continue;
      a[MH_NMBH] += 1;
      const int ux = r.x - l.x, uy = dn.x - up.x, vx = r.y - l.y, vy = dn.y - up.y;
      mh_soft(&lbin[8][t], mh_mag(ux, uy), ux, uy, tab);
      mh_soft(&lbin[16][t], mh_mag(vx, vy), vx, vy, tab);
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {                            // the turn's bins come back to registers, and are cleared for the next
      a[MH_HOF + k] = lbin[k][t]; a[MH_MBHX + k] = lbin[8 + k][t]; a[MH_MBHY + k] = lbin[16 + k][t];
      lbin[k][t] = 0; lbin[8 + k][t] = 0; lbin[16 + k][t] = 0;
    }
    if (cells) {
#pragma unroll
      for (int k = 0; k < MH_NACC; ++k) ca[k] += a[k];
    }
    if (key >= 0) {                                          // the wave's 512 pixels fit 32 bits; beyond the wave it is 64
      mh_dpp_stage<0xB1>(a);                                 // quad_perm [1 0 3 2]
      mh_dpp_stage<0x4E>(a);                                 // quad_perm [2 3 0 1]
      mh_dpp_stage<0x141>(a);                                // row_half_mirror
      mh_dpp_stage<0x140>(a);                                // row_mirror
#pragma unroll
      for (int o = 16; o <= 32; o <<= 1) {
        unsigned s[MH_NACC];
#pragma unroll
        for (int k = 0; k < MH_NACC; ++k) s[k] = (unsigned)__shfl_xor((int)a[k], o, FOTG_WAVE);
#pragma unroll
        for (int k = 0; k < MH_NACC; ++k) a[k] += s[k];
      }
      if (lane == 0) {
        int slot = -1;
        for (int p = 0; p < MH_SLOTS && slot < 0; ++p) {
          const int s = (key + p) % MH_SLOTS;
          const int old = atomicCAS(&okey[s], -1, key);
          if (old == -1 || old == key) slot = s;
        }
        unsigned long long *out = reinterpret_cast<unsigned long long *>(objects) + ((size_t)pair * rows + key) * MH_NREC;
#pragma unroll
        for (int k = 0; k < MH_NACC; ++k) {
          if (a[k] == 0) continue;
          if (slot >= 0) atomicAdd(&otab[slot][k], mh_wide(a[k], k));
          else atomicAdd(out + k, mh_wide(a[k], k));
        }
      }
    }
  }
  if (cells) {                                               // the eight lanes of an 8 x 8 block, then one lane per block
    mh_dpp_stage<0xB1>(ca);
    mh_dpp_stage<0x4E>(ca);
    mh_dpp_stage<0x141>(ca);
    if (lane % 8 == 0) {
      unsigned *dst = ctab[(ly0 / cell) * (MH_TW / cell) + lane / cell];
#pragma unroll
      for (int k = 0; k < MH_NACC; ++k)
        if (ca[k] != 0) atomicAdd(dst + k, ca[k]);
    }
  }
  __syncthreads();
  if (obj) {
    const int slot = t / MH_NREC, col = t % MH_NREC, key = okey[slot];
    const unsigned long long v = otab[slot][col];
    if (key >= 0 && v != 0)
      atomicAdd(reinterpret_cast<unsigned long long *>(objects) + ((size_t)pair * rows + key) * MH_NREC + col, v);
  }
  if (cells) {
    const int cpr = MH_TW / cell, cpc = MH_TH / cell, gw = (w + cell - 1) / cell, gh = (h + cell - 1) / cell;
    for (int i = t; i < cpr * cpc * MH_NREC; i += MH_THREADS) {
      const int c = i / MH_NREC, col = i % MH_NREC;
      const int ccx = X0 / cell + c % cpr, ccy = Y0 / cell + c / cpr;
      if (ccx < gw && ccy < gh)
        cells[(((size_t)pair * gh + ccy) * gw + ccx) * MH_NREC + col] = (long long)mh_wide(ctab[c][col], col);
    }
  }
}

}  // namespace fotg
