// flowcolor.hip.h -- Middlebury flow colour code (flow_code/C/color_flow.cpp MotionToColor + colorcode.cpp computeColor) on the GPU.
//
// Two passes per batch, one launch each for all pairs:
//   range pass   per image, over every KNOWN vector (flowIO.cpp unknown_flow: |u| > 1e9 || |v| > 1e9 || isnan): max sqrtf(u^2 + v^2),
//                min/max u, min/max v.  Wave, then workgroup reduction, one atomicMax per workgroup and statistic on ordered-integer
//                keys (order-independent, so deterministic); key 0 = "no vector seen", the reference's initial values are applied
//                when the keys are read (maxrad -1, max* -999, min* 999).
//   colour pass  computeColor(u / maxrad, v / maxrad) per pixel, maxrad per image (maxmotion > 0 overrides it, 0 becomes 1),
//                unknown vectors black; 3 bytes per pixel in R, G, B order, four pixels (3 dwords) per thread over the linear
//                pixel index of the whole batch, so every store is a full aligned dword.
// Inputs: a dense n x h x w x 2 flow (DenseSrc) or the engine's coarse flow, upsampled and cropped on the fly with the
// arithmetic of upsample_crop4_kernel (UpsampleSrc: same source coordinate, same x 2^sc_l per tap, same three lerps in the
// same order) -- the full-resolution flow is never written.
//
// Numerics: the reference's float/double mix is restated operation by operation (f32 sqrt and
// division, double where the reference's expression is double, f32 lerps); the angle is the correctly rounded f32 of the true
// atan2, computed as (float)atan2((double)y, (double)x) -- the reference calls glibc atan2f, which no GPU can match bit for bit.
#pragma once
#include "common.h"
#include "flowsrc.hip.h"

namespace fotg {

// colorcode.cpp makecolorwheel(): RY 15, YG 6, GC 4, CB 11, BM 13, MR 6 -> 55 entries, packed r | g << 8 | b << 16
__constant__ unsigned c_colorwheel[55] = {
    0x0000ff, 0x0011ff, 0x0022ff, 0x0033ff, 0x0044ff, 0x0055ff, 0x0066ff, 0x0077ff, 0x0088ff, 0x0099ff, 0x00aaff, 0x00bbff,
    0x00ccff, 0x00ddff, 0x00eeff, 0x00ffff, 0x00ffd5, 0x00ffaa, 0x00ff80, 0x00ff55, 0x00ff2b, 0x00ff00, 0x3fff00, 0x7fff00,
    0xbfff00, 0xffff00, 0xffe800, 0xffd100, 0xffba00, 0xffa300, 0xff8c00, 0xff7400, 0xff5d00, 0xff4600, 0xff2f00, 0xff1800,
    0xff0000, 0xff0013, 0xff0027, 0xff003a, 0xff004e, 0xff0062, 0xff0075, 0xff0089, 0xff009c, 0xff00b0, 0xff00c4, 0xff00d7,
    0xff00eb, 0xff00ff, 0xd500ff, 0xaa00ff, 0x8000ff, 0x5500ff, 0x2b00ff};

enum { FC_NSTAT = 5 };   // per image: maxrad, minu, maxu, minv, maxv (the order of the C-ABI's stats)

// ordered-integer key of a float: a < b  <=>  key(a) < key(b) (unsigned) for every non-NaN float; key >= 0x007fffff, so 0 is below all
__host__ __device__ inline unsigned fc_key(float f)
{
  const unsigned u = __builtin_bit_cast(unsigned, f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ inline float fc_unkey(unsigned k)
{
  return __builtin_bit_cast(float, (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

__device__ __forceinline__ bool fc_unknown(float u, float v)
{
  return fabsf(u) > 1e9f || fabsf(v) > 1e9f || __builtin_isnan(u) || __builtin_isnan(v);   // 1e9 is exact in f32
}

__device__ __forceinline__ unsigned fc_wave_max(unsigned v)
{
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const unsigned t = __shfl_xor(v, o, 64); v = t > v ? t : v; }
  return v;
}

// Range pass: grid = per_img * n workgroups of 256, workgroup b covers image b / per_img.  keys: n x 5, zeroed before the launch;
// key slots (all atomicMax): key(maxrad), ~key(minu), key(maxu), ~key(minv), key(maxv).
template <class Src>
__global__ __launch_bounds__(256) void flow_range_kernel(Src src, int w, int h, int per_img, unsigned *__restrict__ keys)
{
  const int pair = blockIdx.x / per_img, part = blockIdx.x % per_img;
  const long hw = (long)w * h;
  unsigned k[FC_NSTAT] = {0, 0, 0, 0, 0};
  for (long r = (long)part * blockDim.x + threadIdx.x; r < hw; r += (long)per_img * blockDim.x) {
    const int y = (int)(r / w), x = (int)(r - (long)y * w);
    float u, v;
    src.at((long)pair * hw + r, pair, x, y, u, v);
    if (fc_unknown(u, v)) continue;
    const float rad = sqrtf(u * u + v * v);
    const unsigned ku = fc_key(u), kv = fc_key(v), kr = fc_key(rad);
    k[0] = kr > k[0] ? kr : k[0];
    k[1] = ~ku > k[1] ? ~ku : k[1];
    k[2] = ku > k[2] ? ku : k[2];
    k[3] = ~kv > k[3] ? ~kv : k[3];
    k[4] = kv > k[4] ? kv : k[4];
  }
  __shared__ unsigned part_k[256 / FOTG_WAVE][FC_NSTAT];
  const int wave = threadIdx.x / FOTG_WAVE, lane = threadIdx.x % FOTG_WAVE;
#pragma unroll
  for (int s = 0; s < FC_NSTAT; ++s) {
    const unsigned m = fc_wave_max(k[s]);
    if (lane == 0) part_k[wave][s] = m;
  }
  __syncthreads();
  if (threadIdx.x < FC_NSTAT) {
    unsigned m = 0;
    for (int i = 0; i < (int)(blockDim.x / FOTG_WAVE); ++i) m = part_k[i][threadIdx.x] > m ? part_k[i][threadIdx.x] : m;
    if (m != 0) atomicMax(keys + (size_t)pair * FC_NSTAT + threadIdx.x, m);
  }
}

// the statistics color_flow prints, from the keys: the reference's initial values where no known vector was seen (or where every
// vector lies beyond them: __max(-999, u) keeps -999 when all u < -999)
__device__ __forceinline__ void fc_stats(const unsigned *k, float *s)
{
  s[0] = k[0] ? fc_unkey(k[0]) : -1.f;
  const float minu = k[1] ? fc_unkey(~k[1]) : 999.f, maxu = k[2] ? fc_unkey(k[2]) : -999.f;
  const float minv = k[3] ? fc_unkey(~k[3]) : 999.f, maxv = k[4] ? fc_unkey(k[4]) : -999.f;
  s[1] = minu < 999.f ? minu : 999.f;
  s[2] = maxu > -999.f ? maxu : -999.f;
  s[3] = minv < 999.f ? minv : 999.f;
  s[4] = maxv > -999.f ? maxv : -999.f;
}

// colorcode.cpp computeColor(fx, fy), restated: returns r | g << 8 | b << 16.  wf: the wheel as floats, wf[3 k + b] =
// (float)(colorwheel[k][b] / 255.0), b = 0 red.
__device__ __forceinline__ unsigned fc_color(float fx, float fy, const float *wf)
{
  const float rad = sqrtf(fx * fx + fy * fy);
  const float ang = (float)atan2((double)-fy, (double)-fx);          // correctly rounded f32 of atan2(-fy, -fx) (D6)
  const float a = (float)((double)ang / M_PI);
  const float fk = (float)(((double)a + 1.0) / 2.0 * 54.0);          // (a + 1.0) / 2.0 * (ncols - 1)
  const int k0 = (int)fk;
  const int k1 = k0 + 1 == 55 ? 0 : k0 + 1;
  const float f = fk - (float)k0;
  unsigned out = 0;
#pragma unroll
  for (int b = 0; b < 3; ++b) {
    const float col0 = wf[3 * k0 + b], col1 = wf[3 * k1 + b];
    float col = (1 - f) * col0 + f * col1;
    if (rad <= 1)
      col = 1 - rad * (1 - col);
    else
      col = col * 0.75f;                       // (double)col * .75 is exact, so its f32 rounding is the f32 product
    out |= (unsigned)(int)(255.0 * (double)col) << (8 * b);
  }
  return out;
}

// Colour pass: thread q writes pixels 4q .. 4q+3 of the batch (linear index over n x h x w) = bytes 12q .. 12q+11 of rgb.
template <class Src>
__global__ __launch_bounds__(256) void flow_color_kernel(Src src, int w, int h, long npix, const unsigned *__restrict__ keys,
                                                         float maxmotion, unsigned char *__restrict__ rgb)
{
  __shared__ float wf[55 * 3];
  if (threadIdx.x < 55 * 3)
    wf[threadIdx.x] = (float)((double)((c_colorwheel[threadIdx.x / 3] >> (8 * (threadIdx.x % 3))) & 0xff) / 255.0);
  __syncthreads();
  const long q = (long)blockIdx.x * blockDim.x + threadIdx.x, p0 = 4 * q;
  if (p0 >= npix) return;
  const long hw = (long)w * h;
  int pair = (int)(p0 / hw);
  const long r = p0 - (long)pair * hw;
  int y = (int)(r / w), x = (int)(r - (long)y * w);
  unsigned px[4] = {0, 0, 0, 0};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (p0 + i < npix) {
      float u, v;
      src.at(p0 + i, pair, x, y, u, v);
      if (!fc_unknown(u, v)) {
        // color_flow.cpp:48-52 with the per-image maxrad of the range pass (a known vector here means the image has one: k != 0)
        const unsigned kr = keys[(size_t)pair * FC_NSTAT];
        float maxrad = fc_unkey(kr);
        if (maxmotion > 0) maxrad = maxmotion;
        if (maxrad == 0) maxrad = 1;
        px[i] = fc_color(u / maxrad, v / maxrad, wf);
      }
      if (++x == w) { x = 0; if (++y == h) { y = 0; ++pair; } }
    }
  }
  // 4 x 3 bytes -> 3 dwords, little endian: pixel i at bytes 3i .. 3i+2
  const unsigned d0 = px[0] | px[1] << 24, d1 = px[1] >> 8 | px[2] << 16, d2 = px[2] >> 16 | px[3] << 8;
  unsigned char *o = rgb + 12 * q;
  if (p0 + 4 <= npix && (((size_t)rgb) & 3) == 0) {
    unsigned *od = reinterpret_cast<unsigned *>(o);
    __builtin_nontemporal_store(d0, od);
    __builtin_nontemporal_store(d1, od + 1);
    __builtin_nontemporal_store(d2, od + 2);
  } else {
    const unsigned d[3] = {d0, d1, d2};
    const int nb = (int)(npix - p0 < 4 ? npix - p0 : 4) * 3;
#pragma unroll
    for (int i = 0; i < 12; ++i)                 // (unrolled: constant indices into d, no private array)
      if (i < nb) o[i] = (unsigned char)(d[i >> 2] >> (8 * (i & 3)));
  }
}

// keys -> the five statistics, in place (stats doubles as the key buffer when the caller asked for it)
__global__ __launch_bounds__(256) void flow_stats_kernel(int n, unsigned *keys)
{
  const int pair = blockIdx.x * blockDim.x + threadIdx.x;
  if (pair >= n) return;
  unsigned k[FC_NSTAT];
  float s[FC_NSTAT];
  for (int i = 0; i < FC_NSTAT; ++i) k[i] = keys[(size_t)pair * FC_NSTAT + i];
  fc_stats(k, s);
  for (int i = 0; i < FC_NSTAT; ++i) keys[(size_t)pair * FC_NSTAT + i] = __builtin_bit_cast(unsigned, s[i]);
}

}  // namespace fotg
