// components.hip.h -- connected components of a uint8 code map with a record per component: what turns the per-pixel codes of the
// motion fit (1 = independent motion), of the consistency check or of the warp into a list of objects.  The definition, in order:
//
// Input: code, n x h x w uint8, 1 <= w, h <= 16384 (COMP_MAX_DIM); fg_codes, an 8-bit set with at least one bit: pixel p is
//   foreground iff code[p] < 8 && ((fg_codes >> code[p]) & 1); connectivity 4 or 8 (two foreground pixels are linked when they are
//   horizontal or vertical neighbours, at 8 also diagonal ones); a component is a class of the transitive closure of the links.
//   Components never join across the images of the batch.  values: null or n x h x w x 2 f32 (for moving objects: the fit's residual).
// Label: the linear index y w + x of the component's first pixel in raster order = the minimum linear index over its pixels.  It
//   does not depend on the tile shape, the launch shape, the order in which workgroups arrive or the route the merges took.
// Record, eleven int64, every one independent of the order of reduction:
//   label, area, xmin, ymin, xmax, ymax, sum x, sum y, n_val, sum U, sum V
//   U = (int)rintf(256 u), V = (int)rintf(256 v) of the pixel's vector (u, v) in `values`, the fixed point of the motion fit; a vector
//   is admissible iff |u| <= 4096 && |v| <= 4096 (false for a NaN or an infinity, and beyond +-4096 px); n_val counts the admissible
//   pixels of the component, sum U and sum V run over them; all three are 0 without `values`.
//   For w, h <= 16384 none can overflow: area <= 2^28, sum x and sum y < 2^28 x 2^14 = 2^42, |sum U|, |sum V| <= 2^28 x 2^20 = 2^48;
//   the per-pixel int32 area holds 2^28, and inside a tile of 1024 pixels the 32-bit partial sums stay below 1024 x 2^20 = 2^30.
// Selection and order: a component is kept iff area >= min_area (min_area >= 1).  The kept components, in ascending label order, are
//   the rows of objects (n x max_objects x 11, 1 <= max_objects <= 65536): at most the first max_objects of them are written, every
//   row after the written ones is zero.
// Outputs beside objects, each optional: labels int32 n x h x w, the component's label or -1 for background (components below
//   min_area keep theirs); ids int32 n x h x w, the row of the pixel's component in objects, or -1 (background, a component too
//   small, one beyond max_objects); stats int64 n x 4: foreground pixels, components, components with area >= min_area, rows written.
// tests/objects_ref.py restates all of this in numpy.
//
// Kernels: union-find over the pixels, parent[p] <= p always, the smaller root wins every union, so the root of a set is its
// minimum = the label.  Tiles are COMP_TW x COMP_TH = 64 x 16 pixels, one workgroup of 256 threads, a thread owns four consecutive
// pixels of a row.  Seven launches, everything between them crosses a kernel boundary:
//   comp_tile_kernel     the tile in LDS: runs inside a thread's four pixels point at their start, then unions (LDS atomicMin) along
//                        the links comp_links() keeps; writes per foreground pixel the global index of its tile-local root, -1 for
//                        background, and clears the area array
//   comp_merge_kernel    one thread per pixel of a tile's top row (links to the row above) or left column (links to the column
//                        to the left, the diagonals across the edge and the tile corners included at 8-connectivity):
//                        union(a, b) = find both roots, atomicMin the larger root's parent with the smaller, go on with the value the
//                        atomic returned until it returns the root itself.  Parent reads are relaxed agent-scope atomic loads: a
//                        stale one costs an iteration, never a wrong link (any value ever stored in parent[x] is a member of x's
//                        set that is <= x).  Nothing waits: every loop ends after finitely many steps of its own.
//   comp_flatten_kernel  per tile: label = root; the areas, grouped in LDS by tile-local root (what comp_tile_kernel left in the
//                        parents of the non-root pixels), one find and one 32-bit atomicAdd per group to area[root]; a non-root
//                        pixel keeps its group's LDS slot in its own (otherwise unused) area entry for comp_reduce_kernel.  The
//                        finds of other tiles may walk through parents this tile is replacing by their roots: those are relaxed
//                        agent-scope atomic stores of a smaller member of the same set, so a find that meets one only gets there sooner
//   comp_count_kernel    per 1024-pixel chunk of linear index: foreground pixels, roots, roots with area >= min_area
//   comp_scan_kernel     per image an exclusive scan over the chunk counts; rows written = min(total, max_objects)
//   comp_emit_kernel     per chunk: a kept root's row = offset + its rank in the chunk (raster order); writes label, area and the
//                        neutral elements of the box; area[root] becomes the row, or -1
//   comp_reduce_kernel   per tile: box, sum x, sum y, n_val, sum U, sum V per group in LDS (32 bits), per thread over its run of
//                        pixels first, a whole wave with one group reduced by lane crossings and added once; then one 64-bit
//                        integer atomic per group and statistic to the object's row; writes ids
// comp_links() drops links that others imply (with the left neighbour and the upper-left one set, the link upwards closes a
// square): an all-foreground tile makes one union per row, not one per pixel.  Tile kernels take the image index fastest in
// blockIdx.x, so the atomics of one image's large component are spread over the launch and not issued back to back.
// There are no floating-point atomics, no flags and no cooperative launch.
#pragma once
#include "common.h"

namespace fotg {

enum { COMP_TW = 64, COMP_TH = 16, COMP_TILE = COMP_TW * COMP_TH, COMP_THREADS = 256, COMP_CHUNK = 1024, COMP_NREC = 11, COMP_NSTAT = 4,
       COMP_MAX_DIM = 16384, COMP_MAX_OBJECTS = 65536 };
enum { COMP_LINK_U = 1, COMP_LINK_UL = 2, COMP_LINK_UR = 4 };

// which of the links of a foreground pixel to the row above are made, from the foreground flags of its left, upper-left, upper and
// upper-right neighbours (the link to the left always is).  A dropped link is implied: L and UL (4), L and U (8) reach U through the
// links of the pixel to the left; UL and UR hang on U; UL is the upper neighbour of L.
__host__ __device__ inline int comp_links(bool conn8, bool L, bool UL, bool U, bool UR)
{
  if (!conn8) return (U && !(L && UL)) ? COMP_LINK_U : 0;
  if (U) return L ? 0 : COMP_LINK_U;
  return ((UL && !L) ? COMP_LINK_UL : 0) | (UR ? COMP_LINK_UR : 0);
}

__host__ __device__ inline bool comp_known(float u, float v) { return fabsf(u) <= 4096.f && fabsf(v) <= 4096.f; }

template <int SCOPE>
__device__ __forceinline__ int comp_find(int *par, int x)
{
  for (;;) {
    const int q = __hip_atomic_load(par + x, __ATOMIC_RELAXED, SCOPE);
    if (q >= x || q < 0) return x;                      // (q == x: the root.  Nothing else but a smaller member is ever stored)
    x = q;                                              // q < x: ends
  }
}

template <int SCOPE>
__device__ __forceinline__ void comp_union(int *par, int a, int b)
{
  for (;;) {
    a = comp_find<SCOPE>(par, a);
    b = comp_find<SCOPE>(par, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = __hip_atomic_fetch_min(par + a, b, __ATOMIC_RELAXED, SCOPE);
    if (old == a) return;                               // a was a root and now hangs on b
    a = old;                                            // a hung on `old` already: old and b are still to be joined
  }
}

struct CompTile { int img, tx0, ty0; };

// blockIdx.x = tile n + image
__device__ __forceinline__ CompTile comp_tile(int n, int ntx)
{
  const int t = blockIdx.x / n;
  CompTile c;
  c.img = blockIdx.x - t * n;
  const int ty = t / ntx;
  c.tx0 = (t - ty * ntx) * COMP_TW;
  c.ty0 = ty * COMP_TH;
  return c;
}

__device__ __forceinline__ int comp_wave_sum(int v)
{
#pragma unroll
  for (int o = 1; o < FOTG_WAVE; o <<= 1) v += __shfl_xor(v, o, FOTG_WAVE);
  return v;
}
__device__ __forceinline__ int comp_wave_min(int v)
{
#pragma unroll
  for (int o = 1; o < FOTG_WAVE; o <<= 1) v = min(v, __shfl_xor(v, o, FOTG_WAVE));
  return v;
}
__device__ __forceinline__ int comp_wave_max(int v)
{
#pragma unroll
  for (int o = 1; o < FOTG_WAVE; o <<= 1) v = max(v, __shfl_xor(v, o, FOTG_WAVE));
  return v;
}

// s: the thread's one group (>= 0), none (-1) or several (-2).  The lane that adds for the whole wave when every thread of it
// with a group has the same one and none has several; -1 otherwise.  *s0: that group.
__device__ __forceinline__ int comp_wave_leader(int s, int *s0)
{
  const unsigned long long has = __ballot(s >= 0);
  if (__ballot(s == -2) != 0 || has == 0) return -1;
  const int lead = __ffsll((long long)has) - 1;
  *s0 = __shfl(s, lead, FOTG_WAVE);
  return __ballot(s >= 0 && s != *s0) == 0 ? lead : -1;
}

__global__ __launch_bounds__(COMP_THREADS) void comp_tile_kernel(const unsigned char *__restrict__ code, int n, int w, int h, int ntx,
                                                                 unsigned fgset, int conn8, int *__restrict__ par_out, int *__restrict__ aux)
{
  __shared__ int par[COMP_TILE];
  const CompTile T = comp_tile(n, ntx);
  const int tid = threadIdx.x, l0 = tid * 4, lx0 = (tid & 15) * 4, ly = tid >> 4;
  const int x0 = T.tx0 + lx0, y = T.ty0 + ly;
  const size_t base = (size_t)T.img * w * h;
  unsigned word = 0xffffffffu;                          // (a code >= 8: background)
  if (y < h && x0 < w) {
    const unsigned char *o = code + base + (size_t)y * w + x0;
    if (x0 + 3 < w && (((size_t)o) & 3) == 0) {
      word = *reinterpret_cast<const unsigned *>(o);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (x0 + i < w) word = (word & ~(0xffu << (8 * i))) | ((unsigned)o[i] << (8 * i));
    }
  }
  unsigned fg = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const unsigned c = (word >> (8 * i)) & 0xffu;
    if (c < 8 && ((fgset >> c) & 1)) fg |= 1u << i;
  }
  int start = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (i > 0 && !((fg >> (i - 1)) & 1)) start = i;
    par[l0 + i] = ((fg >> i) & 1) ? l0 + start : -1;
  }
  __syncthreads();
  constexpr int WG = __HIP_MEMORY_SCOPE_WORKGROUP;
  auto set = [&](int l) { return __hip_atomic_load(par + l, __ATOMIC_RELAXED, WG) >= 0; };   // (the sign of an entry never changes)
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (!((fg >> i) & 1)) continue;
    const int l = l0 + i, lx = lx0 + i;
    const bool L = i > 0 ? ((fg >> (i - 1)) & 1) != 0 : (lx > 0 && set(l - 1));
    if (i == 0 && L) comp_union<WG>(par, l, l - 1);
    if (ly > 0) {
      const bool U = set(l - COMP_TW), UL = lx > 0 && set(l - COMP_TW - 1), UR = lx < COMP_TW - 1 && set(l - COMP_TW + 1);
      const int m = comp_links(conn8 != 0, L, UL, U, UR);
      if (m & COMP_LINK_U) comp_union<WG>(par, l, l - COMP_TW);
      if (m & COMP_LINK_UL) comp_union<WG>(par, l, l - COMP_TW - 1);
      if (m & COMP_LINK_UR) comp_union<WG>(par, l, l - COMP_TW + 1);
    }
  }
  __syncthreads();
  if (y < h) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (x0 + i >= w) continue;
      const size_t g = base + (size_t)y * w + x0 + i;
      int out = -1;
      if ((fg >> i) & 1) {
        const int r = comp_find<WG>(par, l0 + i);
        out = (T.ty0 + r / COMP_TW) * w + T.tx0 + r % COMP_TW;
      }
      par_out[g] = out;
      aux[g] = 0;
    }
  }
}

// grid (ceil(total / 256), n); thread t < nrow: pixel (t % w, (t / w + 1) COMP_TH), the top row of a tile; the others: pixel
// ((t' / h + 1) COMP_TW, t' % h), the left column of a tile
__global__ __launch_bounds__(COMP_THREADS) void comp_merge_kernel(int *__restrict__ par_all, int w, int h, int conn8, int nrow, int total)
{
  int t = blockIdx.x * COMP_THREADS + threadIdx.x;
  if (t >= total) return;
  int *par = par_all + (size_t)blockIdx.y * w * h;
  constexpr int AG = __HIP_MEMORY_SCOPE_AGENT;
  auto set = [&](int x, int y) {
    return x >= 0 && x < w && y >= 0 && y < h && __hip_atomic_load(par + y * w + x, __ATOMIC_RELAXED, AG) >= 0;
  };
  if (t < nrow) {
    const int j = t / w, x = t - j * w, y = (j + 1) * COMP_TH, p = y * w + x;
    if (!set(x, y)) return;
    const bool L = set(x - 1, y), U = set(x, y - 1);
    const bool UL = set(x - 1, y - 1), UR = conn8 && set(x + 1, y - 1);
    const int m = comp_links(conn8 != 0, L, UL, U, UR);
    if (m & COMP_LINK_U) comp_union<AG>(par, p, p - w);
    if (m & COMP_LINK_UL) comp_union<AG>(par, p, p - w - 1);
    if (m & COMP_LINK_UR) comp_union<AG>(par, p, p - w + 1);
  } else {
    t -= nrow;
    const int i = t / h, y = t - i * h, x = (i + 1) * COMP_TW, p = y * w + x;
    if (!set(x, y)) return;
    if (set(x - 1, y)) {
      comp_union<AG>(par, p, p - 1);
    } else if (conn8) {
      // this pixel's link to its upper left (on a tile's top row the row thread makes it), and the upper-right link of the pixel
      // to the lower left (unless that one lies on a tile's top row): comp_links with L = false resp. U = false
      if (y % COMP_TH != 0 && !set(x, y - 1) && set(x - 1, y - 1)) comp_union<AG>(par, p, p - w - 1);
      if ((y + 1) % COMP_TH != 0 && set(x - 1, y + 1)) comp_union<AG>(par, p, p + w - 1);
    }
  }
}

__global__ __launch_bounds__(COMP_THREADS) void comp_flatten_kernel(int *__restrict__ par_all, int *__restrict__ aux_all, int n, int w, int h,
                                                                    int ntx)
{
  __shared__ int cnt[COMP_TILE];
  __shared__ int rootof[COMP_TILE];
  const CompTile T = comp_tile(n, ntx);
  const int tid = threadIdx.x, l0 = tid * 4, lx0 = (tid & 15) * 4, ly = tid >> 4;
  const int x0 = T.tx0 + lx0, y = T.ty0 + ly;
  int *par = par_all + (size_t)T.img * w * h, *aux = aux_all + (size_t)T.img * w * h;
#pragma unroll
  for (int i = 0; i < 4; ++i) cnt[l0 + i] = 0;
  __syncthreads();
  const int g0 = y * w + x0;
  int slot[4];
  // the group of a pixel: the tile-local root its parent still names (for a pixel that was such a root: itself, or the root of
  // this tile it was hung on -- the same component either way)
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    slot[i] = -1;
    if (y < h && x0 + i < w) {
      const int pv = par[g0 + i];
      if (pv >= 0) {
        slot[i] = l0 + i;
        if (pv != g0 + i) {
          const int ky = pv / w, kx = pv - ky * w;
          if (ky >= T.ty0 && ky < T.ty0 + COMP_TH && kx >= T.tx0 && kx < T.tx0 + COMP_TW) slot[i] = (ky - T.ty0) * COMP_TW + (kx - T.tx0);
        }
      }
    }
  }
  // per thread over its run, per wave where it has one group only
  int s = -1, c = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (slot[i] < 0) continue;
    if (s == -1) s = slot[i];
    else if (s != slot[i]) s = -2;
    ++c;
  }
  int s0 = 0;
  const int lead = comp_wave_leader(s, &s0);
  if (lead >= 0) {
    c = comp_wave_sum(c);
    if ((tid & (FOTG_WAVE - 1)) == lead) atomicAdd(&cnt[s0], c);
  } else if (s >= 0) {
    atomicAdd(&cnt[s], c);
  } else if (s == -2) {
    int cur = -1, k = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (slot[i] != cur && k > 0) { atomicAdd(&cnt[cur], k); k = 0; }
      cur = slot[i];
      if (cur >= 0) ++k;
    }
    if (k > 0) atomicAdd(&cnt[cur], k);
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int k = cnt[l0 + i];
    if (k > 0) {                                        // (this pixel is a group's key: foreground, inside the image)
      const int r = comp_find<__HIP_MEMORY_SCOPE_AGENT>(par, g0 + i);
      atomicAdd(&aux[r], k);
      rootof[l0 + i] = r;
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (slot[i] < 0) continue;
    const int r = rootof[slot[i]];
    __hip_atomic_store(par + g0 + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // (other tiles' finds may pass through here)
    if (r != g0 + i) aux[g0 + i] = slot[i];
  }
}

// the workgroup's sum of v, valid in thread 0
__device__ __forceinline__ int comp_block_sum(int v, int *ws)
{
  v = comp_wave_sum(v);
  if ((threadIdx.x & (FOTG_WAVE - 1)) == 0) ws[threadIdx.x / FOTG_WAVE] = v;
  __syncthreads();
  int t = 0;
  if (threadIdx.x == 0)
    for (int i = 0; i < COMP_THREADS / FOTG_WAVE; ++i) t += ws[i];
  __syncthreads();
  return t;
}

// grid (chunks, n): chunk blockIdx.x holds the linear indices blockIdx.x 1024 .. + 1023, four per thread
__global__ __launch_bounds__(COMP_THREADS) void comp_count_kernel(const int *__restrict__ lab_all, const int *__restrict__ aux_all, int hw,
                                                                  long long min_area, int *__restrict__ chunk_cnt,
                                                                  long long *__restrict__ stats)
{
  __shared__ int ws[COMP_THREADS / FOTG_WAVE];
  const size_t base = (size_t)blockIdx.y * hw;
  const int i0 = (blockIdx.x * COMP_THREADS + threadIdx.x) * 4;
  int nfg = 0, nroot = 0, nkept = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i = i0 + k;
    if (i >= hw) continue;
    const int lab = lab_all[base + i];
    nfg += lab >= 0;
    if (lab == i) {
      ++nroot;
      nkept += (long long)aux_all[base + i] >= min_area;
    }
  }
  nfg = comp_block_sum(nfg, ws);
  nroot = comp_block_sum(nroot, ws);
  nkept = comp_block_sum(nkept, ws);
  if (threadIdx.x == 0) {
    chunk_cnt[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = nkept;
    if (stats) {
      unsigned long long *st = reinterpret_cast<unsigned long long *>(stats) + (size_t)blockIdx.y * COMP_NSTAT;
      if (nfg) atomicAdd(st + 0, (unsigned long long)nfg);
      if (nroot) atomicAdd(st + 1, (unsigned long long)nroot);
      if (nkept) atomicAdd(st + 2, (unsigned long long)nkept);
    }
  }
}

// grid n: the chunk counts of image blockIdx.x become their exclusive prefix sums
__global__ __launch_bounds__(COMP_THREADS) void comp_scan_kernel(int *__restrict__ chunk_cnt, int chunks, int max_objects,
                                                                 long long *__restrict__ stats)
{
  __shared__ int part[COMP_THREADS];
  int *c = chunk_cnt + (size_t)blockIdx.x * chunks;
  const int per = (chunks + COMP_THREADS - 1) / COMP_THREADS;
  const int a = min(chunks, (int)threadIdx.x * per), b = min(chunks, a + per);
  int s = 0;
  for (int i = a; i < b; ++i) s += c[i];
  part[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    int run = 0;
    for (int i = 0; i < COMP_THREADS; ++i) { const int v = part[i]; part[i] = run; run += v; }
    if (stats) stats[(size_t)blockIdx.x * COMP_NSTAT + 3] = run < max_objects ? run : max_objects;
  }
  __syncthreads();
  int run = part[threadIdx.x];
  for (int i = a; i < b; ++i) { const int v = c[i]; c[i] = run; run += v; }
}

// grid (chunks, n): the kept roots of the chunk, in raster order, take the rows chunk_off + rank
__global__ __launch_bounds__(COMP_THREADS) void comp_emit_kernel(const int *__restrict__ lab_all, int *__restrict__ aux_all, int w, int hw,
                                                                 long long min_area, const int *__restrict__ chunk_off, int max_objects,
                                                                 long long *__restrict__ objects)
{
  __shared__ int ws[COMP_THREADS / FOTG_WAVE];
  const size_t base = (size_t)blockIdx.y * hw;
  const int i0 = (blockIdx.x * COMP_THREADS + threadIdx.x) * 4;
  unsigned root = 0, kept = 0;
  int area[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i = i0 + k;
    area[k] = 0;
    if (i < hw && lab_all[base + i] == i) {
      root |= 1u << k;
      area[k] = aux_all[base + i];
      if ((long long)area[k] >= min_area) kept |= 1u << k;
    }
  }
  const int mine = __popc(kept), lane = threadIdx.x & (FOTG_WAVE - 1), wave = threadIdx.x / FOTG_WAVE;
  int incl = mine;
#pragma unroll
  for (int o = 1; o < FOTG_WAVE; o <<= 1) {
    const int v = __shfl_up(incl, o, FOTG_WAVE);
    if (lane >= o) incl += v;
  }
  if (lane == FOTG_WAVE - 1) ws[wave] = incl;
  __syncthreads();
  int row = chunk_off[(size_t)blockIdx.y * gridDim.x + blockIdx.x] + incl - mine;
  for (int i = 0; i < wave; ++i) row += ws[i];
  long long *obj = objects + (size_t)blockIdx.y * max_objects * COMP_NREC;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (!((root >> k) & 1)) continue;
    int r = -1;
    if ((kept >> k) & 1) {
      if (row < max_objects) {
        r = row;
        long long *o = obj + (size_t)row * COMP_NREC;
        const int h = hw / w;
        o[0] = i0 + k; o[1] = area[k]; o[2] = w; o[3] = h; o[4] = -1; o[5] = -1;     // the box: neutral elements of min and max
      }
      ++row;
    }
    aux_all[base + i0 + k] = r;
  }
}

// values: n x h x w x 2 (VAL) or unused.  ids: n x h x w or null.
template <bool VAL>
__global__ __launch_bounds__(COMP_THREADS) void comp_reduce_kernel(const int *__restrict__ lab_all, const int *__restrict__ aux_all,
                                                                   const float *__restrict__ values, int n, int w, int h, int ntx,
                                                                   int max_objects, long long *__restrict__ objects, int *__restrict__ ids)
{
  constexpr int K = VAL ? 9 : 6;                         // xmin ymin xmax ymax sx sy [nv su sv]
  __shared__ int acc[K][COMP_TILE];
  __shared__ int rowof[COMP_TILE];
  const CompTile T = comp_tile(n, ntx);
  const int tid = threadIdx.x, l0 = tid * 4, lx0 = (tid & 15) * 4, ly = tid >> 4;
  const int x0 = T.tx0 + lx0, y = T.ty0 + ly;
  const size_t base = (size_t)T.img * w * h;
  const int *lab_img = lab_all + base, *aux = aux_all + base;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    acc[0][l0 + i] = 0x7fffffff; acc[1][l0 + i] = 0x7fffffff; acc[2][l0 + i] = -1; acc[3][l0 + i] = -1;
#pragma unroll
    for (int k = 4; k < K; ++k) acc[k][l0 + i] = 0;
  }
  __syncthreads();
  const int g0 = y * w + x0;
  int slot[4], lab[4], U[4], V[4], ok[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    slot[i] = -1; lab[i] = -1; U[i] = V[i] = ok[i] = 0;
    if (y < h && x0 + i < w) {
      lab[i] = lab_img[g0 + i];
      if (lab[i] >= 0) {
        slot[i] = lab[i] == g0 + i ? l0 + i : aux[g0 + i];
        if (VAL) {
          const float u = values[2 * (base + g0 + i)], v = values[2 * (base + g0 + i) + 1];
          if (comp_known(u, v)) { ok[i] = 1; U[i] = (int)rintf(u * 256.f); V[i] = (int)rintf(v * 256.f); }
        }
      }
    }
  }
  auto flush = [&](int s, int xa, int xb, int sx, int cn, int nv, int su, int sv) {
    atomicMin(&acc[0][s], xa); atomicMin(&acc[1][s], y); atomicMax(&acc[2][s], xb); atomicMax(&acc[3][s], y);
    atomicAdd(&acc[4][s], sx); atomicAdd(&acc[5][s], cn * y);
    if (VAL && nv) { atomicAdd(&acc[6][s], nv); atomicAdd(&acc[7][s], su); atomicAdd(&acc[8][s], sv); }
  };
  int s = -1, xa = 0x7fffffff, xb = -1, sx = 0, cn = 0, nv = 0, su = 0, sv = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (slot[i] < 0) continue;
    if (s == -1) s = slot[i];
    else if (s != slot[i]) s = -2;
    xa = min(xa, x0 + i); xb = max(xb, x0 + i); sx += x0 + i; ++cn;
    nv += ok[i]; su += U[i]; sv += V[i];
  }
  int s0 = 0;
  const int lead = comp_wave_leader(s, &s0);
  if (lead >= 0) {
    // one group in the whole wave (its rows y differ: the wave spans four rows of the tile)
    const int ya = comp_wave_min(s >= 0 ? y : 0x7fffffff), yb = comp_wave_max(s >= 0 ? y : -1);
    const int sy = comp_wave_sum(cn * y);
    xa = comp_wave_min(xa); xb = comp_wave_max(xb); sx = comp_wave_sum(sx);
    if (VAL) { nv = comp_wave_sum(nv); su = comp_wave_sum(su); sv = comp_wave_sum(sv); }
    if ((tid & (FOTG_WAVE - 1)) == lead) {
      atomicMin(&acc[0][s0], xa); atomicMin(&acc[1][s0], ya); atomicMax(&acc[2][s0], xb); atomicMax(&acc[3][s0], yb);
      atomicAdd(&acc[4][s0], sx); atomicAdd(&acc[5][s0], sy);
      if (VAL && nv) { atomicAdd(&acc[6][s0], nv); atomicAdd(&acc[7][s0], su); atomicAdd(&acc[8][s0], sv); }
    }
  } else if (s >= 0) {
    flush(s, xa, xb, sx, cn, nv, su, sv);
  } else if (s == -2) {
    int cur = -1;
    xa = 0; xb = -1; sx = cn = nv = su = sv = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (slot[i] != cur && cn > 0) { flush(cur, xa, xb, sx, cn, nv, su, sv); sx = cn = nv = su = sv = 0; }
      cur = slot[i];
      if (cur >= 0) {
        if (cn == 0) xa = x0 + i;
        xb = x0 + i; sx += x0 + i; ++cn; nv += ok[i]; su += U[i]; sv += V[i];
      }
    }
    if (cn > 0) flush(cur, xa, xb, sx, cn, nv, su, sv);
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (acc[2][l0 + i] < 0) continue;                    // no pixel in this group (else this pixel is its key: foreground)
    const int row = lab[i] >= 0 ? aux[lab[i]] : -1;
    rowof[l0 + i] = row;
    if (row < 0) continue;
    unsigned long long *o = reinterpret_cast<unsigned long long *>(objects) + ((size_t)T.img * max_objects + row) * COMP_NREC;
    long long *os = reinterpret_cast<long long *>(o);
    atomicMin(os + 2, (long long)acc[0][l0 + i]); atomicMin(os + 3, (long long)acc[1][l0 + i]);
    atomicMax(os + 4, (long long)acc[2][l0 + i]); atomicMax(os + 5, (long long)acc[3][l0 + i]);
    atomicAdd(o + 6, (unsigned long long)(long long)acc[4][l0 + i]);
    atomicAdd(o + 7, (unsigned long long)(long long)acc[5][l0 + i]);
    if (VAL && acc[6][l0 + i]) {
      atomicAdd(o + 8, (unsigned long long)(long long)acc[6][l0 + i]);
      atomicAdd(o + 9, (unsigned long long)(long long)acc[7][l0 + i]);
      atomicAdd(o + 10, (unsigned long long)(long long)acc[8][l0 + i]);
    }
  }
  if (!ids) return;
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (y < h && x0 + i < w) ids[base + g0 + i] = slot[i] >= 0 ? rowof[slot[i]] : -1;
}

}  // namespace fotg
