// objtracks.hip.h -- object tracks: the objects of fotg_label_components (components.hip.h) linked across the frames of a sequence
// by the flow, which says per pixel where an object's pixels land in the next frame.  Integer arithmetic from the first step to
// the last, so any order of reduction gives the same bytes.  The definition, in order:
//
// Step 1, overlap votes, per pair of frames a -> b.  ids_a, ids_b: int32 n x h x w, the `ids` of fotg_label_components (the row of
// the pixel's object, -1 for none); flow: n x h x w x 2 f32, a -> b on a's grid; mask: null or n x h x w bytes in the alphabet of the
// consistency check (only 0 votes); row counts ka, kb in 1 .. 1024 (OT_MAX_K); 1 <= w, h <= 16384 (OT_MAX_DIM).  For every pixel (x, y)
// with i = ids_a in [0, ka) -- any other value, negative or >= ka, is background and is ignored -- in this order:
//   1. inadmissible = mask != 0 || u or v not finite || |u| > 4096 || |v| > 4096:  sent[i][3]++
//   2. otherwise xq = x + (int)rintf(u), yq = y + (int)rintf(v) (to nearest even); the target outside the frame:  sent[i][2]++
//   3. otherwise j = ids_b[yq][xq]:  j in [0, kb): votes[i][j]++ and sent[i][0]++;  otherwise (background): sent[i][1]++
// Outputs: votes int32 n x ka x kb, sent int64 n x ka x 4, both cleared by the call.  The four columns of sent[i] add up to the
// number of pixels carrying id i.  Pairs of a batch never mix.
//
// Step 2, links.  votes; the two object tables (int64 n x k x 11, the area is column 1); min_votes >= 1; min_frac256 in 0 .. 256.
//   best_b(i) = the lowest j that maximises votes[i][.], defined only if that maximum is > 0;  best_a(j) = the lowest i that
//   maximises votes[.][j], likewise
//   i and j are matched iff best_b(i) = j && best_a(j) = i && votes[i][j] >= min_votes &&
//                           256 votes[i][j] >= min_frac256 min(area_a[i], area_b[j])          (64-bit integers)
// Outputs: link_ab int32 n x ka x 3 = (the matched j or -1, best_b(i) or -1, the votes of that best or 0), link_ba int32 n x kb x 3
// likewise.  A match is one-to-one by construction.
//
// Step 3, tracks over one sequence (time is the batch axis): T + 1 frames, T pairs, K rows per frame; a row counts as written iff
// its area > 0.
//   frame 0: the written rows get the track ids 0, 1, .. in row order
//   frame t + 1, rows in ascending order: a written row j whose link_ba[t][j] names a match i in [0, K) inherits track[t][i]; any
//   other written row gets the next unused id;  unwritten rows get -1
// Outputs: track int32 (T + 1) x K; tracks int64 max_tracks x 8, one row per track id < max_tracks, the others zero: first_frame,
// last_frame, first_row, last_row, sum of area, max area, sum of votes over its links, end; stats int64 x 4 = tracks started, tracks
// with a table row, links made, tracks alive at frame T.  A track has exactly one object per frame from first_frame to last_frame.
//   end, decided at the track's last frame t < T from row i = last_row: 3 if link_ab[t][i] has no best target (no pixel of it landed
//   on an object: it left the frame or vanished), 1 if its best target j has best_a(j) = i (mutual, but a threshold failed), 2
//   otherwise (the target prefers another object: a merge, or a tie lost to a lower row);  0: alive at frame T
// All ties are decided by the lower index.  tests/tracks_ref.py restates all of this in numpy.
//
// objvote_kernel<Src>: the hot path, streaming.  A wave owns a strip of 256 pixels x OT_ROWS rows, a lane four adjacent pixels of
// each row; the strip is shifted left by the row's misalignment, so that the lane's four ids (16 bytes), four vectors (2 x 16 bytes)
// and four mask bytes leave in whole loads wherever the four pixels lie inside the row, and one by one at its two ends.  A row whose
// 256 pixels are all background costs its ids and nothing more: neither flow nor mask is read.  Every foreground pixel makes one
// key, (i, j) or (i, the column of sent); equal keys are counted within the wave before anything leaves it: the wave walks its
// distinct keys (v_readlane of a live key, a ballot of its equals over the four pixel slots, the popcounts added) and keeps them, a
// key and a count per lane, over all rows of the strip; a key met again adds to its lane.  When the strip ends the lanes put their
// keys into a table of 256 slots in LDS, where the four strips of the workgroup meet, and one thread per slot adds its count with
// one integer atomic: a workgroup of one object costs two atomics for 8192 pixels.  (A 65th key in a strip sends the 64 held ones
// straight to memory.)  Without the table the one-object extreme takes 1.15 times as long (docs/EXPERIMENTS.md).
// objlink_kernel: one workgroup per pair; a wave per row for the row arg-max, a thread per column for the column arg-max, both held
// in LDS, then the two link tables.  objtrack_kernel: one workgroup walks t = 0 .. T, one thread per row; the new ids of a frame
// come from a workgroup prefix sum over "written and unmatched".  No kernel waits for another workgroup; none uses scratch.
#pragma once
#include <type_traits>
#include "common.h"
#include "flowsrc.hip.h"

namespace fotg {

enum { OT_THREADS = 256, OT_WAVES = OT_THREADS / FOTG_WAVE, OT_ROWS = 8, OT_STRIP = 4 * FOTG_WAVE, OT_MAX_K = 1024, OT_MAX_DIM = 16384,
       OT_MAX_TRACKS = 65536, OT_NLINK = 3, OT_NSENT = 4, OT_NTRACK = 8, OT_NSTAT = 4, OT_NREC = 11, OT_AREA = 1 };

// the lane's pending (key, count) leaves: key = i (kb + 4) + j for a vote, i (kb + 4) + kb + c for column c = 1 .. 3 of sent
__device__ __forceinline__ void ot_flush(int mk, int mt, int kb, int *__restrict__ votes, long long *__restrict__ sent)
{
  if (mk < 0) return;
  const int ks = kb + OT_NSENT, i = mk / ks, r = mk - i * ks;
  if (r < kb) {
    atomicAdd(votes + (size_t)i * kb + r, mt);
    atomicAdd(reinterpret_cast<unsigned long long *>(sent) + OT_NSENT * i, (unsigned long long)mt);
  } else {
    atomicAdd(reinterpret_cast<unsigned long long *>(sent) + OT_NSENT * i + (r - kb), (unsigned long long)mt);
  }
}

// flow: the vectors of a -> b; ids_a, ids_b: n x h x w; mask: n x h x w bytes or null; votes (n x ka x kb) and sent (n x ka x 4) were
// cleared before the launch.  vec: ids_a, a dense flow and the mask are aligned for 16-byte (the mask: 4-byte) loads.
// grid (ceil((w + 3) / 256), ceil(h / (OT_WAVES OT_ROWS)), n).
template <class Src>
__global__ __launch_bounds__(OT_THREADS) void objvote_kernel(Src flow, const int *__restrict__ ids_a, const int *__restrict__ ids_b,
                                                             const unsigned char *__restrict__ mask, int w, int h, int ka, int kb,
                                                             int vec, int *__restrict__ votes, long long *__restrict__ sent)
{
  const int lane = threadIdx.x % FOTG_WAVE, wave = threadIdx.x / FOTG_WAVE;
  const int pair = blockIdx.z;
  const size_t img = (size_t)pair * w * h;
  const int y0 = ((int)blockIdx.y * OT_WAVES + wave) * OT_ROWS;
  const int ks = kb + OT_NSENT;
  votes += (size_t)pair * ka * kb;
  sent += (size_t)pair * ka * OT_NSENT;
  int mk = -1, mt = 0, held = 0;                             // the lane's pending key and count; held: lanes in use (wave-uniform)
  __shared__ int tkey[OT_THREADS], tcnt[OT_THREADS];         // the workgroup's table between its waves and memory: key, count
  tkey[threadIdx.x] = -1; tcnt[threadIdx.x] = 0;
  __syncthreads();
  for (int r = 0; r < OT_ROWS; ++r) {
    const int y = y0 + r;
    if (y >= h) break;                                       // wave-uniform
    const size_t row = img + (size_t)y * w;
    const int x = ((int)blockIdx.x * FOTG_WAVE + lane) * 4 - (vec ? (int)(row & 3) : 0);
    const bool whole = vec && x >= 0 && x + 4 <= w;          // then row + x is a multiple of four
    int ia[4];
    if (whole) {
      const int4 t = *reinterpret_cast<const int4 *>(ids_a + row + x);
      ia[0] = t.x; ia[1] = t.y; ia[2] = t.z; ia[3] = t.w;
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) ia[q] = (x + q >= 0 && x + q < w) ? ids_a[row + x + q] : -1;
    }
    unsigned live = 0;                                       // bit q: pixel q carries an object of a
#pragma unroll
    for (int q = 0; q < 4; ++q) live |= ((unsigned)ia[q] < (unsigned)ka ? 1u : 0u) << q;
    if (__ballot(live != 0) == 0) continue;                  // all background: nothing further

    int key[4] = {-1, -1, -1, -1};
    if (live) {
      float u[4], v[4];
      unsigned mk4 = 0;                                      // the four mask bytes
      if (whole) {
        if constexpr (std::is_same<Src, DenseSrc>::value) {
          const float4 f0 = *reinterpret_cast<const float4 *>(flow.flow + 2 * (row + x));
          const float4 f1 = *reinterpret_cast<const float4 *>(flow.flow + 2 * (row + x) + 4);
          u[0] = f0.x; v[0] = f0.y; u[1] = f0.z; v[1] = f0.w; u[2] = f1.x; v[2] = f1.y; u[3] = f1.z; v[3] = f1.w;
        } else {
#pragma unroll
          for (int q = 0; q < 4; ++q) flow.at((long)(row + x + q), pair, x + q, y, u[q], v[q]);
        }
        if (mask) mk4 = *reinterpret_cast<const unsigned *>(mask + row + x);
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          u[q] = v[q] = 0.f;
          if ((live >> q) & 1) {
            flow.at((long)(row + x + q), pair, x + q, y, u[q], v[q]);
            if (mask) mk4 |= (unsigned)mask[row + x + q] << (8 * q);
          }
        }
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (!((live >> q) & 1)) continue;
        int c = 3;
        if (((mk4 >> (8 * q)) & 0xffu) == 0 && fabsf(u[q]) <= 4096.f && fabsf(v[q]) <= 4096.f) {   // false for a NaN or an infinity
          const int xq = x + q + (int)rintf(u[q]), yq = y + (int)rintf(v[q]);
          c = 2;
          if (xq >= 0 && xq < w && yq >= 0 && yq < h) {
            const int j = ids_b[img + (size_t)yq * w + xq];
            c = (unsigned)j < (unsigned)kb ? j - kb : 1;     // a vote: the key's column is j
          }
        }
        key[q] = ia[q] * ks + kb + c;
      }
    }

    // the wave's distinct keys, one per turn
    for (;;) {
      const unsigned long long any = __ballot(live != 0);
      if (any == 0) break;
      const int mine = (live & 1) ? key[0] : (live & 2) ? key[1] : (live & 4) ? key[2] : key[3];
      const int k = __builtin_amdgcn_readlane(mine, __builtin_amdgcn_readfirstlane(__ffsll((long long)any) - 1));
      int total = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const bool e = ((live >> q) & 1) && key[q] == k;
        total += __popcll(__ballot(e));
        if (e) live &= ~(1u << q);
      }
      if (__ballot(mk == k) != 0) {
        if (mk == k) mt += total;
      } else {
        if (held == FOTG_WAVE) {                             // every lane holds a key: they leave, the wave starts over
          ot_flush(mk, mt, kb, votes, sent);
          mk = -1; mt = 0; held = 0;
        }
        if (lane == held) { mk = k; mt = total; }
        ++held;
      }
    }
  }
  // the four strips of the workgroup mostly hold the same objects: their keys meet in the table (open addressing, eight probes; a
  // key that finds no slot leaves on its own), and one thread per slot adds what gathered there
  if (mk >= 0) {
    unsigned slot = ((unsigned)mk * 2654435761u) >> 24;      // 0 .. OT_THREADS - 1
    bool placed = false;
    for (int probe = 0; probe < 8 && !placed; ++probe, slot = (slot + 1) % OT_THREADS) {
      const int old = atomicCAS(&tkey[slot], -1, mk);
      if (old == -1 || old == mk) { atomicAdd(&tcnt[slot], mt); placed = true; }
    }
    if (!placed) ot_flush(mk, mt, kb, votes, sent);
  }
  __syncthreads();
  ot_flush(tkey[threadIdx.x], tcnt[threadIdx.x], kb, votes, sent);
}

// the larger value, the lower index among equals, over the wave (all 64 lanes active), in every lane
__device__ __forceinline__ void ot_wave_argmax(int &v, int &idx)
{
#pragma unroll
  for (int o = 1; o < FOTG_WAVE; o <<= 1) {
    const int v2 = __shfl_xor(v, o, FOTG_WAVE), i2 = __shfl_xor(idx, o, FOTG_WAVE);
    if (v2 > v || (v2 == v && i2 < idx)) { v = v2; idx = i2; }
  }
}

// grid n, OT_THREADS threads: the links of pair blockIdx.x from its votes (ka x kb) and the areas of the two object tables
__global__ __launch_bounds__(OT_THREADS) void objlink_kernel(const int *__restrict__ votes, const long long *__restrict__ objects_a,
                                                             const long long *__restrict__ objects_b, int ka, int kb, int min_votes,
                                                             int min_frac256, int *__restrict__ link_ab, int *__restrict__ link_ba)
{
  __shared__ int best_b[OT_MAX_K], vote_b[OT_MAX_K], best_a[OT_MAX_K], vote_a[OT_MAX_K];
  const int lane = threadIdx.x % FOTG_WAVE, wave = threadIdx.x / FOTG_WAVE;
  const size_t pair = blockIdx.x;
  votes += pair * ka * kb;
  objects_a += pair * ka * OT_NREC;
  objects_b += pair * kb * OT_NREC;
  link_ab += pair * ka * OT_NLINK;
  link_ba += pair * kb * OT_NLINK;
  for (int i = wave; i < ka; i += OT_WAVES) {                // a wave per row: its lanes stride over the columns
    int bv = 0, bj = OT_MAX_K;
    for (int j = lane; j < kb; j += FOTG_WAVE) {
      const int t = votes[(size_t)i * kb + j];
      if (t > bv) { bv = t; bj = j; }                        // strictly greater: the lowest j of the lane stays
    }
    ot_wave_argmax(bv, bj);
    if (lane == 0) { best_b[i] = bv > 0 ? bj : -1; vote_b[i] = bv; }
  }
  for (int j = threadIdx.x; j < kb; j += OT_THREADS) {       // a thread per column: adjacent threads read adjacent votes
    int bv = 0, bi = -1;
    for (int i = 0; i < ka; ++i) {
      const int t = votes[(size_t)i * kb + j];
      if (t > bv) { bv = t; bi = i; }
    }
    best_a[j] = bi; vote_a[j] = bv;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < ka; i += OT_THREADS) {
    const int j = best_b[i], t = vote_b[i];
    int m = -1;
    if (j >= 0 && best_a[j] == i && t >= min_votes) {
      const long long aa = objects_a[(size_t)i * OT_NREC + OT_AREA], ab = objects_b[(size_t)j * OT_NREC + OT_AREA];
      if (256LL * t >= (long long)min_frac256 * (aa < ab ? aa : ab)) m = j;
    }
    link_ab[OT_NLINK * i] = m; link_ab[OT_NLINK * i + 1] = j; link_ab[OT_NLINK * i + 2] = t;
  }
  for (int j = threadIdx.x; j < kb; j += OT_THREADS) {
    const int i = best_a[j], t = vote_a[j];
    int m = -1;
    if (i >= 0 && best_b[i] == j && t >= min_votes) {
      const long long aa = objects_a[(size_t)i * OT_NREC + OT_AREA], ab = objects_b[(size_t)j * OT_NREC + OT_AREA];
      if (256LL * t >= (long long)min_frac256 * (aa < ab ? aa : ab)) m = i;
    }
    link_ba[OT_NLINK * j] = m; link_ba[OT_NLINK * j + 1] = i; link_ba[OT_NLINK * j + 2] = t;
  }
}

// one workgroup of ceil(K / 64) waves, thread j = row j: the tracks of the sequence.  objects (T + 1) x K x 11; link_ab, link_ba T x K x 3;
// track (T + 1) x K; tracks (max_tracks x 8) and stats (4, or null) were cleared before the launch.
__global__ __launch_bounds__(OT_MAX_K) void objtrack_kernel(const long long *__restrict__ objects, const int *__restrict__ link_ab,
                                                            const int *__restrict__ link_ba, int T, int K, int max_tracks,
                                                            int *__restrict__ track, long long *__restrict__ tracks,
                                                            long long *__restrict__ stats)
{
  __shared__ int trk[2][OT_MAX_K];                           // the track ids of the previous and of this frame
  __shared__ int wsum[OT_MAX_K / FOTG_WAVE];
  __shared__ int s_links[OT_MAX_K / FOTG_WAVE];
  const int j = threadIdx.x, lane = j % FOTG_WAVE, wave = j / FOTG_WAVE, nwave = blockDim.x / FOTG_WAVE;
  const bool row = j < K;
  unsigned long long *tr = reinterpret_cast<unsigned long long *>(tracks);
  int next = 0, links = 0, alive = 0;                        // next: the same in every thread; links: the thread's own; alive: the wave's
  for (int t = 0; t <= T; ++t) {
    const long long area = row ? objects[((size_t)t * K + j) * OT_NREC + OT_AREA] : 0;
    const bool written = area > 0;
    int m = -1, mv = 0;
    if (written && t > 0) {
      const int *l = link_ba + ((size_t)(t - 1) * K + j) * OT_NLINK;
      m = l[0]; mv = l[2];
      if (m < 0 || m >= K) m = -1;
    }
    const bool fresh = written && m < 0;
    // the exclusive prefix sum of `fresh` over the rows
    const unsigned long long b = __ballot(fresh);
    if (lane == 0) wsum[wave] = __popcll(b);
    __syncthreads();
    int before = __popcll(b & ((1ULL << lane) - 1)), total = 0;
    for (int k = 0; k < nwave; ++k) {
      const int s = wsum[k];
      before += k < wave ? s : 0;
      total += s;
    }
    int id = -1;
    if (fresh) id = next + before;
    else if (written) id = trk[(t - 1) & 1][m];
    next += total;
    if (row) {
      trk[t & 1][j] = id;
      track[(size_t)t * K + j] = id;
    }
    if (id >= 0 && id < max_tracks) {                        // one object per track and frame: one thread per table row
      unsigned long long *rec = tr + (size_t)id * OT_NTRACK;
      if (fresh) { rec[0] = (unsigned long long)t; rec[2] = (unsigned long long)j; }
      rec[1] = (unsigned long long)t; rec[3] = (unsigned long long)j;
      atomicAdd(rec + 4, (unsigned long long)area);
      atomicMax(rec + 5, (unsigned long long)area);
      if (!fresh) atomicAdd(rec + 6, (unsigned long long)mv);
      int end = 0;
      if (t < T) {
        const int *l = link_ab + ((size_t)t * K + j) * OT_NLINK;
        const int best = l[1];
        if (l[0] < 0) end = (best < 0 || best >= K) ? 3 : (link_ba[((size_t)t * K + best) * OT_NLINK + 1] == j ? 1 : 2);
      }
      rec[7] = (unsigned long long)end;                      // the last frame that reaches the track decides
    }
    links += written && !fresh;
    if (t == T) alive = __popcll(__ballot(written));
    __syncthreads();                                         // trk[t & 1] is complete; wsum may be rewritten
  }
  if (stats) {
    int ls = links;
#pragma unroll
    for (int o = 1; o < FOTG_WAVE; o <<= 1) ls += __shfl_xor(ls, o, FOTG_WAVE);
    if (lane == 0) { wsum[wave] = alive; s_links[wave] = ls; }
    __syncthreads();
    if (j == 0) {
      long long l = 0, a = 0;
      for (int k = 0; k < nwave; ++k) { l += s_links[k]; a += wsum[k]; }
      stats[0] = next; stats[1] = next < max_tracks ? next : max_tracks; stats[2] = l; stats[3] = a;
    }
  }
}

}  // namespace fotg
