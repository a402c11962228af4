// examples/temporal_filter.cpp -- temporal denoising over the C-ABI and the C++ shim: a file of raw 8-bit gray frames in, every frame
// averaged with its neighbours at distance +-1 .. +-radius, each pulled onto it along its own flow and weighted per pixel by the
// local photometric difference.  Per centre frame: one batch of 2 radius flows (centre -> neighbour), then one fused call that
// upsamples the coarse flows on the fly, gathers the neighbours and writes the filtered frame; no full-resolution flow and no
// warped frame is ever written.
//
//   hipcc -O2 -Iinclude examples/temporal_filter.cpp -Lflowonthego_amd -lfotg -Wl,-rpath,$PWD/flowonthego_amd -o examples/temporal_filter
//   examples/temporal_filter frames.raw width height count out.raw [radius 1..4] [tau] [operating point 1..4]
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "fotg/temporal.h"

static void hip_check(hipError_t e, const char *what)
{
  if (e != hipSuccess) { fprintf(stderr, "%s: %s\n", what, hipGetErrorString(e)); exit(1); }
}

static void fotg_check(int st, const char *what)
{
  if (st != FOTG_OK) { fprintf(stderr, "%s: %s\n", what, fotg_strerror(st)); exit(1); }
}

int main(int argc, char *argv[])
{
  if (argc < 6 || argc > 9) {
    fprintf(stderr, "\n  usage: %s frames.raw width height count out.raw [radius 1..4] [tau] [operating point 1..4]\n\n", argv[0]);
    return 1;
  }
  const int w = atoi(argv[2]), h = atoi(argv[3]), T = atoi(argv[4]);
  const int radius = argc > 6 ? atoi(argv[6]) : 1;
  const float tau = argc > 7 ? (float)atof(argv[7]) : 30.f;
  const int op = argc > 8 ? atoi(argv[8]) : 2;
  if (w <= 0 || h <= 0 || T < 1 || radius < 1 || radius > 4 || !(tau > 0.f)) {
    fprintf(stderr, "temporal_filter: bad size, count, radius or tau\n");
    return 1;
  }
  const int K = 2 * radius;
  const size_t npix = (size_t)w * h;
  std::vector<unsigned char> frames(npix * T);
  FILE *f = fopen(argv[1], "rb");
  const size_t got = f ? fread(frames.data(), 1, frames.size(), f) : 0;
  if (f) fclose(f);
  if (got != frames.size()) { fprintf(stderr, "temporal_filter: cannot read %zu bytes from %s\n", frames.size(), argv[1]); return 1; }

  fotg_params p;
  fotg_check(fotg_op_point(op, w, 1, &p), "fotg_op_point");
  fotg_ctx *ctx = nullptr;
  fotg_check(fotg_create(&p, w, h, 0, K, &ctx), "fotg_create");           // one centre per batch: K pairs
  int wl, hl;
  fotg_check(fotg_out_size(ctx, &wl, &hl), "fotg_out_size");

  unsigned char *dframes = nullptr, *d0 = nullptr, *d1 = nullptr, *dout = nullptr;
  float *dflows = nullptr;
  double *dstats = nullptr;
  hip_check(hipMalloc((void **)&dframes, npix * T), "hipMalloc");
  hip_check(hipMalloc((void **)&d0, npix * K), "hipMalloc");
  hip_check(hipMalloc((void **)&d1, npix * K), "hipMalloc");
  hip_check(hipMalloc((void **)&dout, npix * T), "hipMalloc");
  hip_check(hipMalloc((void **)&dflows, (size_t)K * wl * hl * 2 * sizeof(float)), "hipMalloc");
  hip_check(hipMalloc((void **)&dstats, (size_t)T * 4 * sizeof(double)), "hipMalloc");
  hip_check(hipMemcpy(dframes, frames.data(), npix * T, hipMemcpyHostToDevice), "hipMemcpy");

  // all on the null stream, in order
  for (int c = 0; c < T; ++c) {
    int nbr[OFC::TEMPORAL_MAX_NEIGHBORS];
    for (int r = 1; r <= radius; ++r) {                                   // -1, +1, -2, +2, ...; -1 = beyond the sequence
      nbr[2 * r - 2] = c - r >= 0 ? c - r : -1;
      nbr[2 * r - 1] = c + r < T ? c + r : -1;
    }
    for (int k = 0; k < K; ++k) {                                         // an absent neighbour keeps its slot in the flow batch
      const int b = nbr[k] >= 0 ? nbr[k] : c;
      hip_check(hipMemcpyAsync(d0 + k * npix, dframes + c * npix, npix, hipMemcpyDeviceToDevice, nullptr), "hipMemcpyAsync");
      hip_check(hipMemcpyAsync(d1 + k * npix, dframes + b * npix, npix, hipMemcpyDeviceToDevice, nullptr), "hipMemcpyAsync");
    }
    fotg_check(fotg_calc_batch_u8(ctx, K, d0, d1, nullptr, dflows, nullptr), "fotg_calc_batch_u8");
    fotg_check(OFC::UpsampleCropTemporalFilter(ctx, dflows, dframes, T, 1, &c, nbr, 1, K, dout + c * npix, nullptr, dstats + 4 * c, tau),
               "fotg_upsample_crop_temporal_filter_u8");
  }

  std::vector<unsigned char> out(npix * T);
  std::vector<double> stats((size_t)T * 4);
  hip_check(hipMemcpy(out.data(), dout, out.size(), hipMemcpyDeviceToHost), "hipMemcpy");
  hip_check(hipMemcpy(stats.data(), dstats, stats.size() * sizeof(double), hipMemcpyDeviceToHost), "hipMemcpy");
  for (int c = 0; c < T; ++c)
    printf("frame %d: mean neighbours used %.3f of %d, unfiltered pixels %.4f\n", c, stats[4 * c + OFC::TEMPORAL_SUM_USED] / npix, K,
           stats[4 * c + OFC::TEMPORAL_UNFILTERED] / npix);
  f = fopen(argv[5], "wb");
  if (!f || fwrite(out.data(), 1, out.size(), f) != out.size()) { fprintf(stderr, "temporal_filter: cannot write %s\n", argv[5]); return 1; }
  fclose(f);
  for (void *q : {(void *)dframes, (void *)d0, (void *)d1, (void *)dout, (void *)dflows, (void *)dstats}) hip_check(hipFree(q), "hipFree");
  fotg_destroy(ctx);
  return 0;
}
