// examples/clean_mask.cpp -- binary morphology over the C-ABI and the C++ shim: a file of raw masks (one byte per pixel, non-zero =
// set) in, the masks opened by one disc and closed by another out (one byte per pixel, 0 or 1).  Two launches: the opening and the
// closing, each with its intermediate map on chip.
//
//   hipcc -O2 -Iinclude examples/clean_mask.cpp -Lflowonthego_amd -lfotg -Wl,-rpath,$PWD/flowonthego_amd -o examples/clean_mask
//   examples/clean_mask masks.raw width height count out.raw [open 0..8] [close 0..8]
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "fotg/morph.h"

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
  const int w = argc > 3 ? atoi(argv[2]) : 0, h = argc > 3 ? atoi(argv[3]) : 0, n = argc > 4 ? atoi(argv[4]) : 0;
  const int open = argc > 6 ? atoi(argv[6]) : 1, close = argc > 7 ? atoi(argv[7]) : 2;
  if (argc < 6 || argc > 8 || w <= 0 || h <= 0 || w > OFC::MORPH_MAX_DIM || h > OFC::MORPH_MAX_DIM || n < 1 || n > 65535 || open < 0 ||
      open > OFC::MORPH_MAX_RADIUS || close < 0 || close > OFC::MORPH_MAX_RADIUS) {
    fprintf(stderr, "\n  usage: %s masks.raw width height count out.raw [open 0..8] [close 0..8]\n\n", argv[0]);
    return 1;
  }
  const size_t bytes = (size_t)w * h * n;
  std::vector<unsigned char> masks(bytes);
  FILE *f = fopen(argv[1], "rb");
  const size_t got = f ? fread(masks.data(), 1, bytes, f) : 0;
  if (f) fclose(f);
  if (got != bytes) { fprintf(stderr, "clean_mask: cannot read %zu bytes from %s\n", bytes, argv[1]); return 1; }

  unsigned char *dsrc = nullptr, *dtmp = nullptr, *dout = nullptr;
  long long *dstats = nullptr;
  hip_check(hipMalloc((void **)&dsrc, bytes), "hipMalloc");
  hip_check(hipMalloc((void **)&dtmp, bytes), "hipMalloc");
  hip_check(hipMalloc((void **)&dout, bytes), "hipMalloc");
  hip_check(hipMalloc((void **)&dstats, (size_t)2 * n * OFC::MORPH_STATS * sizeof(long long)), "hipMalloc");
  hip_check(hipMemcpy(dsrc, masks.data(), bytes, hipMemcpyHostToDevice), "hipMemcpy");

  fotg_check(OFC::CleanMask(dsrc, n, w, h, open, close, dtmp, dout, dstats), "fotg_morph");

  std::vector<long long> stats((size_t)2 * n * OFC::MORPH_STATS);
  hip_check(hipMemcpy(masks.data(), dout, bytes, hipMemcpyDeviceToHost), "hipMemcpy");
  hip_check(hipMemcpy(stats.data(), dstats, stats.size() * sizeof(long long), hipMemcpyDeviceToHost), "hipMemcpy");
  for (int k = 0; k < n; ++k) {
    const long long *o = &stats[(size_t)k * OFC::MORPH_STATS], *c = &stats[(size_t)(n + k) * OFC::MORPH_STATS];
    printf("mask %d: %lld set pixels, the opening by %d removed %lld, the closing by %d added %lld: %lld set pixels\n", k,
           o[OFC::MORPH_N_BEFORE], open, o[OFC::MORPH_N_REMOVED], close, c[OFC::MORPH_N_ADDED], c[OFC::MORPH_N_AFTER]);
  }
  f = fopen(argv[5], "wb");
  if (!f || fwrite(masks.data(), 1, bytes, f) != bytes) { fprintf(stderr, "clean_mask: cannot write %s\n", argv[5]); return 1; }
  fclose(f);
  for (void *q : {(void *)dsrc, (void *)dtmp, (void *)dout, (void *)dstats}) hip_check(hipFree(q), "hipFree");
  return 0;
}
