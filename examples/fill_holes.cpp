// examples/fill_holes.cpp -- hole filling by pull-push over the C-ABI and the C++ shim: a file of raw 8-bit frames and a file of raw
// hole maps (one byte per pixel, non-zero = hole) in, the frames with their holes filled from the known pixels out.  Three launches
// per call.
//
//   hipcc -O2 -Iinclude examples/fill_holes.cpp -Lflowonthego_amd -lfotg -Wl,-rpath,$PWD/flowonthego_amd -o examples/fill_holes
//   examples/fill_holes frames.raw holes.raw width height channels count out.raw
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "fotg/fill.h"

static void hip_check(hipError_t e, const char *what)
{
  if (e != hipSuccess) { fprintf(stderr, "%s: %s\n", what, hipGetErrorString(e)); exit(1); }
}

static void fotg_check(int st, const char *what)
{
  if (st != FOTG_OK) { fprintf(stderr, "%s: %s\n", what, fotg_strerror(st)); exit(1); }
}

static bool read_all(const char *path, std::vector<unsigned char> &buf)
{
  FILE *f = fopen(path, "rb");
  const size_t got = f ? fread(buf.data(), 1, buf.size(), f) : 0;
  if (f) fclose(f);
  if (got != buf.size()) fprintf(stderr, "fill_holes: cannot read %zu bytes from %s\n", buf.size(), path);
  return got == buf.size();
}

int main(int argc, char *argv[])
{
  const int w = argc == 8 ? atoi(argv[3]) : 0, h = argc == 8 ? atoi(argv[4]) : 0, ch = argc == 8 ? atoi(argv[5]) : 0, n = argc == 8 ? atoi(argv[6]) : 0;
  if (argc != 8 || w <= 0 || h <= 0 || w > OFC::FILL_MAX_DIM || h > OFC::FILL_MAX_DIM || (ch != 1 && ch != 3) || n < 1 ||
      n > OFC::FILL_MAX_IMAGES) {
    fprintf(stderr, "\n  usage: %s frames.raw holes.raw width height channels(1|3) count out.raw\n\n", argv[0]);
    return 1;
  }
  const size_t px = (size_t)w * h * n, bytes = px * ch;
  std::vector<unsigned char> frames(bytes), holes(px);
  if (!read_all(argv[1], frames) || !read_all(argv[2], holes)) return 1;

  unsigned char *dsrc = nullptr, *dhole = nullptr, *dout = nullptr;
  long long *dstats = nullptr;
  hip_check(hipMalloc((void **)&dsrc, bytes), "hipMalloc");
  hip_check(hipMalloc((void **)&dhole, px), "hipMalloc");
  hip_check(hipMalloc((void **)&dout, bytes), "hipMalloc");
  hip_check(hipMalloc((void **)&dstats, (size_t)n * OFC::FILL_STATS * sizeof(long long)), "hipMalloc");
  hip_check(hipMemcpy(dsrc, frames.data(), bytes, hipMemcpyHostToDevice), "hipMemcpy");
  hip_check(hipMemcpy(dhole, holes.data(), px, hipMemcpyHostToDevice), "hipMemcpy");
  printf("%lld bytes of stream-ordered memory\n", OFC::FillScratchBytes(n, w, h, ch));

  fotg_check(OFC::FillHoles(dsrc, n, w, h, ch, dhole, dout, nullptr, dstats), "fotg_fill_u8");

  std::vector<long long> stats((size_t)n * OFC::FILL_STATS);
  hip_check(hipMemcpy(frames.data(), dout, bytes, hipMemcpyDeviceToHost), "hipMemcpy");
  hip_check(hipMemcpy(stats.data(), dstats, stats.size() * sizeof(long long), hipMemcpyDeviceToHost), "hipMemcpy");
  for (int k = 0; k < n; ++k) {
    const long long *s = &stats[(size_t)k * OFC::FILL_STATS];
    printf("frame %d: %lld known, %lld filled, %lld unfilled, depth %lld\n", k, s[OFC::FILL_N_KNOWN], s[OFC::FILL_N_FILLED],
           s[OFC::FILL_N_UNFILLED], s[OFC::FILL_DEPTH]);
  }
  FILE *f = fopen(argv[7], "wb");
  if (!f || fwrite(frames.data(), 1, bytes, f) != bytes) { fprintf(stderr, "fill_holes: cannot write %s\n", argv[7]); return 1; }
  fclose(f);
  for (void *q : {(void *)dsrc, (void *)dhole, (void *)dout, (void *)dstats}) hip_check(hipFree(q), "hipFree");
  return 0;
}
