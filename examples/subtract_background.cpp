// examples/subtract_background.cpp -- background subtraction over the C-ABI and the C++ shim: a file of raw 8-bit gray frames in,
// one code map per frame out (0 background, 1 foreground, 2 no plate there, 3 unknown, 4 strong foreground).  Two batches of
// flows -- frame 0 -> frame k for the plate, frame k -> frame 0 for the subtraction -- and two fused calls: the median plate in the
// coordinates of frame 0, then every frame against it.  No full-resolution flow and no warped frame is ever written.
//
//   hipcc -O2 -Iinclude examples/subtract_background.cpp -Lflowonthego_amd -lfotg -Wl,-rpath,$PWD/flowonthego_amd -o examples/subtract_background
//   examples/subtract_background frames.raw width height count out.raw [low] [high] [window 0..2] [operating point 1..4]
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "fotg/plate.h"
#include "fotg/subtract.h"

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
  const int w = argc > 3 ? atoi(argv[2]) : 0, h = argc > 3 ? atoi(argv[3]) : 0, K = argc > 4 ? atoi(argv[4]) : 0;
  const float low = argc > 6 ? (float)atof(argv[6]) : 8.f, high = argc > 7 ? (float)atof(argv[7]) : 24.f;
  const int window = argc > 8 ? atoi(argv[8]) : 1, op = argc > 9 ? atoi(argv[9]) : 2;
  if (argc < 6 || argc > 10 || w <= 0 || h <= 0 || K < 2 || K > OFC::PLATE_MAX_FRAMES || !(low >= 0.f && low <= high && high <= 2047.9375f) ||
      window < 0 || window > OFC::SUBTRACT_MAX_WINDOW || op < 1 || op > 4) {
    fprintf(stderr, "\n  usage: %s frames.raw width height count(2..32) out.raw [low] [high >= low] [window 0..2] [operating point 1..4]\n\n",
            argv[0]);
    return 1;
  }
  const size_t npix = (size_t)w * h;
  std::vector<unsigned char> frames(npix * K);
  FILE *f = fopen(argv[1], "rb");
  const size_t got = f ? fread(frames.data(), 1, frames.size(), f) : 0;
  if (f) fclose(f);
  if (got != frames.size()) { fprintf(stderr, "subtract_background: cannot read %zu bytes from %s\n", frames.size(), argv[1]); return 1; }

  fotg_params p;
  fotg_check(fotg_op_point(op, w, 1, &p), "fotg_op_point");
  fotg_ctx *ctx = nullptr;
  fotg_check(fotg_create(&p, w, h, 0, K, &ctx), "fotg_create");
  int wl, hl;
  fotg_check(fotg_out_size(ctx, &wl, &hl), "fotg_out_size");

  unsigned char *dframes = nullptr, *d0 = nullptr, *dplate = nullptr, *dpcode = nullptr, *dcode = nullptr;
  float *dflows = nullptr;
  long long *dstats = nullptr;
  hip_check(hipMalloc((void **)&dframes, npix * K), "hipMalloc");
  hip_check(hipMalloc((void **)&d0, npix * K), "hipMalloc");
  hip_check(hipMalloc((void **)&dplate, npix), "hipMalloc");
  hip_check(hipMalloc((void **)&dpcode, npix), "hipMalloc");
  hip_check(hipMalloc((void **)&dcode, npix * K), "hipMalloc");
  hip_check(hipMalloc((void **)&dflows, (size_t)K * wl * hl * 2 * sizeof(float)), "hipMalloc");
  hip_check(hipMalloc((void **)&dstats, (size_t)K * OFC::SUBTRACT_STATS * sizeof(long long)), "hipMalloc");
  hip_check(hipMemcpy(dframes, frames.data(), npix * K, hipMemcpyHostToDevice), "hipMemcpy");

  // all on the null stream, in order: K copies of frame 0, the flows frame 0 -> frame k and the plate along them
  std::vector<int> index(K);
  for (int k = 0; k < K; ++k) {
    index[k] = k;
    hip_check(hipMemcpyAsync(d0 + k * npix, dframes, npix, hipMemcpyDeviceToDevice, nullptr), "hipMemcpyAsync");
  }
  fotg_check(fotg_calc_batch_u8(ctx, K, d0, dframes, nullptr, dflows, nullptr), "fotg_calc_batch_u8");
  OFC::PlateOptions<unsigned char> po;
  po.code = dpcode;
  fotg_check(OFC::UpsampleCropBackgroundPlate(ctx, dflows, dframes, K, 1, index.data(), 1, K, dplate, po), "fotg_upsample_crop_plate_u8");

  // the flows frame k -> frame 0 (the plate's call has consumed the others: same stream), then every frame against the plate
  fotg_check(fotg_calc_batch_u8(ctx, K, dframes, d0, nullptr, dflows, nullptr), "fotg_calc_batch_u8");
  OFC::SubtractPlate<unsigned char> sp;
  sp.plate = dplate; sp.W = w; sp.H = h; sp.code = dpcode;
  OFC::SubtractOptions so;
  so.low = low; so.high = high; so.window = window; so.code = dcode; so.stats = dstats;
  fotg_check(OFC::UpsampleCropSubtractBackground(ctx, dflows, dframes, K, 1, sp, so), "fotg_upsample_crop_subtract_u8");

  std::vector<unsigned char> out(npix * K);
  std::vector<long long> stats((size_t)K * OFC::SUBTRACT_STATS);
  hip_check(hipMemcpy(out.data(), dcode, out.size(), hipMemcpyDeviceToHost), "hipMemcpy");
  hip_check(hipMemcpy(stats.data(), dstats, stats.size() * sizeof(long long), hipMemcpyDeviceToHost), "hipMemcpy");
  for (int k = 0; k < K; ++k) {
    const long long *s = &stats[(size_t)k * OFC::SUBTRACT_STATS];
    const long long adm = s[OFC::SUBTRACT_N_BACKGROUND] + s[OFC::SUBTRACT_N_FOREGROUND] + s[OFC::SUBTRACT_N_STRONG];
    printf("frame %d: foreground %.4f  strong %.4f  no plate %.4f  unknown %.4f  mean difference %.3f\n", k,
           (double)(s[OFC::SUBTRACT_N_FOREGROUND] + s[OFC::SUBTRACT_N_STRONG]) / npix, (double)s[OFC::SUBTRACT_N_STRONG] / npix,
           (double)s[OFC::SUBTRACT_N_NO_PLATE] / npix, (double)s[OFC::SUBTRACT_N_UNKNOWN] / npix,
           adm ? s[OFC::SUBTRACT_SUM_DIFF] / 16.0 / adm : 0.0);
  }
  f = fopen(argv[5], "wb");
  if (!f || fwrite(out.data(), 1, out.size(), f) != out.size()) { fprintf(stderr, "subtract_background: cannot write %s\n", argv[5]); return 1; }
  fclose(f);
  for (void *q : {(void *)dframes, (void *)d0, (void *)dplate, (void *)dpcode, (void *)dcode, (void *)dflows, (void *)dstats})
    hip_check(hipFree(q), "hipFree");
  fotg_destroy(ctx);
  return 0;
}
