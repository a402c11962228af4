// examples/background_plate.cpp -- a clean plate over the C-ABI and the C++ shim: a file of raw 8-bit gray frames in, the median over
// the frames in the coordinates of frame 0 out.  One batch of flows frame 0 -> frame k, one fused call that upsamples the coarse
// flows on the fly, gathers the K samples of every pixel and selects their median on chip; no full-resolution flow and no warped
// frame is ever written.  (For a panning shot chain the camera motions instead and call OFC::BackgroundPlateMotion on a canvas.)
//
//   hipcc -O2 -Iinclude examples/background_plate.cpp -Lflowonthego_amd -lfotg -Wl,-rpath,$PWD/flowonthego_amd -o examples/background_plate
//   examples/background_plate frames.raw width height count out.raw [min_count] [mean] [operating point 1..4]
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "fotg/plate.h"

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
  const int min_count = argc > 6 ? atoi(argv[6]) : 1;
  const bool mean = argc > 7 && !strcmp(argv[7], "mean");
  const int op = argc > 8 ? atoi(argv[8]) : 2;
  if (argc < 6 || argc > 9 || w <= 0 || h <= 0 || K < 1 || K > OFC::PLATE_MAX_FRAMES || min_count < 1 || min_count > K ||
      (argc > 7 && !mean && strcmp(argv[7], "median")) || op < 1 || op > 4) {
    fprintf(stderr, "\n  usage: %s frames.raw width height count(1..32) out.raw [min_count 1..count] [median|mean] [operating point 1..4]\n\n",
            argv[0]);
    return 1;
  }
  const size_t npix = (size_t)w * h;
  std::vector<unsigned char> frames(npix * K);
  FILE *f = fopen(argv[1], "rb");
  const size_t got = f ? fread(frames.data(), 1, frames.size(), f) : 0;
  if (f) fclose(f);
  if (got != frames.size()) { fprintf(stderr, "background_plate: cannot read %zu bytes from %s\n", frames.size(), argv[1]); return 1; }

  fotg_params p;
  fotg_check(fotg_op_point(op, w, 1, &p), "fotg_op_point");
  fotg_ctx *ctx = nullptr;
  fotg_check(fotg_create(&p, w, h, 0, K, &ctx), "fotg_create");
  int wl, hl;
  fotg_check(fotg_out_size(ctx, &wl, &hl), "fotg_out_size");

  unsigned char *dframes = nullptr, *d0 = nullptr, *dout = nullptr, *dcode = nullptr;
  float *dflows = nullptr;
  double *dstats = nullptr;
  hip_check(hipMalloc((void **)&dframes, npix * K), "hipMalloc");
  hip_check(hipMalloc((void **)&d0, npix * K), "hipMalloc");
  hip_check(hipMalloc((void **)&dout, npix), "hipMalloc");
  hip_check(hipMalloc((void **)&dcode, npix), "hipMalloc");
  hip_check(hipMalloc((void **)&dflows, (size_t)K * wl * hl * 2 * sizeof(float)), "hipMalloc");
  hip_check(hipMalloc((void **)&dstats, OFC::PLATE_STATS * sizeof(double)), "hipMalloc");
  hip_check(hipMemcpy(dframes, frames.data(), npix * K, hipMemcpyHostToDevice), "hipMemcpy");

  // all on the null stream, in order: the flows frame 0 -> frame k (k = 0 is the zero flow of a frame onto itself), then the plate
  std::vector<int> index(K);
  for (int k = 0; k < K; ++k) {
    index[k] = k;
    hip_check(hipMemcpyAsync(d0 + k * npix, dframes, npix, hipMemcpyDeviceToDevice, nullptr), "hipMemcpyAsync");
  }
  fotg_check(fotg_calc_batch_u8(ctx, K, d0, dframes, nullptr, dflows, nullptr), "fotg_calc_batch_u8");
  OFC::PlateOptions<unsigned char> o;
  o.code = dcode;
  o.stats = dstats;
  o.mode = mean ? OFC::PLATE_MEAN : OFC::PLATE_MEDIAN;
  o.min_count = min_count;
  fotg_check(OFC::UpsampleCropBackgroundPlate(ctx, dflows, dframes, K, 1, index.data(), 1, K, dout, o), "fotg_upsample_crop_plate_u8");

  std::vector<unsigned char> out(npix);
  double stats[OFC::PLATE_STATS];
  hip_check(hipMemcpy(out.data(), dout, npix, hipMemcpyDeviceToHost), "hipMemcpy");
  hip_check(hipMemcpy(stats, dstats, sizeof(stats), hipMemcpyDeviceToHost), "hipMemcpy");
  printf("estimated %.4f  hidden %.4f  uncovered %.4f  frames per pixel %.3f of %d\n", stats[OFC::PLATE_N_ESTIMATED] / npix,
         stats[OFC::PLATE_N_HIDDEN] / npix, stats[OFC::PLATE_N_UNCOVERED] / npix, stats[OFC::PLATE_SUM_COUNT] / npix, K);
  f = fopen(argv[5], "wb");
  if (!f || fwrite(out.data(), 1, out.size(), f) != out.size()) { fprintf(stderr, "background_plate: cannot write %s\n", argv[5]); return 1; }
  fclose(f);
  for (void *q : {(void *)dframes, (void *)d0, (void *)dout, (void *)dcode, (void *)dflows, (void *)dstats}) hip_check(hipFree(q), "hipFree");
  fotg_destroy(ctx);
  return 0;
}
