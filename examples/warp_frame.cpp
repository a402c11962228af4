// examples/warp_frame.cpp -- motion compensation over the C-ABI and the C++ shims: two raw 8-bit gray frames in, both flows from one
// bidirectional call, the forward-backward consistency mask of frame 0, frame 1 pulled back onto frame 0's grid along the forward
// flow with the occluded / outside / unknown pixels filled, and the mean photometric residual before and after.  Nothing but the
// coarse flows, the mask and the warped frame is written on the GPU: check and warp upsample the flow on the fly.
//
//   hipcc -O2 -Iinclude examples/warp_frame.cpp -Lflowonthego_amd -lfotg -Wl,-rpath,$PWD/flowonthego_amd -o examples/warp_frame
//   examples/warp_frame frame0.raw frame1.raw width height out.png [operating point 1..4] [fill 0..255]
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "fotg/fbcheck.h"
#include "fotg/flowcolor.h"
#include "fotg/warp.h"

static void hip_check(hipError_t e, const char *what)
{
  if (e != hipSuccess) { fprintf(stderr, "%s: %s\n", what, hipGetErrorString(e)); exit(1); }
}

static void fotg_check(int st, const char *what)
{
  if (st != FOTG_OK) { fprintf(stderr, "%s: %s\n", what, fotg_strerror(st)); exit(1); }
}

static bool read_raw(std::vector<unsigned char> &v, const char *path)
{
  FILE *f = fopen(path, "rb");
  if (!f) return false;
  const size_t got = fread(v.data(), 1, v.size(), f);
  fclose(f);
  return got == v.size();
}

int main(int argc, char *argv[])
{
  if (argc < 6 || argc > 8) {
    fprintf(stderr, "\n  usage: %s frame0.raw frame1.raw width height out.png [operating point 1..4] [fill 0..255]\n\n", argv[0]);
    return 1;
  }
  const int w = atoi(argv[3]), h = atoi(argv[4]);
  const int op = argc > 6 ? atoi(argv[6]) : 2;
  const float fill = argc > 7 ? (float)atof(argv[7]) : 0.f;
  if (w <= 0 || h <= 0) { fprintf(stderr, "warp_frame: bad size %s x %s\n", argv[3], argv[4]); return 1; }
  const size_t npix = (size_t)w * h;
  std::vector<unsigned char> f0(npix), f1(npix);
  if (!read_raw(f0, argv[1])) { fprintf(stderr, "warp_frame: cannot read %zu bytes from %s\n", npix, argv[1]); return 1; }
  if (!read_raw(f1, argv[2])) { fprintf(stderr, "warp_frame: cannot read %zu bytes from %s\n", npix, argv[2]); return 1; }

  fotg_params p;
  fotg_check(fotg_op_point(op, w, 1, &p), "fotg_op_point");
  p.bidir = 1;
  fotg_ctx *ctx = nullptr;
  fotg_check(fotg_create(&p, w, h, 0, 1, &ctx), "fotg_create");
  int wl, hl;
  fotg_check(fotg_out_size(ctx, &wl, &hl), "fotg_out_size");

  unsigned char *d0 = nullptr, *d1 = nullptr, *dmask = nullptr, *dwarped = nullptr;
  float *dfw = nullptr, *dbw = nullptr;
  double *dstats = nullptr;
  const size_t flow_bytes = (size_t)wl * hl * 2 * sizeof(float);
  hip_check(hipMalloc((void **)&d0, npix), "hipMalloc");
  hip_check(hipMalloc((void **)&d1, npix), "hipMalloc");
  hip_check(hipMalloc((void **)&dmask, npix), "hipMalloc");
  hip_check(hipMalloc((void **)&dwarped, npix), "hipMalloc");
  hip_check(hipMalloc((void **)&dfw, flow_bytes), "hipMalloc");
  hip_check(hipMalloc((void **)&dbw, flow_bytes), "hipMalloc");
  hip_check(hipMalloc((void **)&dstats, 6 * sizeof(double)), "hipMalloc");
  hip_check(hipMemcpy(d0, f0.data(), npix, hipMemcpyHostToDevice), "hipMemcpy");
  hip_check(hipMemcpy(d1, f1.data(), npix, hipMemcpyHostToDevice), "hipMemcpy");

  // all on the null stream, in order: flows, mask of frame 0, frame 1 warped onto frame 0
  fotg_check(fotg_calc_bidir_u8(ctx, 1, d0, d1, nullptr, nullptr, dfw, dbw, nullptr), "fotg_calc_bidir_u8");
  fotg_check(OFC::UpsampleCropFbCheck(ctx, dfw, dbw, dmask), "fotg_upsample_crop_fb_check");
  fotg_check(OFC::UpsampleCropWarp(ctx, dfw, d1, 1, dwarped, nullptr, dstats, d0, dmask, OFC::WARP_FILL_INVALID, fill),
             "fotg_upsample_crop_warp_u8");

  std::vector<unsigned char> warped(npix), rgb(npix * 3);
  double stats[6];
  hip_check(hipMemcpy(warped.data(), dwarped, npix, hipMemcpyDeviceToHost), "hipMemcpy");
  hip_check(hipMemcpy(stats, dstats, sizeof(stats), hipMemcpyDeviceToHost), "hipMemcpy");
  for (size_t i = 0; i < npix; ++i) rgb[3 * i] = rgb[3 * i + 1] = rgb[3 * i + 2] = warped[i];
  const double valid = stats[OFC::WARP_VALID] > 0 ? stats[OFC::WARP_VALID] : 1;
  printf("valid %.4f  occluded %.4f  outside %.4f  unknown %.4f\n", stats[0] / npix, stats[1] / npix, stats[2] / npix, stats[3] / npix);
  printf("mean |I0 - I1| %.4f  mean |I0 - warp(I1)| %.4f  (over the valid pixels)\n", stats[OFC::WARP_SUM_ABS_UNWARPED] / valid,
         stats[OFC::WARP_SUM_ABS_WARPED] / valid);
  if (!OFC::SavePNG(rgb.data(), w, h, argv[5])) { fprintf(stderr, "SavePNG: cannot write %s\n", argv[5]); return 1; }
  for (void *q : {(void *)d0, (void *)d1, (void *)dmask, (void *)dwarped, (void *)dfw, (void *)dbw, (void *)dstats}) hip_check(hipFree(q), "hipFree");
  fotg_destroy(ctx);
  return 0;
}
