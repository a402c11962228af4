// examples/fit_motion.cpp -- the camera motion of a flow over the C-ABI and the C++ shim: a Middlebury .flo file in, the six
// parameters of the fitted motion (u = a00 x + a01 y + tx, v = a10 x + a11 y + ty) and the share of the pixels that follow it out.
// One call: four passes over the flow (plain least squares, then three rounds on the pixels within 1 px of the previous motion) and
// a final pass for the counts, all on the device; the host reads twelve numbers back.
//
//   hipcc -O2 -Iinclude examples/fit_motion.cpp -Lflowonthego_amd -lfotg -Wl,-rpath,$PWD/flowonthego_amd -o examples/fit_motion
//   examples/fit_motion flow.flo [translation|similarity|affine]
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "fotg/motion.h"

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
  static const char *names[3] = {"translation", "similarity", "affine"};
  int model = OFC::MOTION_AFFINE;
  if (argc == 3) {
    model = -1;
    for (int m = 0; m < 3; ++m)
      if (!strcmp(argv[2], names[m])) model = m;
  }
  if (argc < 2 || argc > 3 || model < 0) {
    fprintf(stderr, "\n  usage: %s flow.flo [translation|similarity|affine]\n\n", argv[0]);
    return 1;
  }
  FILE *f = fopen(argv[1], "rb");
  float tag = 0.f;
  int w = 0, h = 0;
  if (!f || fread(&tag, 4, 1, f) != 1 || fread(&w, 4, 1, f) != 1 || fread(&h, 4, 1, f) != 1 || tag != 202021.25f || w < 1 || h < 1 ||
      w > 16384 || h > 16384) {
    fprintf(stderr, "fit_motion: %s is not a .flo file of at most 16384 x 16384\n", argv[1]);
    return 1;
  }
  const size_t npix = (size_t)w * h;
  std::vector<float> flow(npix * 2);
  const size_t got = fread(flow.data(), sizeof(float), flow.size(), f);
  fclose(f);
  if (got != flow.size()) { fprintf(stderr, "fit_motion: %s is truncated\n", argv[1]); return 1; }

  float *dflow = nullptr;
  double *dparams = nullptr;
  long long *dstats = nullptr;
  hip_check(hipMalloc((void **)&dflow, flow.size() * sizeof(float)), "hipMalloc");
  hip_check(hipMalloc((void **)&dparams, 6 * sizeof(double)), "hipMalloc");
  hip_check(hipMalloc((void **)&dstats, 6 * sizeof(long long)), "hipMalloc");
  hip_check(hipMemcpy(dflow, flow.data(), flow.size() * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy");

  fotg_check(OFC::FitMotion(dflow, nullptr, w, h, dparams, model, nullptr, nullptr, dstats), "fotg_fit_motion");

  double p[6];
  long long st[6];
  hip_check(hipMemcpy(p, dparams, sizeof(p), hipMemcpyDeviceToHost), "hipMemcpy");
  hip_check(hipMemcpy(st, dstats, sizeof(st), hipMemcpyDeviceToHost), "hipMemcpy");
  printf("%.9g %.9g %.9g %.9g %.9g %.9g\n", p[0], p[1], p[2], p[3], p[4], p[5]);
  printf("%s: follows %.4f%s\n", names[model], (double)st[OFC::MOTION_FOLLOWS] / npix, st[OFC::MOTION_FITTED] ? "" : "  (not fitted)");
  for (void *q : {(void *)dflow, (void *)dparams, (void *)dstats}) hip_check(hipFree(q), "hipFree");
  return 0;
}
