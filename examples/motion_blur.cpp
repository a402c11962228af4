// examples/motion_blur.cpp -- a shutter simulated along a flow over the C-ABI and the C++ shim: a Middlebury .flo file in, a
// synthetic 8-bit checkerboard of the flow's size blurred along it on the device, the blurred frame out as a binary PGM, and the
// statistics of the call on the terminal.
//
//   hipcc -O2 -Iinclude examples/motion_blur.cpp -Lflowonthego_amd -lfotg -Wl,-rpath,$PWD/flowonthego_amd -o examples/motion_blur
//   examples/motion_blur flow.flo out.pgm [shutter [max_blur]]
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "fotg/blur.h"

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
  const double shutter = argc >= 4 ? atof(argv[3]) : 0.5;
  const int max_blur = argc >= 5 ? atoi(argv[4]) : OFC::BLUR_MAX;
  const int shutter256 = (int)(256.0 * shutter + 0.5);
  if (argc < 3 || argc > 5 || !(shutter > 0.0 && shutter <= 2.0) || shutter256 < 1 || max_blur < 1 || max_blur > OFC::BLUR_MAX) {
    fprintf(stderr, "\n  usage: %s flow.flo out.pgm [shutter in (0, 2] = 0.5 [max_blur in 1 .. 32 = 32]]\n\n", argv[0]);
    return 1;
  }
  FILE *f = fopen(argv[1], "rb");
  float tag = 0.f;
  int w = 0, h = 0;
  if (!f || fread(&tag, 4, 1, f) != 1 || fread(&w, 4, 1, f) != 1 || fread(&h, 4, 1, f) != 1 || tag != 202021.25f || w < 1 || h < 1 ||
      w > 16384 || h > 16384) {
    fprintf(stderr, "motion_blur: %s is not a .flo file of at most 16384 x 16384\n", argv[1]);
    return 1;
  }
  std::vector<float> flow((size_t)w * h * 2);
  const size_t got = fread(flow.data(), sizeof(float), flow.size(), f);
  fclose(f);
  if (got != flow.size()) { fprintf(stderr, "motion_blur: %s is truncated\n", argv[1]); return 1; }

  std::vector<unsigned char> frame((size_t)w * h);
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) frame[(size_t)y * w + x] = ((x / 8 + y / 8) & 1) ? 230 : 25;

  float *dflow = nullptr;
  unsigned char *dsrc = nullptr, *ddst = nullptr;
  long long *dstats = nullptr;
  hip_check(hipMalloc((void **)&dflow, flow.size() * sizeof(float)), "hipMalloc");
  hip_check(hipMalloc((void **)&dsrc, frame.size()), "hipMalloc");
  hip_check(hipMalloc((void **)&ddst, frame.size()), "hipMalloc");
  hip_check(hipMalloc((void **)&dstats, OFC::BLUR_STATS * sizeof(long long)), "hipMalloc");
  hip_check(hipMemcpy(dflow, flow.data(), flow.size() * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy");
  hip_check(hipMemcpy(dsrc, frame.data(), frame.size(), hipMemcpyHostToDevice), "hipMemcpy");
  fotg_check(OFC::MotionBlur(dsrc, dflow, w, h, 1, ddst, shutter256, max_blur, nullptr, nullptr, nullptr, dstats), "fotg_motion_blur");
  long long st[OFC::BLUR_STATS];
  hip_check(hipMemcpy(frame.data(), ddst, frame.size(), hipMemcpyDeviceToHost), "hipMemcpy");
  hip_check(hipMemcpy(st, dstats, sizeof(st), hipMemcpyDeviceToHost), "hipMemcpy");

  FILE *o = fopen(argv[2], "wb");
  if (!o || fprintf(o, "P5\n%d %d\n255\n", w, h) < 0 || fwrite(frame.data(), 1, frame.size(), o) != frame.size()) {
    fprintf(stderr, "motion_blur: cannot write %s\n", argv[2]);
    return 1;
  }
  fclose(o);
  const double px = (double)w * h;
  printf("untouched %.4f  blurred %.4f  clamped %.4f  unknown %.4f  taps per pixel %.3f  copy tiles %lld  longest half-streak %.4f px\n",
         st[OFC::BLUR_N_UNTOUCHED] / px, st[OFC::BLUR_N_BLURRED] / px, st[OFC::BLUR_N_CLAMPED] / px, st[OFC::BLUR_N_UNKNOWN] / px,
         st[OFC::BLUR_TAPS] / px, st[OFC::BLUR_COPY_TILES], st[OFC::BLUR_MAX_LEN] / 16.0);
  for (void *q : {(void *)dflow, (void *)dsrc, (void *)ddst, (void *)dstats}) hip_check(hipFree(q), "hipFree");
  return 0;
}
