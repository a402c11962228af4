// examples/color_flow.cpp -- the reference's flow_code/C color_flow tool over the C++ shim (include/fotg/flowcolor.h): read a .flo,
// upload it, colour it on the GPU, write a PNG; the same arguments and the same printed lines.
//
//   hipcc -O2 -Iinclude examples/color_flow.cpp -Lflowonthego_amd -lfotg -Wl,-rpath,$PWD/flowonthego_amd -o examples/color_flow
//   examples/color_flow [-quiet] in.flo out.png [maxmotion]
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "fotg/flowcolor.h"

static const char *usage = "\n  usage: %s [-quiet] in.flo out.png [maxmotion]\n";

static void hip_check(hipError_t e, const char *what)
{
  if (e != hipSuccess) { fprintf(stderr, "%s: %s\n", what, hipGetErrorString(e)); exit(1); }
}

int main(int argc, char *argv[])
{
  int argn = 1, verbose = 1;
  if (argc > 1 && argv[1][0] == '-' && argv[1][1] == 'q') { verbose = 0; argn++; }
  if (!(argn >= argc - 3 && argn <= argc - 2)) { fprintf(stderr, usage, argv[0]); fprintf(stderr, "\n"); return 1; }
  const char *flowname = argv[argn++], *outname = argv[argn++];
  const float maxmotion = argn < argc ? (float)atof(argv[argn++]) : -1;
  std::vector<float> flow;
  int w, h;
  if (!OFC::ReadFlowFile(flow, w, h, flowname)) { fprintf(stderr, "ReadFlowFile: cannot read %s\n", flowname); return 1; }
  float *dflow = nullptr, *dstats = nullptr;
  unsigned char *drgb = nullptr;
  hip_check(hipMalloc((void **)&dflow, flow.size() * sizeof(float)), "hipMalloc");
  hip_check(hipMalloc((void **)&drgb, (size_t)w * h * 3), "hipMalloc");
  hip_check(hipMalloc((void **)&dstats, 5 * sizeof(float)), "hipMalloc");
  hip_check(hipMemcpy(dflow, flow.data(), flow.size() * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy");
  const int st = OFC::MotionToColor(dflow, w, h, drgb, maxmotion, dstats);
  if (st != FOTG_OK) { fprintf(stderr, "fotg_flow_color: %s\n", fotg_strerror(st)); return 1; }
  std::vector<unsigned char> rgb((size_t)w * h * 3);
  float s[5];
  hip_check(hipMemcpy(rgb.data(), drgb, rgb.size(), hipMemcpyDeviceToHost), "hipMemcpy");
  hip_check(hipMemcpy(s, dstats, sizeof(s), hipMemcpyDeviceToHost), "hipMemcpy");
  printf("max motion: %.4f  motion range: u = %.3f .. %.3f;  v = %.3f .. %.3f\n", s[0], s[1], s[2], s[3], s[4]);
  fflush(stdout);
  float maxrad = maxmotion > 0 ? maxmotion : s[0];
  if (maxrad == 0) maxrad = 1;
  if (verbose) {
    fprintf(stderr, "normalizing by %g\n", maxrad);
    fprintf(stderr, "Writing image %s\n", outname);
  }
  if (!OFC::SavePNG(rgb.data(), w, h, outname)) { fprintf(stderr, "SavePNG: cannot write %s\n", outname); return 1; }
  hip_check(hipFree(dflow), "hipFree");
  hip_check(hipFree(drgb), "hipFree");
  hip_check(hipFree(dstats), "hipFree");
  return 0;
}
