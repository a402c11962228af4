// examples/filter_flow.cpp -- edge- and occlusion-aware filtering of a .flo file over the C++ shim (include/fotg/flowfilter.h): read
// the flow frame 0 -> 1, the raw 8-bit gray frame 0 as guide and, optionally, the flow frame 1 -> 0; with the backward flow the
// forward-backward check runs first and the vectors it rejects are filled from their neighbours.  Writes the filtered flow and
// prints the share of each code and the mean change.
//
//   hipcc -O2 -Iinclude examples/filter_flow.cpp -Lflowonthego_amd -lfotg -Wl,-rpath,$PWD/flowonthego_amd -o examples/filter_flow
//   examples/filter_flow fw.flo frame0.raw out.flo [bw.flo | -] [radius 1..7] [tau] [iters 1..4]
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "fotg/fbcheck.h"
#include "fotg/flowcolor.h"
#include "fotg/flowfilter.h"
#include "fotg/flowio.h"

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
  if (argc < 4 || argc > 8) {
    fprintf(stderr, "\n  usage: %s fw.flo frame0.raw out.flo [bw.flo | -] [radius 1..7] [tau] [iters 1..4]\n\n", argv[0]);
    return 1;
  }
  const char *bw_name = argc > 4 && strcmp(argv[4], "-") != 0 ? argv[4] : nullptr;
  const int radius = argc > 5 ? atoi(argv[5]) : 3;
  const float tau = argc > 6 ? (float)atof(argv[6]) : 20.f;
  const int iters = argc > 7 ? atoi(argv[7]) : 2;
  if (radius < 1 || radius > OFC::FLOWFILTER_MAX_RADIUS || !(tau > 0.f) || iters < 1 || iters > OFC::FLOWFILTER_MAX_ITERS) {
    fprintf(stderr, "filter_flow: bad radius, tau or iters\n");
    return 1;
  }
  std::vector<float> fw, bw;
  int w, h, wb, hb;
  if (!OFC::ReadFlowFile(fw, w, h, argv[1])) { fprintf(stderr, "ReadFlowFile: cannot read %s\n", argv[1]); return 1; }
  if (bw_name && (!OFC::ReadFlowFile(bw, wb, hb, bw_name) || wb != w || hb != h)) {
    fprintf(stderr, "filter_flow: cannot read %s, or it differs in size\n", bw_name);
    return 1;
  }
  const size_t npix = (size_t)w * h;
  std::vector<unsigned char> guide(npix);
  FILE *f = fopen(argv[2], "rb");
  const size_t got = f ? fread(guide.data(), 1, npix, f) : 0;
  if (f) fclose(f);
  if (got != npix) { fprintf(stderr, "filter_flow: cannot read %zu bytes from %s\n", npix, argv[2]); return 1; }

  float *dfw = nullptr, *dbw = nullptr, *dout = nullptr;
  unsigned char *dguide = nullptr, *dmask = nullptr;
  double *dstats = nullptr;
  hip_check(hipMalloc((void **)&dfw, npix * 2 * sizeof(float)), "hipMalloc");
  hip_check(hipMalloc((void **)&dout, npix * 2 * sizeof(float)), "hipMalloc");
  hip_check(hipMalloc((void **)&dguide, npix), "hipMalloc");
  hip_check(hipMalloc((void **)&dstats, 4 * sizeof(double)), "hipMalloc");
  hip_check(hipMemcpy(dfw, fw.data(), npix * 2 * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy");
  hip_check(hipMemcpy(dguide, guide.data(), npix, hipMemcpyHostToDevice), "hipMemcpy");
  if (bw_name) {                                                            // the mask of frame 0
    hip_check(hipMalloc((void **)&dbw, npix * 2 * sizeof(float)), "hipMalloc");
    hip_check(hipMalloc((void **)&dmask, npix), "hipMalloc");
    hip_check(hipMemcpy(dbw, bw.data(), npix * 2 * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy");
    fotg_check(OFC::FbCheck(dfw, dbw, w, h, dmask), "fotg_fb_check");
  }
  float spatial[OFC::FLOWFILTER_MAX_RADIUS + 1];
  OFC::FlowFilterSpatialTable(radius, radius / 2.0, spatial);
  fotg_check(OFC::FlowFilter(dfw, dguide, w, h, 1, 1, dout, nullptr, dstats, dmask, radius, spatial, tau, iters), "fotg_flow_filter_u8");

  std::vector<float> out(npix * 2);
  double stats[4];
  hip_check(hipMemcpy(out.data(), dout, out.size() * sizeof(float), hipMemcpyDeviceToHost), "hipMemcpy");
  hip_check(hipMemcpy(stats, dstats, sizeof(stats), hipMemcpyDeviceToHost), "hipMemcpy");
  printf("filtered %.4f  filled %.4f  unsupported %.4f  mean change %.4f px\n", stats[OFC::FLOWFILTER_N_FILTERED] / npix,
         stats[OFC::FLOWFILTER_N_FILLED] / npix, stats[OFC::FLOWFILTER_N_UNSUPPORTED] / npix,
         stats[OFC::FLOWFILTER_SUM_ABS_CHANGE] / (stats[OFC::FLOWFILTER_N_FILTERED] > 0 ? 2.0 * stats[OFC::FLOWFILTER_N_FILTERED] : 1.0));
  if (!OFC::SaveFlowFile(out.data(), w, h, argv[3])) { fprintf(stderr, "SaveFlowFile: cannot write %s\n", argv[3]); return 1; }
  for (void *q : {(void *)dfw, (void *)dbw, (void *)dout, (void *)dguide, (void *)dmask, (void *)dstats})
    if (q) hip_check(hipFree(q), "hipFree");
  return 0;
}
