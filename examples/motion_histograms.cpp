// examples/motion_histograms.cpp -- a flow turned into features over the C-ABI and the C++ shims: a Middlebury .flo file in, the
// image's HOF, MBHx and MBHy out, with and without the affine camera motion subtracted.  The motion fit and the histograms per cell
// run on the device; the host reads the cells back and adds them up.
//
//   hipcc -O2 -Iinclude examples/motion_histograms.cpp -Lflowonthego_amd -lfotg -Wl,-rpath,$PWD/flowonthego_amd -o examples/motion_histograms
//   examples/motion_histograms flow.flo [cell]
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "fotg/histograms.h"
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
  const int cell = argc == 3 ? atoi(argv[2]) : 16;
  if (argc < 2 || argc > 3 || (cell != 8 && cell != 16 && cell != 32)) {
    fprintf(stderr, "\n  usage: %s flow.flo [cell = 8 | 16 | 32]\n\n", argv[0]);
    return 1;
  }
  FILE *f = fopen(argv[1], "rb");
  float tag = 0.f;
  int w = 0, h = 0;
  if (!f || fread(&tag, 4, 1, f) != 1 || fread(&w, 4, 1, f) != 1 || fread(&h, 4, 1, f) != 1 || tag != 202021.25f || w < 1 || h < 1 ||
      w > 16384 || h > 16384) {
    fprintf(stderr, "motion_histograms: %s is not a .flo file of at most 16384 x 16384\n", argv[1]);
    return 1;
  }
  std::vector<float> flow((size_t)w * h * 2);
  const size_t got = fread(flow.data(), sizeof(float), flow.size(), f);
  fclose(f);
  if (got != flow.size()) { fprintf(stderr, "motion_histograms: %s is truncated\n", argv[1]); return 1; }

  const size_t ncell = (size_t)OFC::HistCells(h, cell) * OFC::HistCells(w, cell);
  float *dflow = nullptr;
  double *dparams = nullptr;
  long long *dcells = nullptr;
  hip_check(hipMalloc((void **)&dflow, flow.size() * sizeof(float)), "hipMalloc");
  hip_check(hipMalloc((void **)&dparams, 6 * sizeof(double)), "hipMalloc");
  hip_check(hipMalloc((void **)&dcells, ncell * OFC::HIST_FIELDS * sizeof(long long)), "hipMalloc");
  hip_check(hipMemcpy(dflow, flow.data(), flow.size() * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy");
  fotg_check(OFC::FitMotion(dflow, nullptr, w, h, dparams), "fotg_fit_motion");

  std::vector<long long> cells(ncell * OFC::HIST_FIELDS);
  for (int pass = 0; pass < 2; ++pass) {
    fotg_check(OFC::MotionHistograms(dflow, w, h, dcells, cell, nullptr, nullptr, 256, nullptr, pass ? dparams : nullptr), "fotg_motion_histograms");
    hip_check(hipMemcpy(cells.data(), dcells, cells.size() * sizeof(long long), hipMemcpyDeviceToHost), "hipMemcpy");
    long long sum[OFC::HIST_FIELDS] = {0};
    for (size_t c = 0; c < ncell; ++c)
      for (int k = 0; k < OFC::HIST_FIELDS; ++k) sum[k] += cells[c * OFC::HIST_FIELDS + k];
    printf("%s\n", pass ? "camera motion subtracted:" : "as it is:");
    const int parts[3] = {OFC::HIST_HOF, OFC::HIST_MBHX, OFC::HIST_MBHY};
    static const char *const names[3] = {"HOF ", "MBHx", "MBHy"};
    for (int p = 0; p < 3; ++p) {
      printf("  %s", names[p]);
      for (int k = 0; k < OFC::HIST_BINS; ++k) printf(" %lld", sum[parts[p] + k]);
      printf("\n");
    }
    printf("  zero bin %lld of %lld admissible pixels (%.4f), %lld not admissible, %zu cells of %d\n", sum[OFC::HIST_ZERO], sum[OFC::HIST_N],
           sum[OFC::HIST_N] ? (double)sum[OFC::HIST_ZERO] / (double)sum[OFC::HIST_N] : 0.0, sum[OFC::HIST_N_BAD], ncell, cell);
  }
  for (void *q : {(void *)dflow, (void *)dparams, (void *)dcells}) hip_check(hipFree(q), "hipFree");
  return 0;
}
