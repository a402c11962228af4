// examples/motion_layers.cpp -- the motion layers of a flow over the C-ABI and the C++ shim: a Middlebury .flo file in, the label
// map (one byte per pixel: the layer, 253 unassigned, 254 masked, 255 unknown) as a binary PGM and the six parameters of every
// layer out.  One call: the seeding of every layer, three refinement rounds and the final pass, all on the device; the host reads
// the labels and a few numbers per layer back.
//
//   hipcc -O2 -Iinclude examples/motion_layers.cpp -Lflowonthego_amd -lfotg -Wl,-rpath,$PWD/flowonthego_amd -o examples/motion_layers
//   examples/motion_layers flow.flo labels.pgm [layers 1..8] [translation|similarity|affine]
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "fotg/layers.h"

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
  int model = OFC::MOTION_AFFINE, K = 3;
  if (argc >= 4) {
    char *end = nullptr;
    const long v = strtol(argv[3], &end, 10);
    K = (*argv[3] && !*end && v >= 1 && v <= OFC::LAYERS_MAX) ? (int)v : -1;
  }
  if (argc == 5) {
    model = -1;
    for (int m = 0; m < 3; ++m)
      if (!strcmp(argv[4], names[m])) model = m;
  }
  if (argc < 3 || argc > 5 || K < 0 || model < 0) {
    fprintf(stderr, "\n  usage: %s flow.flo labels.pgm [layers 1..8] [translation|similarity|affine]\n\n", argv[0]);
    return 1;
  }
  FILE *f = fopen(argv[1], "rb");
  float tag = 0.f;
  int w = 0, h = 0;
  if (!f || fread(&tag, 4, 1, f) != 1 || fread(&w, 4, 1, f) != 1 || fread(&h, 4, 1, f) != 1 || tag != 202021.25f || w < 1 || h < 1 ||
      w > 16384 || h > 16384) {
    fprintf(stderr, "motion_layers: %s is not a .flo file of at most 16384 x 16384\n", argv[1]);
    return 1;
  }
  const size_t npix = (size_t)w * h;
  std::vector<float> flow(npix * 2);
  const size_t got = fread(flow.data(), sizeof(float), flow.size(), f);
  fclose(f);
  if (got != flow.size()) { fprintf(stderr, "motion_layers: %s is truncated\n", argv[1]); return 1; }

  float *dflow = nullptr;
  double *dparams = nullptr;
  unsigned char *dlabels = nullptr;
  long long *drecords = nullptr;
  hip_check(hipMalloc((void **)&dflow, flow.size() * sizeof(float)), "hipMalloc");
  hip_check(hipMalloc((void **)&dparams, (size_t)K * 6 * sizeof(double)), "hipMalloc");
  hip_check(hipMalloc((void **)&dlabels, npix), "hipMalloc");
  hip_check(hipMalloc((void **)&drecords, (size_t)K * 8 * sizeof(long long)), "hipMalloc");
  hip_check(hipMemcpy(dflow, flow.data(), flow.size() * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy");

  fotg_check(OFC::MotionLayers(dflow, nullptr, w, h, K, dparams, model, dlabels, nullptr, drecords), "fotg_motion_layers");

  std::vector<double> p((size_t)K * 6);
  std::vector<long long> rec((size_t)K * 8);
  std::vector<unsigned char> labels(npix);
  hip_check(hipMemcpy(p.data(), dparams, p.size() * sizeof(double), hipMemcpyDeviceToHost), "hipMemcpy");
  hip_check(hipMemcpy(rec.data(), drecords, rec.size() * sizeof(long long), hipMemcpyDeviceToHost), "hipMemcpy");
  hip_check(hipMemcpy(labels.data(), dlabels, npix, hipMemcpyDeviceToHost), "hipMemcpy");
  for (int k = 0; k < K; ++k) {
    const double *q = &p[(size_t)k * 6];
    printf("layer %d: %.9g %.9g %.9g %.9g %.9g %.9g  ", k, q[0], q[1], q[2], q[3], q[4], q[5]);
    if (rec[(size_t)k * 8 + OFC::LAYER_REC_LIVE]) printf("share %.4f\n", (double)rec[(size_t)k * 8 + OFC::LAYER_REC_LABELLED] / npix);
    else printf("dead\n");
  }
  FILE *o = fopen(argv[2], "wb");
  if (!o || fprintf(o, "P5\n%d %d\n255\n", w, h) < 0 || fwrite(labels.data(), 1, npix, o) != npix || fclose(o) != 0) {
    fprintf(stderr, "motion_layers: cannot write %s\n", argv[2]);
    return 1;
  }
  for (void *q : {(void *)dflow, (void *)dparams, (void *)dlabels, (void *)drecords}) hip_check(hipFree(q), "hipFree");
  return 0;
}
