// examples/moving_objects.cpp -- the moving objects of a flow over the C-ABI and the C++ shims: a Middlebury .flo file in, the
// camera motion and one line per object out (box, area, centroid, mean motion relative to the camera).  Two calls: the motion fit
// with its per-pixel code and residual, then the connected components of code 1 with the residual as values; the host reads the
// six parameters, four counts and the written rows back.
//
//   hipcc -O2 -Iinclude examples/moving_objects.cpp -Lflowonthego_amd -lfotg -Wl,-rpath,$PWD/flowonthego_amd -o examples/moving_objects
//   examples/moving_objects flow.flo [min_area]
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "fotg/motion.h"
#include "fotg/objects.h"

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
  const int max_objects = 256;
  long long min_area = 64;
  if (argc == 3) min_area = atoll(argv[2]);
  if (argc < 2 || argc > 3 || min_area < 1) {
    fprintf(stderr, "\n  usage: %s flow.flo [min_area]\n\n", argv[0]);
    return 1;
  }
  FILE *f = fopen(argv[1], "rb");
  float tag = 0.f;
  int w = 0, h = 0;
  if (!f || fread(&tag, 4, 1, f) != 1 || fread(&w, 4, 1, f) != 1 || fread(&h, 4, 1, f) != 1 || tag != 202021.25f || w < 1 || h < 1 ||
      w > 16384 || h > 16384) {
    fprintf(stderr, "moving_objects: %s is not a .flo file of at most 16384 x 16384\n", argv[1]);
    return 1;
  }
  const size_t npix = (size_t)w * h;
  std::vector<float> flow(npix * 2);
  const size_t got = fread(flow.data(), sizeof(float), flow.size(), f);
  fclose(f);
  if (got != flow.size()) { fprintf(stderr, "moving_objects: %s is truncated\n", argv[1]); return 1; }

  float *dflow = nullptr, *dres = nullptr;
  unsigned char *dcode = nullptr;
  double *dparams = nullptr;
  long long *dobj = nullptr, *dstats = nullptr;
  hip_check(hipMalloc((void **)&dflow, flow.size() * sizeof(float)), "hipMalloc");
  hip_check(hipMalloc((void **)&dres, flow.size() * sizeof(float)), "hipMalloc");
  hip_check(hipMalloc((void **)&dcode, npix), "hipMalloc");
  hip_check(hipMalloc((void **)&dparams, 6 * sizeof(double)), "hipMalloc");
  hip_check(hipMalloc((void **)&dobj, max_objects * OFC::OBJECT_FIELDS * sizeof(long long)), "hipMalloc");
  hip_check(hipMalloc((void **)&dstats, 4 * sizeof(long long)), "hipMalloc");
  hip_check(hipMemcpy(dflow, flow.data(), flow.size() * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy");

  fotg_check(OFC::FitMotion(dflow, nullptr, w, h, dparams, OFC::MOTION_AFFINE, dcode, dres), "fotg_fit_motion");
  fotg_check(OFC::LabelComponents(dcode, w, h, dobj, max_objects, dres, min_area, 1 << OFC::MOTION_INDEPENDENT, 8, nullptr, nullptr, dstats),
             "fotg_label_components");

  double p[6];
  long long st[4];
  std::vector<long long> obj((size_t)max_objects * OFC::OBJECT_FIELDS);
  hip_check(hipMemcpy(p, dparams, sizeof(p), hipMemcpyDeviceToHost), "hipMemcpy");
  hip_check(hipMemcpy(st, dstats, sizeof(st), hipMemcpyDeviceToHost), "hipMemcpy");
  hip_check(hipMemcpy(obj.data(), dobj, obj.size() * sizeof(long long), hipMemcpyDeviceToHost), "hipMemcpy");
  printf("%.9g %.9g %.9g %.9g %.9g %.9g\n", p[0], p[1], p[2], p[3], p[4], p[5]);
  for (long long r = 0; r < st[OFC::OBJECTS_WRITTEN]; ++r) {
    const long long *o = obj.data() + r * OFC::OBJECT_FIELDS;
    const double a = (double)o[OFC::OBJECT_AREA], nv = 256.0 * (double)o[OFC::OBJECT_N_VAL];
    printf("%lld %lld %lld %lld  area %lld  centroid %.2f %.2f  motion %.3f %.3f\n", o[OFC::OBJECT_XMIN], o[OFC::OBJECT_YMIN],
           o[OFC::OBJECT_XMAX], o[OFC::OBJECT_YMAX], o[OFC::OBJECT_AREA], o[OFC::OBJECT_SUM_X] / a, o[OFC::OBJECT_SUM_Y] / a,
           o[OFC::OBJECT_SUM_U] / nv, o[OFC::OBJECT_SUM_V] / nv);
  }
  printf("%lld objects of at least %lld pixels (%lld components, %lld pixels)\n", st[OFC::OBJECTS_KEPT], min_area,
         st[OFC::OBJECTS_COMPONENTS], st[OFC::OBJECTS_FOREGROUND]);
  for (void *q : {(void *)dflow, (void *)dres, (void *)dcode, (void *)dparams, (void *)dobj, (void *)dstats}) hip_check(hipFree(q), "hipFree");
  return 0;
}
