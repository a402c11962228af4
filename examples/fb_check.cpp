// examples/fb_check.cpp -- forward-backward consistency of two .flo files over the C++ shim (include/fotg/fbcheck.h): read the
// flow frame 0 -> 1 and the flow frame 1 -> 0, check them on the GPU, write frame 0's mask as a PNG (consistent white, occluded
// red, outside the frame blue, unknown black) and print the fraction of each code.
//
//   hipcc -O2 -Iinclude examples/fb_check.cpp -Lflowonthego_amd -lfotg -Wl,-rpath,$PWD/flowonthego_amd -o examples/fb_check
//   examples/fb_check fw.flo bw.flo out.png [alpha1 alpha2]
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "fotg/fbcheck.h"
#include "fotg/flowcolor.h"

static void hip_check(hipError_t e, const char *what)
{
  if (e != hipSuccess) { fprintf(stderr, "%s: %s\n", what, hipGetErrorString(e)); exit(1); }
}

int main(int argc, char *argv[])
{
  if (argc != 4 && argc != 6) { fprintf(stderr, "\n  usage: %s fw.flo bw.flo out.png [alpha1 alpha2]\n\n", argv[0]); return 1; }
  const float alpha1 = argc == 6 ? (float)atof(argv[4]) : 0.01f, alpha2 = argc == 6 ? (float)atof(argv[5]) : 0.5f;
  std::vector<float> fw, bw;
  int w, h, wb, hb;
  if (!OFC::ReadFlowFile(fw, w, h, argv[1])) { fprintf(stderr, "ReadFlowFile: cannot read %s\n", argv[1]); return 1; }
  if (!OFC::ReadFlowFile(bw, wb, hb, argv[2])) { fprintf(stderr, "ReadFlowFile: cannot read %s\n", argv[2]); return 1; }
  if (w != wb || h != hb) { fprintf(stderr, "fb_check: the two flows differ in size\n"); return 1; }
  const size_t npix = (size_t)w * h;
  float *dfw = nullptr, *dbw = nullptr;
  unsigned char *dmask = nullptr;
  unsigned *dcounts = nullptr;
  hip_check(hipMalloc((void **)&dfw, fw.size() * sizeof(float)), "hipMalloc");
  hip_check(hipMalloc((void **)&dbw, bw.size() * sizeof(float)), "hipMalloc");
  hip_check(hipMalloc((void **)&dmask, npix), "hipMalloc");
  hip_check(hipMalloc((void **)&dcounts, 8 * sizeof(unsigned)), "hipMalloc");
  hip_check(hipMemcpy(dfw, fw.data(), fw.size() * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy");
  hip_check(hipMemcpy(dbw, bw.data(), bw.size() * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy");
  const int st = OFC::FbCheck(dfw, dbw, w, h, dmask, nullptr, dcounts, alpha1, alpha2);
  if (st != FOTG_OK) { fprintf(stderr, "fotg_fb_check: %s\n", fotg_strerror(st)); return 1; }
  std::vector<unsigned char> mask(npix), rgb(npix * 3);
  unsigned counts[8];
  hip_check(hipMemcpy(mask.data(), dmask, npix, hipMemcpyDeviceToHost), "hipMemcpy");
  hip_check(hipMemcpy(counts, dcounts, sizeof(counts), hipMemcpyDeviceToHost), "hipMemcpy");
  static const unsigned char palette[4][3] = {{255, 255, 255}, {255, 0, 0}, {0, 0, 255}, {0, 0, 0}};
  for (size_t i = 0; i < npix; ++i)
    for (int c = 0; c < 3; ++c) rgb[3 * i + c] = palette[mask[i] & 3][c];
  printf("consistent %.4f  occluded %.4f  outside %.4f  unknown %.4f\n", (double)counts[0] / npix, (double)counts[1] / npix,
         (double)counts[2] / npix, (double)counts[3] / npix);
  if (!OFC::SavePNG(rgb.data(), w, h, argv[3])) { fprintf(stderr, "SavePNG: cannot write %s\n", argv[3]); return 1; }
  hip_check(hipFree(dfw), "hipFree");
  hip_check(hipFree(dbw), "hipFree");
  hip_check(hipFree(dmask), "hipFree");
  hip_check(hipFree(dcounts), "hipFree");
  return 0;
}
