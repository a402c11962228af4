// examples/interp_frame.cpp -- frame-rate up-conversion over the C-ABI and the C++ shims: two raw 8-bit gray frames in, both flows
// from one bidirectional call, the frame at time t between them out.  Nothing but the coarse flows and the new frame is written to
// the caller's memory: the consistency check and the interpolation upsample the flows on the fly.
//
//   hipcc -O2 -Iinclude examples/interp_frame.cpp -Lflowonthego_amd -lfotg -Wl,-rpath,$PWD/flowonthego_amd -o examples/interp_frame
//   examples/interp_frame frame0.raw frame1.raw width height out.png [t 0..1, default 0.5] [operating point 1..4]
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "fotg/flowcolor.h"
#include "fotg/interp.h"

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
    fprintf(stderr, "\n  usage: %s frame0.raw frame1.raw width height out.png [t, default 0.5] [operating point 1..4]\n\n", argv[0]);
    return 1;
  }
  const int w = atoi(argv[3]), h = atoi(argv[4]);
  const float t = argc > 6 ? (float)atof(argv[6]) : 0.5f;
  const int op = argc > 7 ? atoi(argv[7]) : 2;
  if (w <= 0 || h <= 0) { fprintf(stderr, "interp_frame: bad size %s x %s\n", argv[3], argv[4]); return 1; }
  if (!(t > 0.f && t < 1.f)) { fprintf(stderr, "interp_frame: t must lie strictly between 0 and 1\n"); return 1; }
  const size_t npix = (size_t)w * h;
  std::vector<unsigned char> f0(npix), f1(npix);
  if (!read_raw(f0, argv[1])) { fprintf(stderr, "interp_frame: cannot read %zu bytes from %s\n", npix, argv[1]); return 1; }
  if (!read_raw(f1, argv[2])) { fprintf(stderr, "interp_frame: cannot read %zu bytes from %s\n", npix, argv[2]); return 1; }

  fotg_params p;
  fotg_check(fotg_op_point(op, w, 1, &p), "fotg_op_point");
  p.bidir = 1;
  fotg_ctx *ctx = nullptr;
  fotg_check(fotg_create(&p, w, h, 0, 1, &ctx), "fotg_create");
  int wl, hl;
  fotg_check(fotg_out_size(ctx, &wl, &hl), "fotg_out_size");

  unsigned char *d0 = nullptr, *d1 = nullptr, *dout = nullptr;
  float *dfw = nullptr, *dbw = nullptr;
  double *dstats = nullptr;
  const size_t flow_bytes = (size_t)wl * hl * 2 * sizeof(float);
  hip_check(hipMalloc((void **)&d0, npix), "hipMalloc");
  hip_check(hipMalloc((void **)&d1, npix), "hipMalloc");
  hip_check(hipMalloc((void **)&dout, npix), "hipMalloc");
  hip_check(hipMalloc((void **)&dfw, flow_bytes), "hipMalloc");
  hip_check(hipMalloc((void **)&dbw, flow_bytes), "hipMalloc");
  hip_check(hipMalloc((void **)&dstats, 6 * sizeof(double)), "hipMalloc");
  hip_check(hipMemcpy(d0, f0.data(), npix, hipMemcpyHostToDevice), "hipMemcpy");
  hip_check(hipMemcpy(d1, f1.data(), npix, hipMemcpyHostToDevice), "hipMemcpy");

  // all on the null stream, in order: both flows, then check + interpolation in one call
  fotg_check(fotg_calc_bidir_u8(ctx, 1, d0, d1, nullptr, nullptr, dfw, dbw, nullptr), "fotg_calc_bidir_u8");
  fotg_check(OFC::UpsampleCropInterpolate(ctx, dfw, dbw, d0, d1, 1, t, dout, nullptr, dstats), "fotg_upsample_crop_interp_u8");

  std::vector<unsigned char> out(npix), rgb(npix * 3);
  double stats[6];
  hip_check(hipMemcpy(out.data(), dout, npix, hipMemcpyDeviceToHost), "hipMemcpy");
  hip_check(hipMemcpy(stats, dstats, sizeof(stats), hipMemcpyDeviceToHost), "hipMemcpy");
  for (size_t i = 0; i < npix; ++i) rgb[3 * i] = rgb[3 * i + 1] = rgb[3 * i + 2] = out[i];
  printf("t %.4f  from_forward %.4f  from_backward %.4f  holes %.4f  one_sided %.4f\n", t, stats[OFC::INTERP_N_FORWARD] / npix,
         stats[OFC::INTERP_N_BACKWARD] / npix, stats[OFC::INTERP_N_HOLES] / npix, stats[OFC::INTERP_N_ONE_SIDED] / npix);
  if (!OFC::SavePNG(rgb.data(), w, h, argv[5])) { fprintf(stderr, "SavePNG: cannot write %s\n", argv[5]); return 1; }
  for (void *q : {(void *)d0, (void *)d1, (void *)dout, (void *)dfw, (void *)dbw, (void *)dstats}) hip_check(hipFree(q), "hipFree");
  fotg_destroy(ctx);
  return 0;
}
