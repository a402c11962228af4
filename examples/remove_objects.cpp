// examples/remove_objects.cpp -- object removal over the C-ABI and the C++ shim: a file of raw 8-bit gray frames and a file of
// masks (one byte per pixel, non-zero = take this pixel out) in, the frames without the masked objects out.  Two batches of flows --
// frame 0 -> frame k for the plate, frame k -> frame 0 for the removal -- and two fused calls: the median plate in the coordinates
// of frame 0 over the pixels that are not masked, then every frame's mask, grown and feathered, filled from it.  No
// full-resolution flow and no warped plate is ever written.
//
//   hipcc -O2 -Iinclude examples/remove_objects.cpp -Lflowonthego_amd -lfotg -Wl,-rpath,$PWD/flowonthego_amd -o examples/remove_objects
//   examples/remove_objects frames.raw masks.raw width height count out.raw [grow 0..8] [feather 0..8] [operating point 1..4]
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "fotg/erase.h"
#include "fotg/plate.h"

static void hip_check(hipError_t e, const char *what)
{
  if (e != hipSuccess) { fprintf(stderr, "%s: %s\n", what, hipGetErrorString(e)); exit(1); }
}

static void fotg_check(int st, const char *what)
{
  if (st != FOTG_OK) { fprintf(stderr, "%s: %s\n", what, fotg_strerror(st)); exit(1); }
}

static bool read_all(const char *path, std::vector<unsigned char> &buf)
{
  FILE *f = fopen(path, "rb");
  const size_t got = f ? fread(buf.data(), 1, buf.size(), f) : 0;
  if (f) fclose(f);
  if (got != buf.size()) fprintf(stderr, "remove_objects: cannot read %zu bytes from %s\n", buf.size(), path);
  return got == buf.size();
}

int main(int argc, char *argv[])
{
  const int w = argc > 4 ? atoi(argv[3]) : 0, h = argc > 4 ? atoi(argv[4]) : 0, K = argc > 5 ? atoi(argv[5]) : 0;
  const int grow = argc > 7 ? atoi(argv[7]) : 2, feather = argc > 8 ? atoi(argv[8]) : 3, op = argc > 9 ? atoi(argv[9]) : 2;
  if (argc < 7 || argc > 10 || w <= 0 || h <= 0 || K < 2 || K > OFC::PLATE_MAX_FRAMES || grow < 0 || grow > OFC::ERASE_MAX_GROW ||
      feather < 0 || feather > OFC::ERASE_MAX_FEATHER || op < 1 || op > 4) {
    fprintf(stderr, "\n  usage: %s frames.raw masks.raw width height count(2..32) out.raw [grow 0..8] [feather 0..8] [operating point 1..4]\n\n",
            argv[0]);
    return 1;
  }
  const size_t npix = (size_t)w * h;
  std::vector<unsigned char> frames(npix * K), masks(npix * K);
  if (!read_all(argv[1], frames) || !read_all(argv[2], masks)) return 1;

  fotg_params p;
  fotg_check(fotg_op_point(op, w, 1, &p), "fotg_op_point");
  fotg_ctx *ctx = nullptr;
  fotg_check(fotg_create(&p, w, h, 0, K, &ctx), "fotg_create");
  int wl, hl;
  fotg_check(fotg_out_size(ctx, &wl, &hl), "fotg_out_size");

  unsigned char *dframes = nullptr, *dmasks = nullptr, *d0 = nullptr, *dplate = nullptr, *dpcode = nullptr, *dout = nullptr;
  float *dflows = nullptr;
  long long *dstats = nullptr;
  hip_check(hipMalloc((void **)&dframes, npix * K), "hipMalloc");
  hip_check(hipMalloc((void **)&dmasks, npix * K), "hipMalloc");
  hip_check(hipMalloc((void **)&d0, npix * K), "hipMalloc");
  hip_check(hipMalloc((void **)&dplate, npix), "hipMalloc");
  hip_check(hipMalloc((void **)&dpcode, npix), "hipMalloc");
  hip_check(hipMalloc((void **)&dout, npix * K), "hipMalloc");
  hip_check(hipMalloc((void **)&dflows, (size_t)K * wl * hl * 2 * sizeof(float)), "hipMalloc");
  hip_check(hipMalloc((void **)&dstats, (size_t)K * OFC::ERASE_STATS * sizeof(long long)), "hipMalloc");
  hip_check(hipMemcpy(dframes, frames.data(), npix * K, hipMemcpyHostToDevice), "hipMemcpy");
  hip_check(hipMemcpy(dmasks, masks.data(), npix * K, hipMemcpyHostToDevice), "hipMemcpy");

  // all on the null stream, in order: K copies of frame 0, the flows frame 0 -> frame k and the plate along them, the masked
  // pixels of every frame left out of the median
  std::vector<int> index(K);
  for (int k = 0; k < K; ++k) {
    index[k] = k;
    hip_check(hipMemcpyAsync(d0 + k * npix, dframes, npix, hipMemcpyDeviceToDevice, nullptr), "hipMemcpyAsync");
  }
  fotg_check(fotg_calc_batch_u8(ctx, K, d0, dframes, nullptr, dflows, nullptr), "fotg_calc_batch_u8");
  OFC::PlateOptions<unsigned char> po;
  po.code = dpcode;
  po.exclude = dmasks;
  fotg_check(OFC::UpsampleCropBackgroundPlate(ctx, dflows, dframes, K, 1, index.data(), 1, K, dplate, po), "fotg_upsample_crop_plate_u8");

  // the flows frame k -> frame 0 (the plate's call has consumed the others: same stream), then every frame's mask filled from the plate
  fotg_check(fotg_calc_batch_u8(ctx, K, dframes, d0, nullptr, dflows, nullptr), "fotg_calc_batch_u8");
  OFC::ErasePlate<unsigned char> ep;
  ep.plate = dplate; ep.W = w; ep.H = h; ep.code = dpcode;
  OFC::EraseOptions<unsigned char> eo;
  eo.grow = grow; eo.feather = feather; eo.dst = dout; eo.stats = dstats;
  fotg_check(OFC::UpsampleCropRemoveObjects(ctx, dflows, dframes, K, 1, ep, dmasks, eo), "fotg_upsample_crop_erase_u8");

  std::vector<unsigned char> out(npix * K);
  std::vector<long long> stats((size_t)K * OFC::ERASE_STATS);
  hip_check(hipMemcpy(out.data(), dout, out.size(), hipMemcpyDeviceToHost), "hipMemcpy");
  hip_check(hipMemcpy(stats.data(), dstats, stats.size() * sizeof(long long), hipMemcpyDeviceToHost), "hipMemcpy");
  for (int k = 0; k < K; ++k) {
    const long long *s = &stats[(size_t)k * OFC::ERASE_STATS];
    printf("frame %d: masked %.4f  replaced %.4f  blended %.4f  holes %lld (the plate knows nothing there: the object is still visible)\n", k,
           (double)s[OFC::ERASE_N_REMOVE] / npix, (double)s[OFC::ERASE_N_REPLACED] / npix, (double)s[OFC::ERASE_N_BLENDED] / npix,
           s[OFC::ERASE_N_HOLES]);
  }
  FILE *f = fopen(argv[6], "wb");
  if (!f || fwrite(out.data(), 1, out.size(), f) != out.size()) { fprintf(stderr, "remove_objects: cannot write %s\n", argv[6]); return 1; }
  fclose(f);
  for (void *q : {(void *)dframes, (void *)dmasks, (void *)d0, (void *)dplate, (void *)dpcode, (void *)dout, (void *)dflows, (void *)dstats})
    hip_check(hipFree(q), "hipFree");
  fotg_destroy(ctx);
  return 0;
}
