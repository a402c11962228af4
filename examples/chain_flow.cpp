// examples/chain_flow.cpp -- long-range flow over the C-ABI and the C++ shims: T+1 raw 8-bit gray frames in, the flows of the whole
// sequence in both directions from one call, then one launch that follows every pixel of frame 0 through all T flows with an
// occlusion test per step.  Writes the displacement frame 0 -> T as a .flo file and prints how the chains ended.  Nothing but the
// coarse flows and the chain's outputs is written on the GPU: the chain upsamples the flows on the fly.  That is the form that
// needs no memory for full-resolution flows; at 1080p and T = 8 the other route, fotg_upsample_crop of the flows followed by
// fotg_flow_chain on them, measured faster and gives the same bytes.
//
//   hipcc -O2 -Iinclude examples/chain_flow.cpp -Lflowonthego_amd -lfotg -Wl,-rpath,$PWD/flowonthego_amd -o examples/chain_flow
//   examples/chain_flow width height out.flo frame0.raw frame1.raw [frame2.raw ...]
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "fotg/chain.h"
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
  if (argc < 6) {
    fprintf(stderr, "\n  usage: %s width height out.flo frame0.raw frame1.raw [frame2.raw ...]\n\n", argv[0]);
    return 1;
  }
  const int w = atoi(argv[1]), h = atoi(argv[2]), T = argc - 5;
  if (w <= 0 || h <= 0) { fprintf(stderr, "chain_flow: bad size %s x %s\n", argv[1], argv[2]); return 1; }
  const size_t npix = (size_t)w * h;
  std::vector<unsigned char> frames((size_t)(T + 1) * npix);
  for (int k = 0; k <= T; ++k) {
    FILE *f = fopen(argv[4 + k], "rb");
    const size_t got = f ? fread(frames.data() + k * npix, 1, npix, f) : 0;
    if (f) fclose(f);
    if (got != npix) { fprintf(stderr, "chain_flow: cannot read %zu bytes from %s\n", npix, argv[4 + k]); return 1; }
  }

  fotg_params p;
  fotg_check(fotg_op_point(2, w, 1, &p), "fotg_op_point");
  p.bidir = 1;
  fotg_ctx *ctx = nullptr;
  fotg_check(fotg_create(&p, w, h, 0, T, &ctx), "fotg_create");
  int wl, hl;
  fotg_check(fotg_out_size(ctx, &wl, &hl), "fotg_out_size");

  unsigned char *dframes = nullptr, *dcode = nullptr;
  float *dfw = nullptr, *dbw = nullptr, *dtotal = nullptr;
  unsigned long long *dstats = nullptr;
  const size_t flow_bytes = (size_t)T * wl * hl * 2 * sizeof(float);
  hip_check(hipMalloc((void **)&dframes, frames.size()), "hipMalloc");
  hip_check(hipMalloc((void **)&dcode, npix), "hipMalloc");
  hip_check(hipMalloc((void **)&dfw, flow_bytes), "hipMalloc");
  hip_check(hipMalloc((void **)&dbw, flow_bytes), "hipMalloc");
  hip_check(hipMalloc((void **)&dtotal, npix * 2 * sizeof(float)), "hipMalloc");
  hip_check(hipMalloc((void **)&dstats, 5 * sizeof(unsigned long long)), "hipMalloc");
  hip_check(hipMemcpy(dframes, frames.data(), frames.size(), hipMemcpyHostToDevice), "hipMemcpy");

  // all on the null stream, in order: the 2 T flows of the sequence, then the chain over them
  fotg_check(fotg_calc_sequence_bidir_u8(ctx, T + 1, dframes, nullptr, nullptr, dfw, dbw, nullptr), "fotg_calc_sequence_bidir_u8");
  fotg_check(OFC::UpsampleCropFlowChain(ctx, T, dfw, dbw, dtotal, dcode, nullptr, dstats), "fotg_upsample_crop_flow_chain");

  std::vector<float> total(npix * 2);
  unsigned long long stats[5];
  hip_check(hipMemcpy(total.data(), dtotal, total.size() * sizeof(float), hipMemcpyDeviceToHost), "hipMemcpy");
  hip_check(hipMemcpy(stats, dstats, sizeof(stats), hipMemcpyDeviceToHost), "hipMemcpy");
  printf("%d steps: valid %.4f  occluded %.4f  outside %.4f  unknown %.4f  mean steps %.3f\n", T,
         (double)stats[OFC::CHAIN_VALID] / npix, (double)stats[OFC::CHAIN_OCCLUDED] / npix, (double)stats[OFC::CHAIN_OUTSIDE] / npix,
         (double)stats[OFC::CHAIN_UNKNOWN] / npix, (double)stats[OFC::CHAIN_SUM_STEPS] / npix);
  if (!OFC::SaveFlowFile(total.data(), w, h, argv[3])) { fprintf(stderr, "SaveFlowFile: cannot write %s\n", argv[3]); return 1; }
  for (void *q : {(void *)dframes, (void *)dcode, (void *)dfw, (void *)dbw, (void *)dtotal, (void *)dstats}) hip_check(hipFree(q), "hipFree");
  fotg_destroy(ctx);
  return 0;
}
