// examples/block_motion.cpp -- block motion vectors for a video encoder over the C++ shim (include/fotg/blockmotion.h): read the raw
// 8-bit gray frame to predict, the raw frame to predict it from and the flow between them as a .flo file; print the sum of the SADs
// of the chosen vectors, that of the zero vector and the PSNR of the prediction, and write one line per block: bx by mvx mvy (in
// quarter pixels) SAD kind.
//
//   hipcc -O2 -Iinclude examples/block_motion.cpp -Lflowonthego_amd -lfotg -Wl,-rpath,$PWD/flowonthego_amd -o examples/block_motion
//   examples/block_motion cur.raw ref.raw flow.flo out.txt [block 8|16|32] [refine 0..3]
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "fotg/blockmotion.h"
#include "fotg/flowcolor.h"

static void hip_check(hipError_t e, const char *what)
{
  if (e != hipSuccess) { fprintf(stderr, "%s: %s\n", what, hipGetErrorString(e)); exit(1); }
}

static void fotg_check(int st, const char *what)
{
  if (st != FOTG_OK) { fprintf(stderr, "%s: %s\n", what, fotg_strerror(st)); exit(1); }
}

static bool read_raw(const char *name, std::vector<unsigned char> &buf)
{
  FILE *f = fopen(name, "rb");
  const size_t got = f ? fread(buf.data(), 1, buf.size(), f) : 0;
  if (f) fclose(f);
  if (got != buf.size()) fprintf(stderr, "block_motion: cannot read %zu bytes from %s\n", buf.size(), name);
  return got == buf.size();
}

int main(int argc, char *argv[])
{
  if (argc < 5 || argc > 7) {
    fprintf(stderr, "\n  usage: %s cur.raw ref.raw flow.flo out.txt [block 8|16|32] [refine 0..3]\n\n", argv[0]);
    return 1;
  }
  const int block = argc > 5 ? atoi(argv[5]) : 16, refine = argc > 6 ? atoi(argv[6]) : 2;
  if (!OFC::BlockMotionValidBlock(block) || refine < 0 || refine > OFC::BLOCKMOTION_MAX_REFINE) {
    fprintf(stderr, "block_motion: bad block or refine\n");
    return 1;
  }
  std::vector<float> flow;
  int w, h, bw, bh;
  if (!OFC::ReadFlowFile(flow, w, h, argv[3])) { fprintf(stderr, "ReadFlowFile: cannot read %s\n", argv[3]); return 1; }
  const size_t npix = (size_t)w * h;
  std::vector<unsigned char> cur(npix), ref(npix);
  if (!read_raw(argv[1], cur) || !read_raw(argv[2], ref)) return 1;
  OFC::BlockMotionGrid(w, h, block, bw, bh);
  const size_t nblk = (size_t)bw * bh;

  float *dflow = nullptr;
  unsigned char *dcur = nullptr, *dref = nullptr, *dkind = nullptr;
  short *dmv = nullptr;
  unsigned *dcost = nullptr;
  long long *dstats = nullptr;
  hip_check(hipMalloc((void **)&dflow, npix * 2 * sizeof(float)), "hipMalloc");
  hip_check(hipMalloc((void **)&dcur, npix), "hipMalloc");
  hip_check(hipMalloc((void **)&dref, npix), "hipMalloc");
  hip_check(hipMalloc((void **)&dmv, nblk * 2 * sizeof(short)), "hipMalloc");
  hip_check(hipMalloc((void **)&dcost, nblk * 2 * sizeof(unsigned)), "hipMalloc");
  hip_check(hipMalloc((void **)&dkind, nblk), "hipMalloc");
  hip_check(hipMalloc((void **)&dstats, OFC::BLOCKMOTION_NSTAT * sizeof(long long)), "hipMalloc");
  hip_check(hipMemcpy(dflow, flow.data(), npix * 2 * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy");
  hip_check(hipMemcpy(dcur, cur.data(), npix, hipMemcpyHostToDevice), "hipMemcpy");
  hip_check(hipMemcpy(dref, ref.data(), npix, hipMemcpyHostToDevice), "hipMemcpy");
  fotg_check(OFC::BlockMotion(dcur, dref, dflow, w, h, 1, 1, dmv, dcost, dkind, nullptr, dstats, nullptr, block, refine),
             "fotg_block_motion");

  std::vector<short> mv(nblk * 2);
  std::vector<unsigned> cost(nblk * 2);
  std::vector<unsigned char> kind(nblk);
  long long stats[OFC::BLOCKMOTION_NSTAT];
  hip_check(hipMemcpy(mv.data(), dmv, mv.size() * sizeof(short), hipMemcpyDeviceToHost), "hipMemcpy");
  hip_check(hipMemcpy(cost.data(), dcost, cost.size() * sizeof(unsigned), hipMemcpyDeviceToHost), "hipMemcpy");
  hip_check(hipMemcpy(kind.data(), dkind, kind.size(), hipMemcpyDeviceToHost), "hipMemcpy");
  hip_check(hipMemcpy(stats, dstats, sizeof(stats), hipMemcpyDeviceToHost), "hipMemcpy");
  const double sse = (double)stats[OFC::BLOCKMOTION_SSE];
  printf("SAD %lld  zero-vector SAD %lld  prediction PSNR %.2f dB\n", stats[OFC::BLOCKMOTION_SAD], stats[OFC::BLOCKMOTION_SAD_ZERO],
         sse > 0 ? 10.0 * std::log10(255.0 * 255.0 * (double)npix / sse) : INFINITY);
  FILE *f = fopen(argv[4], "w");
  if (!f) { fprintf(stderr, "block_motion: cannot write %s\n", argv[4]); return 1; }
  for (size_t b = 0; b < nblk; ++b)
    fprintf(f, "%d %d %d %d %u %d\n", (int)(b % bw), (int)(b / bw), mv[2 * b], mv[2 * b + 1], cost[2 * b], kind[b]);
  fclose(f);
  for (void *q : {(void *)dflow, (void *)dcur, (void *)dref, (void *)dmv, (void *)dcost, (void *)dkind, (void *)dstats})
    hip_check(hipFree(q), "hipFree");
  return 0;
}
