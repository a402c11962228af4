// examples/track_objects.cpp -- the moving objects of a sequence of flows, tracked, over the C-ABI and the C++ shims: the Middlebury
// .flo files of consecutive frame pairs in (flow t: frame t -> t + 1, all of one size), one line per track out.  Per flow the motion
// fit with its per-pixel code and residual and the connected components of code 1 with their ids, batched over the sequence; then
// the overlap votes, the links and the tracks (OFC::TrackObjects); the host reads the counts and the track table back.
//
//   hipcc -O2 -Iinclude examples/track_objects.cpp -Lflowonthego_amd -lfotg -Wl,-rpath,$PWD/flowonthego_amd -o examples/track_objects
//   examples/track_objects flow0.flo flow1.flo [flow2.flo ...]
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "fotg/motion.h"
#include "fotg/objects.h"
#include "fotg/tracks.h"

static void hip_check(hipError_t e, const char *what)
{
  if (e != hipSuccess) { fprintf(stderr, "%s: %s\n", what, hipGetErrorString(e)); exit(1); }
}

static void fotg_check(int st, const char *what)
{
  if (st != FOTG_OK) { fprintf(stderr, "%s: %s\n", what, fotg_strerror(st)); exit(1); }
}

template <class T>
static T *dev_alloc(size_t count)
{
  T *p = nullptr;
  hip_check(hipMalloc((void **)&p, count * sizeof(T)), "hipMalloc");
  return p;
}

int main(int argc, char *argv[])
{
  const int K = 256, max_tracks = 1024, frames = argc - 1, T = frames - 1;
  const long long min_area = 64;
  if (frames < 2) {
    fprintf(stderr, "\n  usage: %s flow0.flo flow1.flo [flow2.flo ...]\n\n", argv[0]);
    return 1;
  }
  int w = 0, h = 0;
  std::vector<float> flow;
  for (int t = 0; t < frames; ++t) {
    FILE *f = fopen(argv[1 + t], "rb");
    float tag = 0.f;
    int wt = 0, ht = 0;
    if (!f || fread(&tag, 4, 1, f) != 1 || fread(&wt, 4, 1, f) != 1 || fread(&ht, 4, 1, f) != 1 || tag != 202021.25f || wt < 1 || ht < 1 ||
        wt > 16384 || ht > 16384 || (t > 0 && (wt != w || ht != h))) {
      fprintf(stderr, "track_objects: %s is not a .flo file of at most 16384 x 16384 and of the first one's size\n", argv[1 + t]);
      return 1;
    }
    w = wt; h = ht;
    const size_t count = (size_t)w * h * 2;
    flow.resize((size_t)(t + 1) * count);
    const size_t got = fread(flow.data() + (size_t)t * count, sizeof(float), count, f);
    fclose(f);
    if (got != count) { fprintf(stderr, "track_objects: %s is truncated\n", argv[1 + t]); return 1; }
  }
  const size_t npix = (size_t)frames * w * h;

  float *dflow = dev_alloc<float>(npix * 2), *dres = dev_alloc<float>(npix * 2);
  unsigned char *dcode = dev_alloc<unsigned char>(npix);
  double *dparams = dev_alloc<double>((size_t)frames * 6);
  int *dids = dev_alloc<int>(npix), *dvotes = dev_alloc<int>((size_t)T * K * K);
  int *dab = dev_alloc<int>((size_t)T * K * OFC::LINK_FIELDS), *dba = dev_alloc<int>((size_t)T * K * OFC::LINK_FIELDS);
  int *dtrack = dev_alloc<int>((size_t)frames * K);
  long long *dobj = dev_alloc<long long>((size_t)frames * K * OFC::OBJECT_FIELDS), *dsent = dev_alloc<long long>((size_t)T * K * OFC::SENT_FIELDS);
  long long *dtracks = dev_alloc<long long>((size_t)max_tracks * OFC::TRACK_FIELDS), *dstats = dev_alloc<long long>(4);
  hip_check(hipMemcpy(dflow, flow.data(), flow.size() * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy");

  fotg_check(OFC::FitMotion(dflow, nullptr, w, h, dparams, OFC::MOTION_AFFINE, dcode, dres, nullptr, nullptr, 3, 1.0f, frames), "fotg_fit_motion");
  fotg_check(OFC::LabelComponents(dcode, w, h, dobj, K, dres, min_area, 1 << OFC::MOTION_INDEPENDENT, 8, nullptr, dids, nullptr, frames),
             "fotg_label_components");
  fotg_check(OFC::TrackObjects(dids, dobj, dflow, w, h, T, K, dvotes, dsent, dab, dba, dtrack, dtracks, max_tracks, dstats), "OFC::TrackObjects");

  long long st[4];
  std::vector<long long> tracks((size_t)max_tracks * OFC::TRACK_FIELDS);
  hip_check(hipMemcpy(st, dstats, sizeof(st), hipMemcpyDeviceToHost), "hipMemcpy");
  hip_check(hipMemcpy(tracks.data(), dtracks, tracks.size() * sizeof(long long), hipMemcpyDeviceToHost), "hipMemcpy");
  static const char *const ends[] = {"alive", "threshold", "merged", "lost"};
  for (long long k = 0; k < st[OFC::TRACKS_RECORDED]; ++k) {
    const long long *r = tracks.data() + k * OFC::TRACK_FIELDS;
    const long long len = r[OFC::TRACK_LAST_FRAME] - r[OFC::TRACK_FIRST_FRAME] + 1;
    printf("%lld  frames %lld .. %lld  rows %lld %lld  mean area %.1f  largest %lld  votes %lld  %s\n", k, r[OFC::TRACK_FIRST_FRAME],
           r[OFC::TRACK_LAST_FRAME], r[OFC::TRACK_FIRST_ROW], r[OFC::TRACK_LAST_ROW], (double)r[OFC::TRACK_SUM_AREA] / (double)len,
           r[OFC::TRACK_MAX_AREA], r[OFC::TRACK_SUM_VOTES], ends[r[OFC::TRACK_END] & 3]);
  }
  printf("%lld tracks over %d object maps (%lld links, %lld alive at the end)\n", st[OFC::TRACKS_STARTED], frames, st[OFC::TRACKS_LINKS],
         st[OFC::TRACKS_ALIVE]);
  for (void *q : {(void *)dflow, (void *)dres, (void *)dcode, (void *)dparams, (void *)dids, (void *)dvotes, (void *)dab, (void *)dba,
                  (void *)dtrack, (void *)dobj, (void *)dsent, (void *)dtracks, (void *)dstats})
    hip_check(hipFree(q), "hipFree");
  return 0;
}
