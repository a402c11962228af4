// tests/fill_levels_drv.cpp -- a stand-alone check of flowonthego_amd/csrc/fill_levels.h (plain C++, built with g++ and the address
// and undefined-behaviour sanitizers by tests/test_host_fill.py): for every w, h in 1 .. 130 and for 16384 against each of them, and
// ch in 1 .. 3, the level sizes equal the recurrence w_{l+1} = (w_l + 1) >> 1 restated here, L is the first level of size 1 x 1, the
// parts of an image's memory lie in order, at multiples of 16 bytes, without overlap and inside `bytes`, each as large as the
// definition says, and the chunk and the bytes of a call follow their rule.  Exits non-zero at the first mismatch.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../flowonthego_amd/csrc/fill_levels.h"

using namespace fotg;

static int fails = 0;
#define CHECK(cond) \
  do { \
    if (!(cond)) { \
      printf("w %d h %d ch %d: %s (line %d)\n", w, h, ch, #cond, __LINE__); \
      if (++fails > 20) exit(1); \
    } \
  } while (0)

struct Part { long long at, bytes; };

static void check(int w, int h, int ch)
{
  const FillLevels g = fill_levels(w, h, ch);
  // the recurrence
  std::vector<int> lw(1, w), lh(1, h);
  while (lw.back() > 1 || lh.back() > 1) {
    lw.push_back((lw.back() + 1) >> 1);
    lh.push_back((lh.back() + 1) >> 1);
  }
  const int L = (int)lw.size() - 1;
  CHECK(g.L == L && g.L <= FILL_MAX_LEVEL && g.top == (L > 6 ? L : 6) && g.w == w && g.h == h && g.ch == ch);
  for (int l = 0; l <= FILL_MAX_LEVEL + 1; ++l) {
    CHECK(fill_dim(w, l) == (l <= L ? lw[l] : 1));
    CHECK(fill_dim(h, l) == (l <= L ? lh[l] : 1));
  }
  CHECK(g.tw == fill_dim(w, 6) && g.th == fill_dim(h, 6) && g.tw == (w + 63) / 64 && g.th == (h + 63) / 64);
  // the parts, in order
  std::vector<Part> parts;
  for (int l = 1; l <= 5; ++l) {
    const long long pw = fill_plane_dim(g.tw, l), ph = fill_plane_dim(g.th, l);
    CHECK(pw == (long long)g.tw * (64 >> l) && ph == (long long)g.th * (64 >> l) && pw >= fill_dim(w, l) && ph >= fill_dim(h, l));
    parts.push_back({g.mean[l], pw * ph * ch * 4});
  }
  parts.push_back({g.dep, (long long)g.tw * g.th * 4});
  for (int l = 6; l <= g.top; ++l) {
    const long long blocks = (long long)fill_dim(w, l) * fill_dim(h, l);
    parts.push_back({g.sum[l], blocks * ch * 8});
    parts.push_back({g.cnt[l], blocks * 4});
    parts.push_back({g.val[l], blocks * ch * 4});
  }
  parts.push_back({g.flags, FILL_NFLAG * 4});
  long long end = 0, used = 0;
  for (const Part &p : parts) {
    CHECK(p.at % 16 == 0 && p.at >= end && p.at < end + 16 && p.bytes > 0);
    end = p.at + p.bytes;
    used += p.bytes;
  }
  CHECK(parts[0].at == 0 && g.bytes >= end && g.bytes < end + 256 && g.bytes % 256 == 0 && used <= g.bytes);
  // a call
  const int ns[] = {1, 2, 7, 64, 4096, 65535};
  for (int n : ns) {
    const int chunk = fill_chunk(n, g.bytes);
    CHECK(chunk >= 1 && chunk <= n);
    CHECK(chunk == n || (long long)(chunk + 1) * g.bytes > FILL_SCRATCH_CAP);
    CHECK(chunk == 1 || (long long)chunk * g.bytes <= FILL_SCRATCH_CAP);
    CHECK(fill_scratch_bytes(n, w, h, ch) == (long long)chunk * g.bytes);
  }
}

int main()
{
  for (int ch = 1; ch <= 3; ++ch) {
    for (int w = 1; w <= 130; ++w)
      for (int h = 1; h <= 130; ++h) check(w, h, ch);
    for (int v = 1; v <= 130; ++v) { check(16384, v, ch); check(v, 16384, ch); }
    check(16384, 16384, ch);
    check(1920, 1080, ch);
  }
  {
    const int w = 16384, h = 16384, ch = 3;
    const FillLevels g = fill_levels(w, h, ch);
    CHECK(g.L == 14 && g.tw == 256 && g.th == 256 && g.bytes > FILL_SCRATCH_CAP && fill_chunk(65535, g.bytes) == 1);
  }
  if (fails) return 1;
  printf("fill_levels ok\n");
  return 0;
}
