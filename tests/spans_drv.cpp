// A driver of flowonthego_amd/csrc/spans.h for tests/test_host_spans.py: the aliasing rule of the add-on entry points, checked
// against the formula restated here on integers -- false when either pointer is null, otherwise a < b + nb && b < a + na -- and
// against the answer written out per case.  The addresses are made up and never dereferenced.  Exits non-zero on any mismatch.
#include <stdint.h>
#include <stdio.h>
#include "../flowonthego_amd/csrc/spans.h"

using fotg::Span;

namespace {

int failures = 0;

const uintptr_t B = 0x100000;

Span span(uintptr_t p, size_t bytes) { return Span{reinterpret_cast<const void *>(p), bytes}; }

bool formula(uintptr_t a, size_t na, uintptr_t b, size_t nb) { return a != 0 && b != 0 && a < b + nb && b < a + na; }

void check(const char *what, bool got, bool want)
{
  if (got == want) return;
  printf("MISMATCH %s: got %d, want %d\n", what, (int)got, (int)want);
  ++failures;
}

struct Case { const char *name; uintptr_t a; size_t na; uintptr_t b; size_t nb; bool want; };

const Case CASES[] = {
    {"disjoint", B, 16, B + 64, 16, false},
    {"disjoint, b first", B + 64, 16, B, 16, false},
    {"adjacent: a ends where b begins", B, 16, B + 16, 16, false},
    {"adjacent: b ends where a begins", B + 16, 16, B, 16, false},
    {"one byte at a's end", B, 17, B + 16, 16, true},
    {"one byte at a's start", B + 15, 16, B, 16, true},
    {"a inside b", B + 4, 4, B, 16, true},
    {"b inside a", B, 16, B + 4, 4, true},
    {"identical", B, 16, B, 16, true},
    {"null on the left", 0, 16, B, 16, false},
    {"null on the right", B, 16, 0, 16, false},
    {"both null", 0, 16, 0, 16, false},
    {"two zero-length spans at one address", B, 0, B, 0, false},
    {"zero-length a strictly inside b", B + 4, 0, B, 16, true},          // what the formula gives: an empty span inside counts
    {"zero-length b strictly inside a", B, 16, B + 4, 0, true},
    {"zero-length a at b's start", B, 0, B, 16, false},
    {"zero-length a at b's end", B + 16, 0, B, 16, false},
};

}  // namespace

int main()
{
  for (const Case &c : CASES) {
    check(c.name, fotg::overlap(span(c.a, c.na), span(c.b, c.nb)), c.want);
    check(c.name, formula(c.a, c.na, c.b, c.nb), c.want);
  }

  // outputs against inputs: the only hit is the last pair
  {
    const Span out[3] = {span(B, 16), span(0, 16), span(B + 0x100, 16)};
    const Span in[2] = {span(B + 0x200, 16), span(B + 0x10f, 16)};
    check("out/in, last pair only", fotg::overlap_any(out, in), true);
    check("out/in, last pair only: no two outputs", fotg::overlap_among(out), false);
    const Span in_clear[2] = {span(B + 0x200, 16), span(B + 0x110, 16)};
    check("out/in, last pair adjacent", fotg::overlap_any(out, in_clear), false);
  }
  // two outputs overlap each other and no input: only the out/out function reports it
  {
    const Span out[3] = {span(B, 16), span(B + 0x100, 16), span(B + 8, 16)};
    const Span in[2] = {span(B + 0x200, 16), span(0, 1 << 20)};
    check("out/out hit, asked out/in", fotg::overlap_any(out, in), false);
    check("out/out hit, asked out/out", fotg::overlap_among(out), true);
    const Span apart[3] = {span(B, 16), span(B + 0x100, 16), span(B + 16, 16)};
    check("outputs adjacent", fotg::overlap_among(apart), false);
    const Span last_two[3] = {span(B, 16), span(B + 0x100, 16), span(B + 0x10f, 1)};
    check("out/out hit at the last pair only", fotg::overlap_among(last_two), true);
    const Span with_null[2] = {span(0, 16), span(0, 16)};
    check("two outputs that were not given", fotg::overlap_among(with_null), false);
  }
  if (failures) printf("%d mismatches\n", failures);
  return failures ? 1 : 0;
}
