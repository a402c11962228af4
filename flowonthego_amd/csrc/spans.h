// spans.h -- "does an output of a call alias an input, or another output", in plain C++ (no HIP): every aliasing rule the add-on
// entry points (fotg_<feature>.hip) promise is decided here, on the host, before the device is touched.
// tests/spans_drv.cpp builds this header with g++ for tests/test_host_spans.py.
// (static: each file keeps its own copy, as it did when these were pasted per file; libfotg.so exports none of them.)
#pragma once
#include <stddef.h>

namespace fotg {

struct Span { const void *p; size_t bytes; };       // p == nullptr: an optional argument that was not given

// a span that was not given overlaps nothing
static inline bool overlap(const Span &a, const Span &b)
{
  if (!a.p || !b.p) return false;
  const char *x = static_cast<const char *>(a.p), *y = static_cast<const char *>(b.p);
  return x < y + b.bytes && y < x + a.bytes;
}

// does any span of `out` overlap any span of `in`
template <size_t NO, size_t NI>
static bool overlap_any(const Span (&out)[NO], const Span (&in)[NI])
{
  for (const Span &o : out)
    for (const Span &i : in)
      if (overlap(o, i)) return true;
  return false;
}

// do any two spans of `out` overlap each other
template <size_t NO>
static bool overlap_among(const Span (&out)[NO])
{
  for (size_t i = 0; i < NO; ++i)
    for (size_t j = i + 1; j < NO; ++j)
      if (overlap(out[i], out[j])) return true;
  return false;
}

}  // namespace fotg
