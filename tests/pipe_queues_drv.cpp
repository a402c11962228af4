// A driver of flowonthego_amd/csrc/pipe_queues.h and of PipeBook::outstanding (pipe_tickets.h) for tests/test_host_pipe_queues.py:
// the placement rule of a pipe's slot streams as the pure function it is.  Built with g++ into the test's temporary directory
// and loaded through ctypes.
#include "../flowonthego_amd/csrc/pipe_queues.h"
#include "../flowonthego_amd/csrc/pipe_tickets.h"

extern "C" {
int drv_max_depth() { return FOTG_PIPE_MAX_DEPTH; }
int drv_parse_mode(const char *s) { return fotg_queues::parse_mode(s); }
int drv_auto_layout(int budget, int depth) { return fotg_queues::auto_layout(budget, depth); }
// cls[depth] = the class of every slot (0 normal, 1 high, 2 low), prio[depth] = its stream priority; returns layout | shared << 8
int drv_place(int layout, int budget, int depth, int prio_least, int prio_greatest, int *cls, int *prio)
{
  const fotg_queues::Plan pl = fotg_queues::place(layout, budget, depth, prio_least, prio_greatest);
  for (int k = 0; k < depth; ++k) {
    cls[k] = pl.cls[k];
    prio[k] = fotg_queues::priority_of(pl.cls[k], prio_least, prio_greatest);
  }
  return pl.layout | (pl.shared ? 256 : 0);
}
int drv_fallback_order(int first, int *out) { return fotg_queues::fallback_order(first, out); }

// a book of `depth` slots after `nsubmit` submits of which the tickets in settle[0..nsettle) were host-waited (stall words clear)
int drv_outstanding(int depth, int nsubmit, const long *settle, int nsettle)
{
  fotg_tickets::PipeBook book(depth);
  for (int i = 0; i < nsubmit; ++i) book.submit(true);
  for (int i = 0; i < nsettle; ++i)
    book.verify(settle[i], 1, [](int) { return FOTG_OK; }, [](long) { return FOTG_OK; });
  return book.outstanding() ? 1 : 0;
}
}
