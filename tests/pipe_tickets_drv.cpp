// A driver of flowonthego_amd/csrc/pipe_tickets.h for tests/test_pipe_tickets.py: the pipe's bookkeeping with the HIP side
// scripted -- each slot's stall word is a bool the test sets, and a recompute is logged and reports a stall again for the tickets
// the test names.  Built with g++ into the test's temporary directory and loaded through ctypes.
#include <set>
#include <vector>
#include "../flowonthego_amd/csrc/pipe_tickets.h"

namespace {
struct Drv {
  explicit Drv(int depth) : book(depth), flag(depth, false) {}
  fotg_tickets::PipeBook book;
  std::vector<bool> flag;
  std::set<long> fails;                 // tickets whose recompute stalls again
  std::vector<long> recomputed;         // recompute requests since the last drv_recomputed
  fotg_tickets::JobBook<16> jobs;

  int take_flag(int k)
  {
    if (!flag[k]) return FOTG_OK;
    flag[k] = false;
    return FOTG_ERR_STALL;
  }
  int recompute(long u)
  {
    recomputed.push_back(u);
    return fails.count(u) ? FOTG_ERR_STALL : FOTG_OK;
  }
};
}  // namespace

extern "C" {
void *drv_new(int depth) { return depth >= 1 && depth <= FOTG_PIPE_MAX_DEPTH ? new Drv(depth) : nullptr; }
void drv_free(void *d) { delete (Drv *)d; }

long drv_submit(void *d, int no_recompute) { return ((Drv *)d)->book.submit(!no_recompute); }

// fotg_pipe_wait(host_wait = 0) / fotg_pipe_ticket_event
int drv_hand_out(void *d, long t)
{
  Drv &r = *(Drv *)d;
  if (!r.book.valid(t)) return FOTG_ERR_ARG;
  r.book.hand_out(t);
  return FOTG_OK;
}

void drv_inject_stall(void *d, int k) { ((Drv *)d)->flag[k] = true; }
void drv_fail_recompute(void *d, long u) { ((Drv *)d)->fails.insert(u); }

// fotg_pipe_wait(host_wait = m), m = 1 or 2
int drv_wait(void *d, long t, int m)
{
  Drv &r = *(Drv *)d;
  if (!r.book.valid(t)) return FOTG_ERR_ARG;
  return r.book.verify(t, m != 2, [&](int k) { return r.take_flag(k); }, [&](long u) { return r.recompute(u); });
}

int drv_sync(void *d)
{
  Drv &r = *(Drv *)d;
  return r.book.sync([&](int k) { return r.take_flag(k); }, [&](long u) { return r.recompute(u); });
}

// the recompute requests since the last call (up to cap of them into out); returns how many there were
int drv_recomputed(void *d, long *out, int cap)
{
  Drv &r = *(Drv *)d;
  const int n = (int)r.recomputed.size();
  for (int i = 0; i < n && i < cap; ++i) out[i] = r.recomputed[i];
  r.recomputed.clear();
  return n;
}

// the number of disjoint ranges in slot k's set of stalled tickets that have left the ring
int drv_lost_ranges(void *d, int k) { return (int)((Drv *)d)->book.lost[k].ranges(); }

// fotg_node_wait's per-job status
void drv_job_record(void *d, long job, int st) { ((Drv *)d)->jobs.record(job, st); }
int drv_job_status(void *d, long job) { return ((Drv *)d)->jobs.status_of(job); }
}
