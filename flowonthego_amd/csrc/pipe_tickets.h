// pipe_tickets.h -- the stall / recompute bookkeeping of a fotg_pipe and the per-job status of a fotg_node, in plain C++ (no HIP):
// which tickets are suspects when a context's stall word is found set, which of them may be recomputed, and what every later host
// wait for a ticket reports.  fotg_capi.hip / fotg_node.hip keep every HIP call (synchronisation, the recompute itself, events) and
// ask this header what to do; tests/pipe_tickets_drv.cpp builds it with g++ and tests/test_pipe_tickets.py drives it against the
// reference model of the contract (tests/pipe_model.py).
//
// The contract (include/fotg.h, RECOMPUTE CONTRACT above fotg_pipe_wait): ticket t runs on slot t % depth.  A host wait for t
// settles every unsettled ticket of that slot -- all of them good if the slot's stall word is clear, otherwise every one submitted
// so far a suspect: recomputed and good where its buffers are still in place, stalled where they are not (or its recompute stalls
// again).  A settled ticket's verdict never changes: a stalled ticket reports FOTG_ERR_STALL from every later host wait, a good
// one never does, however many tickets follow.
#pragma once
#include <algorithm>
#include <vector>
#include "../../include/fotg.h"

namespace fotg_tickets {

// a set of integers as sorted, disjoint, non-adjacent half-open ranges [lo, hi): grows by at most one range per add
class RangeSet {
 public:
  void add(long lo, long hi)
  {
    if (lo >= hi) return;
    // the first range that overlaps or touches [lo, hi), and every later one that does: merged into one
    auto first = std::lower_bound(r_.begin(), r_.end(), lo, [](const Range &a, long v) { return a.hi < v; });
    auto last = first;
    for (; last != r_.end() && last->lo <= hi; ++last) { lo = std::min(lo, last->lo); hi = std::max(hi, last->hi); }
    first = r_.erase(first, last);
    r_.insert(first, Range{lo, hi});
  }
  bool has(long x) const
  {
    auto it = std::upper_bound(r_.begin(), r_.end(), x, [](long v, const Range &a) { return v < a.hi; });
    return it != r_.end() && it->lo <= x;
  }
  size_t ranges() const { return r_.size(); }

 private:
  struct Range { long lo, hi; };
  std::vector<Range> r_;
};

// per-ticket and per-slot state of one pipe.  Every member function is called with the pipe's mutex held.
struct PipeBook {
  enum : signed char { UNVERIFIED = 0, GOOD = 1, STALLED = 2 };
  int depth = 1, nring = 4;                                 // nring = 4 * depth: the tickets the ring describes
  long submitted = 0;
  signed char verdict[4 * FOTG_PIPE_MAX_DEPTH] = {};       // per ring entry (ticket u at u % nring, for u >= submitted - nring)
  bool healable[4 * FOTG_PIPE_MAX_DEPTH] = {};             // its buffers are still in place: it may be recomputed
  long verified[FOTG_PIPE_MAX_DEPTH] = {};                 // per slot: the slot's tickets below this one are settled
  // per slot, in units of the slot's own tickets (u / depth): the STALLED tickets that have left the ring -- suspects that were already
  // out of it when the flag was found, and stalled ring entries folded in when a submit reuses their entry.  Disjoint ranges, not
  // one hull: a good ticket between two stalls stays good.
  RangeSet lost[FOTG_PIPE_MAX_DEPTH];

  explicit PipeBook(int depth_ = 1) : depth(depth_), nring(4 * depth_) {}

  bool valid(long t) const { return t >= 0 && t < submitted; }
  bool in_ring(long u) const { return u >= submitted - nring; }
  int slot(long u) const { return (int)(u % depth); }

  // a submitted ticket that no host wait has settled yet (its batch may still be running)
  bool outstanding() const
  {
    for (int k = 0; k < depth && k < submitted; ++k) {
      const long last = submitted - 1 - (submitted - 1 - k) % depth;      // the slot's last ticket
      if (last >= verified[k]) return true;
    }
    return false;
  }

  // the ticket of the next submission; its ring entry is the one of ticket - nring, which is folded into its slot's lost set first
  // if it was stalled (its verdict must outlive the entry)
  long submit(bool healable_)
  {
    const long t = submitted;
    const int e = (int)(t % nring);
    if (t >= nring && verdict[e] == STALLED) {
      const long old = t - nring;
      lost[slot(old)].add(old / depth, old / depth + 1);
    }
    verdict[e] = UNVERIFIED;
    healable[e] = healable_;
    ++submitted;
    return t;
  }

  // fotg_pipe_wait(host_wait = 0) / fotg_pipe_ticket_event: the caller may free or reuse the buffers once ITS wait is over
  void hand_out(long t) { if (in_ring(t)) healable[t % nring] = false; }

  // status of a settled ticket
  int status(long u) const
  {
    if (in_ring(u)) return verdict[u % nring] == STALLED ? FOTG_ERR_STALL : FOTG_OK;
    return lost[slot(u)].has(u / depth) ? FOTG_ERR_STALL : FOTG_OK;
  }

  // A host wait for ticket t (valid, and the host has synchronised with it): settle the slot's tickets and return t's status.
  //   take_flag(k)  FOTG_OK: slot k's stall word is clear; FOTG_ERR_STALL: it was set, and the caller has synchronised the slot and
  //                 cleared it; anything else: an error, returned as it is
  //   recompute(u)  recompute ticket u from its own arguments: FOTG_OK, FOTG_ERR_STALL (stalled again) or an error (returned as it is)
  // heal = 0 (host_wait = 2): suspects are reported, never recomputed.  newly_stalled counts the tickets this call marks stalled.
  template <class TakeFlag, class Recompute>
  int verify(long t, int heal, TakeFlag take_flag, Recompute recompute, int *newly_stalled = nullptr)
  {
    const int k = slot(t);
    if (t < verified[k]) return status(t);
    const int flag = take_flag(k);
    if (flag == FOTG_OK) {
      // everything of this slot that has completed so far is good: at least the tickets up to t
      for (long u = verified[k]; u <= t; ++u) if (slot(u) == k && in_ring(u)) verdict[u % nring] = GOOD;
      verified[k] = t + 1;
      return FOTG_OK;
    }
    if (flag != FOTG_ERR_STALL) return flag;
    // the word does not say which batch of this context raised it: all of them that are not settled yet are suspects
    for (long u = verified[k]; u < submitted; ++u) {
      if (slot(u) != k) continue;
      if (!in_ring(u)) {
        // more than nring submissions ago: its arguments are gone, so it can be neither recomputed nor cleared
        lost[k].add(u / depth, u / depth + 1);
        if (newly_stalled) ++*newly_stalled;
        continue;
      }
      int st = FOTG_ERR_STALL;
      if (heal && healable[u % nring]) {
        st = recompute(u);
        if (st != FOTG_OK && st != FOTG_ERR_STALL) return st;
      }
      verdict[u % nring] = st == FOTG_OK ? GOOD : STALLED;
      if (st != FOTG_OK && newly_stalled) ++*newly_stalled;
    }
    verified[k] = submitted;
    return status(t);
  }

  // fotg_pipe_sync after the host has synchronised with every slot: settle each slot's last ticket with heal = 1.  FOTG_ERR_STALL if
  // this call marked a ticket stalled (one settled before keeps its status for whoever waits for it).
  template <class TakeFlag, class Recompute>
  int sync(TakeFlag take_flag, Recompute recompute)
  {
    int st = FOTG_OK;
    for (int k = 0; k < depth; ++k) {
      long last = submitted - 1;
      while (last >= 0 && slot(last) != k) --last;
      if (last < 0 || last < verified[k]) continue;
      int bad = 0;
      const int sk = verify(last, 1, take_flag, recompute, &bad);
      if (sk != FOTG_OK) st = sk;
      else if (bad) st = FOTG_ERR_STALL;
    }
    return st;
  }
};

// final status of the jobs a fotg_node has waited for (they are waited for in order): the last `ring` jobs' own status, and every
// job that ended FOTG_ERR_STALL for good -- a later wait for it reports the stall however many jobs have followed
template <int RING>
struct JobBook {
  int status[RING] = {};
  long id[RING];
  RangeSet stalled;

  JobBook() { for (auto &v : id) v = -1; }
  void record(long job, int st)
  {
    status[job % RING] = st; id[job % RING] = job;
    if (st == FOTG_ERR_STALL) stalled.add(job, job + 1);
  }
  int status_of(long job) const
  {
    if (stalled.has(job)) return FOTG_ERR_STALL;
    return id[job % RING] == job ? status[job % RING] : FOTG_OK;
  }
};

}  // namespace fotg_tickets
