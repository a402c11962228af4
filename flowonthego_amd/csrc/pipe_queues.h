// pipe_queues.h -- which priority class each slot stream of a fotg_pipe is created in, in plain C++ (no HIP): a pure function of the
// hardware-queue budget, the depth and the device's stream-priority range.  fotg_capi.hip keeps every HIP call (the streams, the
// overlap probe) and asks this header where the slots go; tests/pipe_queues_drv.cpp builds it with g++ for tests/test_host_pipe_queues.py.
//
// Why: the HIP runtime deals the streams of a process to GPU_MAX_HW_QUEUES hardware queues PER STREAM PRIORITY (three pools: high,
// normal, low), and two busy streams on one queue run one after the other.  The null stream and every stream a framework creates
// live in the normal pool; with the default budget of 4 a pipe of depth 4 in the normal pool has slots that share a queue.  Slot
// streams created with a priority draw from a pool nobody else uses.
#pragma once
#include <string.h>
#include <initializer_list>
#include "../../include/fotg.h"

namespace fotg_queues {

enum : int { MODE_AUTO = -1, MODE_BAD = -2 };                      // the layouts themselves are FOTG_PIPE_QUEUES_* (include/fotg.h)
enum : signed char { CLS_NORMAL = 0, CLS_HIGH = 1, CLS_LOW = 2 };

struct Plan {
  int layout;                                  // FOTG_PIPE_QUEUES_*: what the slots actually got (NORMAL if no slot left the normal pool)
  signed char cls[FOTG_PIPE_MAX_DEPTH];        // per slot: CLS_*
  int count[3];                                // slots per class
  bool shared;                                 // some pool holds more streams than it has queues: slots share a queue (the warning)
};

// FOTG_PIPE_QUEUES=auto|normal|high|split (unset = auto)
inline int parse_mode(const char *s)
{
  if (!s || !*s || !strcmp(s, "auto")) return MODE_AUTO;
  if (!strcmp(s, "normal")) return FOTG_PIPE_QUEUES_NORMAL;
  if (!strcmp(s, "high")) return FOTG_PIPE_QUEUES_HIGH;
  if (!strcmp(s, "split")) return FOTG_PIPE_QUEUES_SPLIT;
  return MODE_BAD;
}

inline const char *layout_name(int layout)
{
  return layout == FOTG_PIPE_QUEUES_HIGH ? "high" : layout == FOTG_PIPE_QUEUES_SPLIT ? "split" : "normal";
}

// the automatic rule: with a queue per slot and one for the null stream the normal pool is enough (exactly the streams the pipe
// always had); below that the slots leave it
inline int auto_layout(int budget, int depth) { return budget >= depth + 1 ? FOTG_PIPE_QUEUES_NORMAL : FOTG_PIPE_QUEUES_HIGH; }

// The slots of one pipe under `layout`.  Priorities as HIP numbers them: smaller = more urgent, 0 = what plain streams get;
// prio_greatest < 0 means the device has a high pool, prio_least > 0 a low one.
//   NORMAL  every slot in the normal pool
//   HIGH    the highest-priority pool first, up to `budget` slots; further slots to the lowest-priority pool, up to `budget`; what is
//           left to normal
//   SPLIT   slots alternate between the high and the low pool (each up to `budget`, the other one when full); what is left to normal
inline Plan place(int layout, int budget, int depth, int prio_least, int prio_greatest)
{
  Plan pl = {};
  if (budget < 1) budget = 1;
  if (depth > FOTG_PIPE_MAX_DEPTH) depth = FOTG_PIPE_MAX_DEPTH;
  int room[3] = {depth, prio_greatest < 0 ? budget : 0, prio_least > 0 ? budget : 0};
  if (layout == FOTG_PIPE_QUEUES_NORMAL) room[CLS_HIGH] = room[CLS_LOW] = 0;
  for (int k = 0; k < depth; ++k) {
    const bool low_first = layout == FOTG_PIPE_QUEUES_SPLIT && (k & 1);
    const signed char first = low_first ? CLS_LOW : CLS_HIGH, second = low_first ? CLS_HIGH : CLS_LOW;
    const signed char c = pl.count[first] < room[first] ? first : pl.count[second] < room[second] ? second : (signed char)CLS_NORMAL;
    pl.cls[k] = c;
    ++pl.count[c];
  }
  pl.layout = pl.count[CLS_NORMAL] == depth ? FOTG_PIPE_QUEUES_NORMAL : layout;
  // the normal pool also carries the null stream: a pipe that lives there alone needs budget >= depth + 1 (the rule the pipe always
  // had); slots that only overflow into it are counted against the budget itself, so three pools serve depth <= 3 * budget
  pl.shared = pl.count[CLS_NORMAL] > (pl.count[CLS_NORMAL] == depth ? budget - 1 : budget);
  return pl;
}

inline int priority_of(signed char cls, int prio_least, int prio_greatest)
{
  return cls == CLS_HIGH ? prio_greatest : cls == CLS_LOW ? prio_least : 0;
}

// the layouts fotg_pipe_create tries after `first` did not overlap: high, split, normal, without `first`
inline int fallback_order(int first, int out[3])
{
  int n = 0;
  for (int l : {FOTG_PIPE_QUEUES_HIGH, FOTG_PIPE_QUEUES_SPLIT, FOTG_PIPE_QUEUES_NORMAL})
    if (l != first) out[n++] = l;
  return n;
}

}  // namespace fotg_queues
