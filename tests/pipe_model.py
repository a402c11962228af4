"""Reference model of the stall / recompute contract of fotg_pipe_* and fotg_node_wait (include/fotg.h: the RECOMPUTE CONTRACT above
fotg_pipe_wait, and fotg_node_wait), in plain Python.  It is the specification the pipe's bookkeeping (flowonthego_amd/csrc/
pipe_tickets.h) is checked against, call by call: tests/test_pipe_tickets.py on the CPU, tests/test_gpu_pipe_tickets.py through the
real library.  Kept deliberately plain: one dict entry per ticket, no ring arithmetic beyond "is it among the last 4 * depth"."""

OK, ARG, STALL = 0, 1, 5
UNVERIFIED, GOOD, STALLED = "unverified", "good", "stalled"


class PipeModel:
    """A pipe of `depth` slots: ticket t runs on slot t % depth; the pipe keeps the arguments of the last 4 * depth submissions."""

    def __init__(self, depth):
        self.depth = depth
        self.ring = 4 * depth
        self.submitted = 0
        self.healable = {}                  # ticket -> its buffers are still in place (it may be recomputed)
        self.verdict = {}                   # ticket -> UNVERIFIED / GOOD / STALLED
        self.flagged = [False] * depth      # per slot: the context's stall word
        self.frontier = [0] * depth         # per slot: its tickets below this one have their verdict

    def slot(self, t):
        return t % self.depth

    def valid(self, t):
        return 0 <= t < self.submitted

    def in_ring(self, t):
        return t >= self.submitted - self.ring

    def submit(self, no_recompute=False):
        t = self.submitted
        self.healable[t] = not no_recompute
        self.verdict[t] = UNVERIFIED
        self.submitted += 1
        return t

    def hand_out(self, t):
        """fotg_pipe_wait(host_wait = 0) and fotg_pipe_ticket_event"""
        if not self.valid(t):
            return ARG
        if self.in_ring(t):
            self.healable[t] = False
        return OK

    def inject_stall(self, k):
        self.flagged[k] = True

    def suspects(self, k):
        """the tickets of slot k a flag found now would make suspects"""
        return [u for u in range(self.frontier[k], self.submitted) if self.slot(u) == k]

    def wait(self, t, m, recompute):
        """host wait, m = 1 (heal) or 2 (report).  recompute(u) recomputes ticket u and returns True if that went through clean."""
        if not self.valid(t):
            return ARG
        k = self.slot(t)
        if t < self.frontier[k]:
            return STALL if self.verdict[t] == STALLED else OK
        if not self.flagged[k]:
            for u in range(self.frontier[k], t + 1):
                if self.slot(u) == k:
                    self.verdict[u] = GOOD
            self.frontier[k] = t + 1
            return OK
        self.flagged[k] = False
        for u in self.suspects(k):
            if not self.in_ring(u):
                self.verdict[u] = STALLED
            elif m == 1 and self.healable[u]:
                self.verdict[u] = GOOD if recompute(u) else STALLED
            else:
                self.verdict[u] = STALLED
        self.frontier[k] = self.submitted
        return STALL if self.verdict[t] == STALLED else OK

    def sync(self, recompute):
        """fotg_pipe_sync: each slot's last ticket with m = 1; FOTG_ERR_STALL if this call marked any ticket stalled"""
        before = sum(v == STALLED for v in self.verdict.values())
        for k in range(self.depth):
            mine = [u for u in range(self.submitted) if self.slot(u) == k]
            if mine:
                self.wait(mine[-1], 1, recompute)
        after = sum(v == STALLED for v in self.verdict.values())
        return STALL if after > before else OK


class NodeModel:
    """fotg_node_wait over one PipeModel per device slot.  A job is a list of pieces (slot, ticket, pulled); pulled pieces of a
    scatter are waited for with m = 2, resident shards and the source slot with m = 1.  Jobs are waited for in order; a job's status
    is the worst of its pieces' and it keeps that status on every later wait."""

    def __init__(self, pipes):
        self.pipes = pipes
        self.jobs = []
        self.status = {}
        self.waited = 0

    def add_job(self, pieces):
        self.jobs.append(list(pieces))
        return len(self.jobs) - 1

    def wait(self, j, recompute):
        """recompute(slot, ticket) -> True if clean"""
        if not 0 <= j < len(self.jobs):
            return ARG
        if j < self.waited:
            return self.status[j]
        worst = OK
        for i in range(self.waited, j + 1):
            st = OK
            for s, t, pulled in self.jobs[i]:
                sp = self.pipes[s].wait(t, 2 if pulled else 1, lambda u, s=s: recompute(s, u))
                if sp != OK and st == OK:
                    st = sp
            self.status[i] = st
            if st != OK and worst == OK:
                worst = st
        self.waited = j + 1
        return worst
