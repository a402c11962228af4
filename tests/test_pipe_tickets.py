"""The stall / recompute bookkeeping of fotg_pipe_* and fotg_node_wait (flowonthego_amd/csrc/pipe_tickets.h), on the CPU: the header is
built with g++ into a small driver (tests/pipe_tickets_drv.cpp) whose stall words and recompute outcomes the test scripts, and every
return value and every recompute request is compared, call by call, with the reference model of the contract (tests/pipe_model.py).
No GPU: the HIP side of these calls (synchronisation, the recompute itself) is covered by tests/test_gpu_pipe_tickets.py."""
import ctypes as C
import os
import random
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
from pipe_model import ARG, OK, STALL, NodeModel, PipeModel  # noqa: E402


@pytest.fixture(scope="module")
def drv(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("pipe_tickets") / "libpipe_tickets_drv.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC",
                           os.path.join(HERE, "pipe_tickets_drv.cpp"), "-o", so])
    L = C.CDLL(so)
    L.drv_new.restype = C.c_void_p
    L.drv_new.argtypes = [C.c_int]
    L.drv_free.argtypes = [C.c_void_p]
    L.drv_submit.restype = C.c_long
    L.drv_submit.argtypes = [C.c_void_p, C.c_int]
    L.drv_hand_out.argtypes = [C.c_void_p, C.c_long]
    L.drv_inject_stall.argtypes = [C.c_void_p, C.c_int]
    L.drv_fail_recompute.argtypes = [C.c_void_p, C.c_long]
    L.drv_wait.argtypes = [C.c_void_p, C.c_long, C.c_int]
    L.drv_sync.argtypes = [C.c_void_p]
    L.drv_recomputed.argtypes = [C.c_void_p, C.POINTER(C.c_long), C.c_int]
    L.drv_lost_ranges.argtypes = [C.c_void_p, C.c_int]
    L.drv_job_record.argtypes = [C.c_void_p, C.c_long, C.c_int]
    L.drv_job_status.argtypes = [C.c_void_p, C.c_long]
    return L


class Book:
    """the header through the driver, with the model's method names"""

    def __init__(self, L, depth):
        self.L, self.depth, self.ring = L, depth, 4 * depth
        self.h = L.drv_new(depth)
        assert self.h

    def close(self):
        self.L.drv_free(self.h)

    def submit(self, no_recompute=False):
        return self.L.drv_submit(self.h, int(no_recompute))

    def hand_out(self, t):
        return self.L.drv_hand_out(self.h, t)

    def inject_stall(self, k):
        self.L.drv_inject_stall(self.h, k)

    def fail_recompute(self, u):
        self.L.drv_fail_recompute(self.h, u)

    def wait(self, t, m):
        return self.L.drv_wait(self.h, t, m)

    def sync(self):
        return self.L.drv_sync(self.h)

    def recomputed(self):
        buf = (C.c_long * 4096)()
        n = self.L.drv_recomputed(self.h, buf, 4096)
        assert n <= 4096
        return list(buf[:n])

    def lost_ranges(self, k):
        return self.L.drv_lost_ranges(self.h, k)


class Pair:
    """the header and the model side by side: every call is made on both and must agree, recompute requests included"""

    def __init__(self, L, depth):
        self.real = Book(L, depth)
        self.model = PipeModel(depth)
        self.fails = set()
        self.log = []

    def close(self):
        self.real.close()

    def _recompute(self, u):
        self.log.append(u)
        return u not in self.fails

    def _check(self, what, got, want):
        asked = self.real.recomputed()
        assert (got, asked) == (want, self.log), "%s: header %r, recomputed %r; model %r, recomputed %r" % (what, got, asked, want, self.log)
        self.log = []
        return got

    def submit(self, no_recompute=False, recompute_stalls=False):
        t = self.real.submit(no_recompute)
        assert t == self.model.submit(no_recompute)
        if recompute_stalls:
            self.fails.add(t)
            self.real.fail_recompute(t)
        return t

    def hand_out(self, t):
        return self._check("hand_out(%d)" % t, self.real.hand_out(t), self.model.hand_out(t))

    def inject_stall(self, k):
        self.real.inject_stall(k)
        self.model.inject_stall(k)

    def wait(self, t, m):
        return self._check("wait(%d, %d)" % (t, m), self.real.wait(t, m), self.model.wait(t, m, self._recompute))

    def sync(self):
        return self._check("sync()", self.real.sync(), self.model.sync(self._recompute))


@pytest.fixture
def pair(drv):
    made = []

    def make(depth):
        p = Pair(drv, depth)
        made.append(p)
        return p
    yield make
    for p in made:
        p.close()


# ---- the three defects of the round-6 review, at the bookkeeping level ---------------------------------------------------------

@pytest.mark.parametrize("how", ["hand_out", "no_recompute", "report"])
def test_a_stalled_ticket_stays_stalled_after_its_ring_entry_is_reused(pair, how):
    """depth 2, ring 8: ticket 0 is stalled and not recomputed (handed out / submitted with NO_RECOMPUTE / found by a host_wait = 2);
    8 more submissions reuse its ring entry -- its waits still report FOTG_ERR_STALL"""
    p = pair(2)
    for k in range(4):
        p.submit(no_recompute=how == "no_recompute" and k == 0)
    if how == "hand_out":
        assert p.hand_out(0) == OK
    p.inject_stall(0)
    if how == "report":
        assert p.wait(0, 2) == STALL
        assert p.wait(2, 1) == STALL                    # (settled by that wait: reported, not recomputed)
    else:
        assert p.wait(2, 1) == OK and p.model.verdict[2] == "good"
        assert p.wait(0, 1) == STALL
    for _ in range(8):
        p.submit()
    assert p.wait(0, 1) == STALL and p.wait(0, 2) == STALL
    for _ in range(40):
        p.submit()
    assert p.wait(0, 1) == STALL and p.sync() == OK and p.wait(0, 1) == STALL
    assert p.wait(1, 1) == OK and p.wait(3, 2) == OK


def test_pulled_scatter_pieces_stay_stalled_behind_a_later_job(pair):
    """the node's pulling scatter slot: jobs A (tickets 0-3) and B (4-7) of NO_RECOMPUTE pieces; the wait for A finds the flag and
    marks every piece of context 0 stalled, B's 4 and 6 included; job C submits 8 pieces before B is waited for"""
    p = pair(2)
    A = [p.submit(no_recompute=True) for _ in range(4)]
    B = [p.submit(no_recompute=True) for _ in range(4)]
    for t in A + B:
        assert p.hand_out(t) == OK                      # (the push-back of its flows waits on the copy stream)
    p.inject_stall(0)
    assert [p.wait(t, 2) for t in A] == [STALL, OK, STALL, OK]
    C_ = [p.submit(no_recompute=True) for _ in range(8)]
    assert [p.wait(t, 2) for t in B] == [STALL, OK, STALL, OK]
    assert [p.wait(t, 2) for t in C_] == [OK] * 8


def test_good_tickets_between_two_stalls_stay_good(pair):
    """depth 1: suspects 0-1 and, much later, 106-107 stalled; every ticket between them was waited for and is good, and stays good
    (one hull range over both stalls reported them all as FOTG_ERR_STALL)"""
    p = pair(1)
    p.submit(no_recompute=True); p.submit(no_recompute=True)
    p.inject_stall(0)
    assert p.wait(1, 2) == STALL and p.wait(0, 1) == STALL
    for _ in range(104):
        t = p.submit()
        assert p.wait(t, 1) == OK
    p.submit(); p.submit()
    p.inject_stall(0)
    assert p.wait(107, 2) == STALL
    for _ in range(20):
        p.submit()
    assert p.sync() == OK
    assert [p.wait(t, 1) for t in (0, 1, 2, 50, 105, 106, 107, 108)] == [STALL, STALL, OK, OK, OK, STALL, STALL, OK]
    assert p.real.lost_ranges(0) == 2


def test_stalled_runs_are_kept_as_few_disjoint_ranges(pair):
    """the per-slot set of stalled tickets that left the ring merges neighbours: 8 stall events of 3 suspects each on slot 1 of a
    depth-2 pipe, with good tickets between the events -> 8 ranges, however many tickets follow"""
    p = pair(2)
    for ev in range(8):
        ts = [p.submit(no_recompute=True) for _ in range(6)]
        p.inject_stall(1)
        assert p.wait(ts[1], 2) == STALL
        for t in ts:
            assert p.wait(t, 1) == (STALL if t % 2 == 1 else OK)
        good = [p.submit() for _ in range(2)]
        assert all(p.wait(t, 1) == OK for t in good)
    for _ in range(30):
        p.submit()
    assert p.real.lost_ranges(1) == 8 and p.real.lost_ranges(0) == 0
    assert all(p.wait(t, 1) == (STALL if t % 8 in (1, 3, 5) else OK) for t in range(64))


def test_a_node_job_that_stalled_reports_it_after_more_than_16_later_jobs(drv):
    """fotg_node_wait keeps a job's own status in a ring of 16 jobs; a job that ended FOTG_ERR_STALL reports it on every later wait,
    however many jobs followed, and nothing else is blamed"""
    b = Book(drv, 1)
    try:
        for j in range(60):
            drv.drv_job_record(b.h, j, STALL if j in (3, 4, 40) else (2 if j == 50 else OK))
        got = [drv.drv_job_status(b.h, j) for j in range(60)]
        assert got == [STALL if j in (3, 4, 40) else (2 if j == 50 else OK) for j in range(60)]
        for j in range(60, 100):
            drv.drv_job_record(b.h, j, OK)
        assert [drv.drv_job_status(b.h, j) for j in (3, 4, 5, 39, 40, 41, 99)] == [STALL, STALL, OK, OK, STALL, OK, OK]
    finally:
        b.close()


def test_invalid_tickets(pair):
    p = pair(3)
    assert p.wait(0, 1) == ARG and p.hand_out(0) == ARG and p.sync() == OK
    t = p.submit()
    assert p.wait(-1, 1) == ARG and p.wait(t + 1, 2) == ARG and p.hand_out(-5) == ARG and p.hand_out(t + 1) == ARG
    assert p.wait(t, 1) == OK


def test_a_recompute_that_stalls_again_is_reported(pair):
    p = pair(2)
    ts = [p.submit(recompute_stalls=(k == 2)) for k in range(6)]
    p.inject_stall(0)
    assert p.wait(ts[0], 1) == OK                       # 0 and 4 healed, 2 stalled again
    assert p.model.verdict[2] == "stalled" and p.wait(2, 1) == STALL and p.wait(4, 1) == OK
    for _ in range(16):
        p.submit()
    assert p.wait(2, 2) == STALL and p.wait(4, 2) == OK


# ---- the hand-written GPU sequences (tests/test_gpu_parity.py, tests/test_gpu_distributed.py) replayed against the header --------

def test_replay_stalled_wait_heals_at_the_host_sync_points(pair):
    p = pair(2)
    ts = [p.submit() for _ in range(4)]
    p.inject_stall(0)
    assert p.wait(ts[0], 1) == OK and p.model.verdict[2] == "good"
    assert [p.wait(ts[k], 1) for k in (2, 1, 3)] == [OK] * 3
    t = p.submit()                                      # fotg_pipe_sync heals as well
    p.inject_stall(t % 2)
    assert p.sync() == OK
    t = p.submit()                                      # host_wait = 2: report, do not recompute -- and the ticket keeps its status
    p.inject_stall(t % 2)
    assert p.wait(t, 2) == STALL and p.wait(t, 2) == STALL and p.wait(t, 1) == STALL
    t2 = p.submit()
    assert p.wait(t2 + 1, 1) == ARG and p.hand_out(t2 + 1) == ARG and p.hand_out(t2) == OK
    assert p.wait(t2, 1) == OK
    t = p.submit()
    assert p.hand_out(t) == OK


def test_replay_recompute_only_where_the_buffers_are_still_in_place(pair):
    p = pair(2)
    ts = [p.submit() for _ in range(4)]                 # (1) ticket 0 handed to a stream, ticket 2 (same slot) not
    assert p.hand_out(ts[0]) == OK
    p.inject_stall(0)
    assert p.wait(ts[2], 1) == OK and p.model.verdict[0] == "stalled"
    assert p.wait(ts[0], 1) == STALL and p.wait(ts[0], 2) == STALL
    assert p.wait(ts[1], 1) == OK and p.wait(ts[3], 1) == OK
    assert p.sync() == OK                               # nothing new to report
    t = p.submit()                                      # ... and through the event hand-out
    assert p.hand_out(t) == OK
    p.inject_stall(t % 2)
    assert p.sync() == STALL and p.wait(t, 1) == STALL
    t = p.submit(no_recompute=True)                     # (2) FOTG_SUBMIT_NO_RECOMPUTE
    p.inject_stall(t % 2)
    assert p.wait(t, 1) == STALL
    p = pair(2)                                         # (3) more than 4 * depth submissions outstanding when the flag is found
    ts = [p.submit() for _ in range(10)]
    p.inject_stall(0)
    assert p.wait(ts[0], 1) == STALL
    for k in (2, 4, 6, 8):
        assert p.model.verdict[k] == "good" and p.wait(ts[k], 1) == OK
    for k in (1, 3, 5, 7, 9):
        assert p.wait(ts[k], 1) == OK
    assert p.wait(ts[0], 1) == STALL


def test_replay_node_heals_or_reports_a_stalled_wait_per_job(drv):
    """test_gpu_distributed.py::test_node_heals_or_reports_a_stalled_wait_per_job on slot 1's pipe (depth 2), through NodeModel"""
    pipes = [Pair(drv, 2), Pair(drv, 2)]
    try:
        node = NodeModel([p.model for p in pipes])

        def piece(s, pulled=False):
            t = pipes[s].real.submit(pulled)
            assert t == pipes[s].model.submit(pulled)
            if pulled:
                assert pipes[s].real.hand_out(t) == OK and pipes[s].model.hand_out(t) == OK
            return (s, t, pulled)

        def wait(j):
            want = node.wait(j, lambda s, u: True)
            got = OK
            for s, t, pulled in node.jobs[j]:
                sp = pipes[s].real.wait(t, 2 if pulled else 1)
                got = sp if got == OK else got
            return want, got

        # resident: 4 pairs on 2 slots, max_batch 2 -> one piece per slot per job
        j = node.add_job([piece(0), piece(1)])
        assert wait(j) == (OK, OK)
        jobs = [node.add_job([piece(0), piece(1)]) for _ in range(3)]
        pipes[1].inject_stall(0)
        for j in jobs:
            assert wait(j) == (OK, OK)
        # scatter, chunk 1: the source slot's pieces in place, slot 1's pulled
        scatter = lambda: node.add_job([piece(0), piece(0), piece(1, True), piece(1, True)])
        t0 = scatter()
        assert wait(t0) == (OK, OK)
        t1 = scatter()
        pipes[1].inject_stall(0)
        assert wait(t1)[0] == STALL
        t2 = scatter()
        assert wait(t2) == (OK, OK)
        assert node.wait(t1, None) == STALL and node.wait(t0, None) == OK and node.wait(t2, None) == OK
    finally:
        for p in pipes:
            p.close()


# ---- seeded random sequences against the model ----------------------------------------------------------------------------------

def run_sequence(p, rng, n_ops):
    """one random sequence of pipe calls on a Pair; every call is checked inside Pair"""
    m = p.model
    for _ in range(n_ops):
        r = rng.random()
        if r < 0.30 or m.submitted == 0:
            for _ in range(rng.choice((1, 1, 1, 2, m.depth, m.ring, 2 * m.ring + 1))):
                p.submit(no_recompute=rng.random() < 0.25, recompute_stalls=rng.random() < 0.1)
        elif r < 0.40:
            p.hand_out(rng.randrange(m.submitted))
        elif r < 0.55:
            p.inject_stall(rng.randrange(m.depth))
        elif r < 0.93:
            x = rng.random()
            if x < 0.35:
                t = rng.randrange(max(0, m.submitted - m.ring), m.submitted)           # in the ring
            elif x < 0.55:
                t = m.submitted - 1
            elif x < 0.9:
                t = rng.randrange(m.submitted)                                         # anywhere, mostly out of the ring
            else:
                t = rng.choice((-1, m.submitted, m.submitted + rng.randrange(1, 50)))   # invalid
            p.wait(t, rng.choice((1, 2)))
        else:
            p.sync()
    # every ticket once more, in a random order and both ways: the verdicts must hold
    ts = list(range(m.submitted))
    rng.shuffle(ts)
    for t in ts:
        p.wait(t, rng.choice((1, 2)))


SEEDS = range(3000)


def test_random_sequences_match_the_model(drv):
    """3000 seeded sequences over depth 1..8, 10-60 operations each (bursts of submits push tickets far out of the ring)"""
    for seed in SEEDS:
        rng = random.Random(seed)
        p = Pair(drv, rng.randint(1, 8))
        try:
            run_sequence(p, rng, rng.randint(10, 60))
        except AssertionError as e:
            raise AssertionError("seed %d, depth %d: %s" % (seed, p.model.depth, e)) from None
        finally:
            p.close()
