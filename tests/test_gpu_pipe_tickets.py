"""The stall / recompute contract of fotg_pipe_* and fotg_node_wait through the real library, against the reference model
(tests/pipe_model.py).  Stalls come only from the inject_stall tap (FOTG_TEST_TAPS=1), which sets a context's host word like a
timed-out inter-workgroup wait would.  Small frames (96 x 160, op-pt 2: no level is tall enough for the tile solver, so nothing
raises the word but the tap), depth <= 3, and three frame pairs cycled through every pipe: a recompute from the wrong ticket's
arguments, or into the wrong ticket's outflow, shows in the flows."""
import ctypes as C
import os
import random
import sys
import time

import numpy as np
import pytest
import torch

from conftest import synth_pair

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pipe_model import ARG, GOOD, OK, STALL, STALLED, NodeModel, PipeModel  # noqa: E402

pytestmark = pytest.mark.gpu

H, W = 96, 160


@pytest.fixture(scope="module")
def frames():
    """three frame pairs on the GPU and their flows from one plain context"""
    import flowonthego_amd as F
    from flowonthego_amd.oflow import OFClass
    pairs = [synth_pair(H, W, seed=900 + k) for k in range(3)]
    A = torch.from_numpy(np.stack([p[0] for p in pairs])).cuda()
    B = torch.from_numpy(np.stack([p[1] for p in pairs])).cuda()
    op = F.operating_point(2, W, 1)
    ip = F.img_params(width=W, height=H, padding=op.patch_size)
    ofc = OFClass(op, ip, max_batch=3)
    ref = ofc.calc_batch(A, B).clone()
    torch.cuda.synchronize()
    ofc.close()
    return F, op, ip, A, B, ref


def _inject(F, ctx):
    assert F.lib().fotg_ctx_counter(ctx, b"inject_stall") == 0


class GpuPipe:
    """a FlowPipeline and the model side by side: ticket t computes pair t % 3 into an outflow of its own"""

    def __init__(self, frames, depth):
        from flowonthego_amd.pipeline import FlowPipeline
        self.F, op, ip, self.A, self.B, self.ref = frames
        self.L = self.F.lib()
        self.pipe = FlowPipeline(op, ip, max_batch=1, depth=depth)
        self.model = PipeModel(depth)
        self.outs = []
        self.zeroed = set()          # tickets whose outflow the test zeroed after their compute
        torch.cuda.synchronize()

    def close(self):
        self.pipe.close()

    def submit(self, no_recompute=False):
        t = len(self.outs)
        out = self.pipe.new_outflow(1)
        got, _ = self.pipe.submit(self.A[t % 3][None], self.B[t % 3][None], None, out, no_recompute=no_recompute)
        assert got == t == self.model.submit(no_recompute)
        self.outs.append(out)
        return t

    def hand_out(self, t, event=False):
        if event:
            got = self.L.fotg_pipe_ticket_event(self.pipe._h, t, C.c_void_p())
        else:
            got = self.L.fotg_pipe_wait(self.pipe._h, t, None, 0)
        assert got == self.model.hand_out(t), ("hand_out", t, event)

    def inject_stall(self, k):
        """the slot has run what it was given; the outflows of the model's suspects are zeroed, then the word is raised"""
        torch.cuda.synchronize()
        for u in self.model.suspects(k):
            self.outs[u].zero_()
            self.zeroed.add(u)
        torch.cuda.synchronize()
        _inject(self.F, self.pipe.context(k))
        self.model.inject_stall(k)

    def wait(self, t, m):
        got = self.L.fotg_pipe_wait(self.pipe._h, t, None, m)
        want = self.model.wait(t, m, lambda u: True)
        assert got == want, ("wait", t, m, got, want)
        self.check_flows()
        return got

    def sync(self):
        got = self.L.fotg_pipe_sync(self.pipe._h)
        want = self.model.sync(lambda u: True)
        assert got == want, ("sync", got, want)
        self.check_flows()
        return got

    def check_flows(self):
        """good tickets hold their pair's flow exactly; stalled ones are as the test left them (the library did not write)"""
        good = [u for u, v in self.model.verdict.items() if v == GOOD]
        stalled = [u for u, v in self.model.verdict.items() if v == STALLED]
        if good:
            got = torch.cat([self.outs[u] for u in good])
            want = self.ref[torch.tensor([u % 3 for u in good], device=got.device)]
            bad = [u for u, g, w in zip(good, got, want) if not torch.equal(g, w)] if not torch.equal(got, want) else []
            assert not bad, "good tickets with a wrong flow: %s" % bad
        for u in stalled:
            want = torch.zeros_like(self.outs[u]) if u in self.zeroed else self.ref[u % 3][None]
            assert torch.equal(self.outs[u], want), "stalled ticket %d was written" % u


@pytest.fixture
def taps(monkeypatch):
    monkeypatch.setenv("FOTG_TEST_TAPS", "1")          # read once at fotg_create


# ---- deterministic regressions of the round-6 review ------------------------------------------------------------------------------

def test_pipe_stalled_ticket_stays_stalled_after_its_ring_entry_is_reused(frames, taps):
    p = GpuPipe(frames, 2)
    try:
        for _ in range(4):
            p.submit()
        p.hand_out(0)
        p.inject_stall(0)
        assert p.wait(2, 1) == OK and p.wait(0, 1) == STALL
        for _ in range(8):
            p.submit()
        assert p.wait(0, 1) == STALL and p.wait(0, 2) == STALL
        assert p.sync() == OK and p.wait(0, 1) == STALL
    finally:
        p.close()


def test_pipe_good_tickets_between_two_stalls_stay_good(frames, taps):
    """depth 1 (ring 4): two stalls whose oldest suspects (0-1, 106-107) have left the ring when the flag is found; every ticket
    between them was waited for and stays good (one hull range over both stalls reported them all as FOTG_ERR_STALL)"""
    p = GpuPipe(frames, 1)
    try:
        for _ in range(6):
            p.submit()
        p.inject_stall(0)
        assert p.wait(5, 2) == STALL
        for _ in range(100):
            p.submit()
        assert p.wait(105, 1) == OK
        for _ in range(6):
            p.submit()
        p.inject_stall(0)
        assert p.wait(111, 2) == STALL
        for _ in range(6):
            p.submit()
        assert p.sync() == OK
        assert [p.wait(t, 1) for t in (0, 5, 6, 50, 105, 106, 107, 111, 112)] == [STALL, STALL, OK, OK, OK, STALL, STALL, STALL, OK]
    finally:
        p.close()


def _node(frames, n_pairs):
    from flowonthego_amd.node import FlowNode
    F, op, ip, A, B, ref = frames
    node = FlowNode(op, ip, devices=[0, 0], max_batch=1, depth=2)
    pipe, ctx = C.c_void_p(), C.c_void_p()
    assert F.lib().fotg_node_pipe(node._h, 1, pipe) == 0 and F.lib().fotg_pipe_context(pipe, 0, ctx) == 0
    idx = torch.arange(n_pairs, device=A.device) % 3
    return node, pipe, ctx, A[idx].contiguous(), B[idx].contiguous(), ref[idx]


def _issued(L, pipe, ticket, what):
    """the node's slot thread has submitted `ticket` to this pipe (a pulled piece: NO_RECOMPUTE anyway, so the hand-out of its
    event changes nothing)"""
    deadline = time.time() + 30
    while L.fotg_pipe_ticket_event(pipe, ticket, C.c_void_p()) != 0:
        assert time.time() < deadline, "%s: ticket %d never issued" % what
        time.sleep(0.01)
    torch.cuda.synchronize()


def test_node_pulled_pieces_stay_stalled_behind_a_later_job(frames, taps):
    """scatter, chunk 1: jobs A and B put tickets 0-3 and 4-7 on slot 1's pipe (depth 2, ring 8); the wait for A finds the flag
    and marks 0, 2, 4, 6 stalled; job C (8 pieces on slot 1) reuses their ring entries before B is waited for"""
    F = frames[0]
    L = F.lib()
    node, pipe, ctx, G0, G1, want = _node(frames, 8)
    G0c, G1c, wantc = (torch.cat([x, x]) for x in (G0, G1, want))
    try:
        outs = [torch.zeros_like(want), torch.zeros_like(want), torch.zeros_like(wantc)]
        torch.cuda.synchronize()
        ta, _ = node.submit_scatter(G0, G1, outs[0], chunk=1)
        tb, _ = node.submit_scatter(G0, G1, outs[1], chunk=1)
        _issued(L, pipe, 7, "job B")
        _inject(F, ctx)
        assert L.fotg_node_wait(node._h, ta) == STALL
        tc, _ = node.submit_scatter(G0c, G1c, outs[2], chunk=1)
        _issued(L, pipe, 15, "job C")
        assert L.fotg_node_wait(node._h, tb) == STALL
        assert L.fotg_node_wait(node._h, tc) == OK and torch.equal(outs[2], wantc)
        assert [L.fotg_node_wait(node._h, t) for t in (ta, tb, tc)] == [STALL, STALL, OK]
    finally:
        node.close()


def test_node_stalled_job_reported_after_more_than_16_later_jobs(frames, taps):
    F = frames[0]
    L = F.lib()
    node, pipe, ctx, G0, G1, want = _node(frames, 2)
    try:
        out = torch.zeros_like(want)
        torch.cuda.synchronize()
        ts, _ = node.submit_scatter(G0, G1, out, chunk=1)          # slot 1: one pulled piece, ticket 0 of its pipe (context 0)
        _issued(L, pipe, 0, "the stalled job")
        _inject(F, ctx)
        assert L.fotg_node_wait(node._h, ts) == STALL
        later = []
        for _ in range(20):
            t, o = node.submit(2, [G0[:1], G0[1:]], [G1[:1], G1[1:]])
            node.wait(t)
            later.append((t, o))
        assert all(torch.equal(torch.cat(o), want) for _, o in later)
        assert L.fotg_node_wait(node._h, ts) == STALL
        assert all(L.fotg_node_wait(node._h, t) == OK for t, _ in later)
        # the model says the same
        pipes = [PipeModel(2), PipeModel(2)]
        nm = NodeModel(pipes)
        j = nm.add_job([(0, pipes[0].submit(), False), (1, pipes[1].submit(True), True)])
        pipes[1].hand_out(0); pipes[1].inject_stall(0)
        assert nm.wait(j, lambda s, u: True) == STALL
        for _ in range(20):
            nm.wait(nm.add_job([(0, pipes[0].submit(), False), (1, pipes[1].submit(), False)]), lambda s, u: True)
        assert nm.wait(j, None) == STALL
    finally:
        node.close()


# ---- model-driven sequences -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_sequence_matches_the_model(frames, taps, seed):
    rng = random.Random(seed)
    p = GpuPipe(frames, 1 + seed % 3)
    m = p.model
    try:
        p.submit()
        for _ in range(150):
            r = rng.random()
            if r < 0.35:
                for _ in range(rng.choice((1, 1, 2, m.depth, m.ring + 1))):
                    p.submit(no_recompute=rng.random() < 0.25)
            elif r < 0.45:
                p.hand_out(rng.randrange(m.submitted), event=rng.random() < 0.5)
            elif r < 0.57:
                p.inject_stall(rng.randrange(m.depth))
            elif r < 0.93:
                x = rng.random()
                if x < 0.4:
                    t = rng.randrange(max(0, m.submitted - m.ring), m.submitted)
                elif x < 0.6:
                    t = m.submitted - 1
                elif x < 0.93:
                    t = rng.randrange(m.submitted)
                else:
                    t = rng.choice((-1, m.submitted, m.submitted + 7))
                assert p.wait(t, rng.choice((1, 2))) in (OK, STALL, ARG)
            else:
                p.sync()
        for t in range(m.submitted):
            p.wait(t, 1)
        assert sum(v == STALLED for v in m.verdict.values()) > 0 and sum(v == GOOD for v in m.verdict.values()) > 0
    finally:
        p.close()
