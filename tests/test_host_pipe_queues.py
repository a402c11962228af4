"""Where a pipe's slot streams go (flowonthego_amd/csrc/pipe_queues.h), on the CPU: the placement rule is a pure function of the
hardware-queue budget, the depth and the device's stream-priority range.  The header is built with g++ into a small driver
(tests/pipe_queues_drv.cpp) and compared, for every budget 1..32 and every depth 1..FOTG_PIPE_MAX_DEPTH, with the rule restated
here from its description in include/fotg.h.  No GPU: the streams themselves and the overlap probe are covered by
tests/test_gpu_pipe_queues.py."""
import ctypes as C
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

NORMAL, HIGH, SPLIT = 0, 1, 2          # FOTG_PIPE_QUEUES_* == the layout names in order
CN, CH, CL = 0, 1, 2                   # a slot's class: normal, high, low
THREE, TWO, ONE = (1, -1), (0, -1), (0, 0)      # (least, greatest) priority: three pools, no low pool, a single level


@pytest.fixture(scope="module")
def drv(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("pipe_queues") / "libpipe_queues_drv.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC",
                           os.path.join(HERE, "pipe_queues_drv.cpp"), "-o", so])
    L = C.CDLL(so)
    L.drv_parse_mode.argtypes = [C.c_char_p]
    L.drv_place.argtypes = [C.c_int] * 5 + [C.POINTER(C.c_int)] * 2
    L.drv_fallback_order.argtypes = [C.c_int, C.POINTER(C.c_int)]
    L.drv_outstanding.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_long), C.c_int]
    return L


def place(L, layout, budget, depth, rng):
    cls, prio = (C.c_int * depth)(), (C.c_int * depth)()
    r = L.drv_place(layout, budget, depth, rng[0], rng[1], cls, prio)
    return r & 255, bool(r >> 8), list(cls), list(prio)


def rule(layout, budget, depth, rng):
    """the rule as include/fotg.h words it -> (classes, warning)"""
    least, greatest = rng
    room = {CH: budget if greatest < 0 else 0, CL: budget if least > 0 else 0}
    if layout == NORMAL:
        room = {CH: 0, CL: 0}
    cls = []
    for k in range(depth):
        order = (CL, CH) if layout == SPLIT and k % 2 else (CH, CL)
        c = next((c for c in order if cls.count(c) < room[c]), CN)
        cls.append(c)
    n = cls.count(CN)
    # a pipe alone in the normal pool shares it with the null stream; overflow into it is counted against the budget itself
    return cls, n > (budget - 1 if n == depth else budget)


def test_max_depth_and_switch_values(drv):
    hdr = open(os.path.join(ROOT, "include", "fotg.h")).read()
    assert drv.drv_max_depth() == int(re.search(r"#define FOTG_PIPE_MAX_DEPTH (\d+)", hdr).group(1)) == 8
    for name, val in (("NORMAL", NORMAL), ("HIGH", HIGH), ("SPLIT", SPLIT)):
        assert int(re.search(r"#define FOTG_PIPE_QUEUES_%s\s+(\d+)" % name, hdr).group(1)) == val
    assert [drv.drv_parse_mode(s) for s in (None, b"", b"auto", b"normal", b"high", b"split")] == [-1, -1, -1, NORMAL, HIGH, SPLIT]
    assert all(drv.drv_parse_mode(s) == -2 for s in (b"Auto", b"low", b"1", b"high "))
    out = (C.c_int * 3)()
    for first, rest in ((NORMAL, [HIGH, SPLIT]), (HIGH, [SPLIT, NORMAL]), (SPLIT, [HIGH, NORMAL])):
        assert drv.drv_fallback_order(first, out) == 2 and list(out)[:2] == rest


@pytest.mark.parametrize("rng", [THREE, TWO, ONE, (2, -3)])
def test_every_layout_follows_the_rule(drv, rng):
    for budget in range(1, 33):
        for depth in range(1, 9):
            for layout in (NORMAL, HIGH, SPLIT):
                got_layout, warn, cls, prio = place(drv, layout, budget, depth, rng)
                want_cls, want_warn = rule(layout, budget, depth, rng)
                assert (cls, warn) == (want_cls, want_warn), (layout, budget, depth)
                assert prio == [{CN: 0, CH: rng[1], CL: rng[0]}[c] for c in cls]
                assert got_layout == (NORMAL if set(cls) == {CN} else layout)
                assert max(cls.count(CH), cls.count(CL)) <= budget


def test_auto_keeps_todays_streams_where_the_budget_is_enough(drv):
    """budget >= depth + 1: normal priority for every slot and no warning, whatever the device offers"""
    for rng in (THREE, TWO, ONE):
        for budget in range(1, 33):
            for depth in range(1, 9):
                auto = drv.drv_auto_layout(budget, depth)
                assert auto == (NORMAL if budget >= depth + 1 else HIGH)
                if auto == NORMAL:
                    assert place(drv, auto, budget, depth, rng) == (NORMAL, False, [CN] * depth, [0] * depth)


def test_auto_below_the_budget_fills_high_then_low_then_normal(drv):
    for budget in range(1, 9):
        for depth in range(budget, 9):          # budget < depth + 1
            layout, warn, cls, _ = place(drv, drv.drv_auto_layout(budget, depth), budget, depth, THREE)
            nh = min(depth, budget)
            nl = min(depth - nh, budget)
            assert cls == [CH] * nh + [CL] * nl + [CN] * (depth - nh - nl) and layout == HIGH
            assert warn == (depth > 3 * budget)          # only when three pools together are too small
    # the cases of the GPU tests: the default budget
    assert place(drv, HIGH, 4, 4, THREE)[1:3] == (False, [CH] * 4)
    assert place(drv, HIGH, 4, 6, THREE)[1:3] == (False, [CH] * 4 + [CL] * 2)
    assert place(drv, HIGH, 4, 8, THREE)[1:3] == (False, [CH] * 4 + [CL] * 4)
    assert place(drv, SPLIT, 4, 4, THREE)[1:3] == (False, [CH, CL, CH, CL])
    assert place(drv, HIGH, 1, 8, THREE)[1:3] == (True, [CH, CL] + [CN] * 6)


def test_single_priority_level_everything_normal_and_the_warning_fires(drv):
    for budget in range(1, 33):
        for depth in range(1, 9):
            for layout in (drv.drv_auto_layout(budget, depth), HIGH, SPLIT):
                got_layout, warn, cls, prio = place(drv, layout, budget, depth, ONE)
                assert (got_layout, cls, prio) == (NORMAL, [CN] * depth, [0] * depth)
                assert warn == (budget < depth + 1)
    # no low pool: high up to the budget, the rest normal
    assert place(drv, HIGH, 4, 6, TWO)[1:3] == (False, [CH] * 4 + [CN] * 2)
    assert place(drv, SPLIT, 2, 4, TWO)[1:3] == (False, [CH, CH, CN, CN])


def test_outstanding_tickets(drv):
    """what fotg_pipe_probe_overlap refuses on: a submitted ticket that no host wait has settled"""
    def outstanding(depth, nsubmit, settled):
        arr = (C.c_long * max(1, len(settled)))(*settled)
        return bool(drv.drv_outstanding(depth, nsubmit, arr, len(settled)))
    for depth in range(1, 9):
        assert not outstanding(depth, 0, [])
        for n in range(1, 3 * depth + 2):
            assert outstanding(depth, n, [])
            last = list(range(max(0, n - depth), n))          # every slot's last ticket
            assert not outstanding(depth, n, last)
            for leave in last:
                assert outstanding(depth, n, [t for t in last if t != leave])
            if n > depth:
                assert outstanding(depth, n, list(range(n - depth)))          # older tickets settled, the last ones not
