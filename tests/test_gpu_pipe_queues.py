"""A pipe's slot streams get a hardware queue each at HIP's default budget (include/fotg.h, HARDWARE QUEUES; csrc/pipe_queues.h).

The budget (GPU_MAX_HW_QUEUES) is read by the HIP runtime when it loads, so every budget runs in ONE fresh child process
(tests/pipe_queues_child.py) that reports one JSON line; the tests of a budget share that one run.  A child that dies of a signal or
hits its timeout fails its tests, nothing is retried and no further child is started.  Frames as in tests/test_gpu_pipe_tickets.py
(96 x 160, op-pt 2)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CHILD = os.path.join(HERE, "pipe_queues_child.py")
FOTG_ERR_ARG = 1
_dead = []          # a child died of a signal or a timeout: start no other


def run_child(which, budget):
    if _dead:
        pytest.fail("no further child process after %s" % _dead[0])
    env = {k: v for k, v in os.environ.items() if k != "FOTG_PIPE_QUEUES"}
    env["GPU_MAX_HW_QUEUES"] = str(budget)
    try:
        r = subprocess.run([sys.executable, CHILD, which], env=env, timeout=300, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    except subprocess.TimeoutExpired:
        _dead.append("%s hit its timeout" % which)
        pytest.fail(_dead[0])
    if r.returncode < 0 or r.returncode in (134, 139):
        _dead.append("%s died (exit status %d): %s" % (which, r.returncode, r.stderr[-2000:]))
        pytest.fail(_dead[0])
    assert r.returncode == 0, r.stderr[-4000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    assert len(line) == 1, r.stdout[-2000:]
    res = json.loads(line[0][7:])
    res["stderr"] = r.stderr
    assert res["budget_env"] == str(budget)
    return res


@pytest.fixture(scope="module")
def budget4():
    return run_child("budget4", 4)


@pytest.fixture(scope="module")
def budget16():
    return run_child("budget16", 16)


def test_budget4_depth4_auto_leaves_the_normal_pool_and_overlaps(budget4):
    """Four slots on four queues: the probe's width (depth * t_alone / t_together of 8 dependent 30 us launches per slot) must reach
    3.0, midway between the 1.9 and 3.8 that profiles/ records for four streams on shared and on separate queues
    (tools/queue_probe.hip).  Measured on MI355X with GPU_MAX_HW_QUEUES=4, first pipe of a fresh process: 1.95 on the layout the
    pipe had before (FOTG_PIPE_QUEUES=normal), 3.82 at creation and 3.84 / 3.80 from probe_overlap() on the new one (auto = high);
    3.79 with high and 3.81 with split forced."""
    r = budget4["auto4"]
    print("budget 4, depth 4, auto:", r["info"], "probe", r["probe"])
    assert r["info"]["budget"] == 4
    assert r["info"]["layout"] != "normal"
    assert any(p != 0 for p in r["info"]["priorities"])
    assert r["info"]["width"] > 0          # creation measured the layout it chose
    assert r["probe"] >= 3.0
    assert "fotg_pipe_create" not in budget4["stderr"]          # no warning: every slot has a queue


@pytest.mark.parametrize("which", ["auto4", "high4", "split4"])
def test_budget4_depth4_bits(budget4, which):
    """eight submits of batch 2: every flow equal to the same pairs through one plain context"""
    r = budget4[which]
    assert len(r["bits"]) == 8 and all(r["bits"]), r
    if which == "high4":
        assert r["info"]["layout"] == "high" and len(set(r["info"]["priorities"])) == 1 and r["info"]["priorities"][0] < 0
        assert r["info"]["width"] == 0          # a forced layout is not probed at creation
    if which == "split4":
        p = r["info"]["priorities"]
        assert r["info"]["layout"] == "split" and p[0] == p[2] < 0 < p[1] == p[3]


def test_budget16_depth4_is_the_pipe_it_always_was(budget16):
    r = budget16["auto4"]
    print("budget 16, depth 4, auto:", r["info"], "probe", r["probe"])
    assert r["info"]["budget"] == 16
    assert r["info"]["layout"] == "normal" and r["info"]["priorities"] == [0, 0, 0, 0]
    assert all(r["bits"]) and len(r["bits"]) == 8


@pytest.mark.parametrize("depth", [6, 8])
def test_budget4_deeper_pipes_spread_over_two_pools(budget4, depth):
    r = budget4["auto%d" % depth]
    print("budget 4, depth %d, auto:" % depth, r["info"])
    p = r["info"]["priorities"]
    assert len(p) == depth and len(set(p)) == 2, p
    assert all(p.count(v) <= 4 for v in set(p))          # no pool holds more slots than it has queues
    assert all(r["bits"]) and len(r["bits"]) == 8


def test_probe_refuses_while_a_ticket_is_outstanding(budget4):
    r = budget4["outstanding"]
    assert r["status"] == FOTG_ERR_ARG and r["width_untouched"]
    assert r["intact"]
    assert r["probe_after_wait"] > 0
