"""Every entry point of include/fotg.h that takes a stream is held to what its header promises: it is asynchronous on that stream,
it takes its inputs in the stream's order, and what follows it on the stream owns its outputs.  The rows are those of
tests/stream_cases.py (tests/test_stream_cases.py holds them to the header); the expected bytes are the same call's own bytes on
the current stream, synchronised, which the add-ons' own tests pin against their restatements.

run_ordered(row), on a fresh non-blocking stream S and without any wait on the host: a delay kernel and an event `gate`; sentinels
under the outputs; X <- A, the call, a clone of its outputs; X <- B, the call, a clone; sentinels over X and the outputs.  X holds B
and the null stream is idle while all of this is enqueued, so a step of the call that runs on stream 0 reads B where A is expected
or is overwritten by the sentinels; the second call meets the stream-ordered memory the first one dirtied; the clone and the
overwriting of X right behind the call meet a forked stream that is not joined; and `gate` is still pending when the last enqueue
returns unless something waited on the host.  The delay is ten times (at least 5 ms) the host time of a rehearsal of the same enqueue on the
current stream (the margin is for the jitter of a shared host), from which the expected bytes are taken.  If `pending` fails, either
the entry point waited on the host or the delay was too short: read the entry point; nothing is retried.

The harness is tested first, on rows of plain torch: it flags an op on the default stream, an accumulator or an output zeroed on the
default stream, a fork that is not joined and a host wait, and passes the correct one.

A. every row through run_ordered.  B. per fotg_*.hip file, its rows from one thread on two streams at once, four rounds.  C. one
fresh child process (tests/streams_child.py): eight host threads with a stream each walk the add-on rows while a ninth flips the
two process-wide knobs.  D. fused calls on two streams against one context while its next batch is computed on a third.

Measured once on an MI355X (_sleep: 2.4e6 cycles per ms), per row of A: the rehearsed host time in ms / the delay in ms / the wall
time of the case in s.
  calc_batch 0.34/5.0/0.21; calc_batch_u8 0.34/5.0/0.13; calc_sequence 0.31/5.0/0.13; calc_sequence_u8 0.34/5.0/0.13;
  calc_bidir 0.53/5.3/0.13; calc_bidir_u8 0.51/5.1/0.13; calc_sequence_bidir 0.46/5.0/0.13;
  calc_sequence_bidir_u8 0.47/5.0/0.13; calc_batch_fused_cglobal 0.22/5.0/0.13; calc_batch_sor_pipe 0.31/5.0/0.34;
  calc_batch_sor_stream 0.32/5.0/0.39; calc_batch_level_pipe 0.30/5.0/0.08; pipe_submit 0.33/5.0/0.13;
  pipe_submit_u8 0.31/5.0/0.12; pipe_submit_ex 0.33/5.0/0.12; upsample_crop 0.07/5.0/0.01; gradient_magnitude 0.09/5.0/0.01;
  gradient_magnitude_u8 0.11/5.0/0.01; flow_color 0.13/5.0/0.01; flow_color_own_keys 0.12/5.0/0.01;
  upsample_crop_color_own_keys 0.11/5.0/0.01; upsample_crop_color 0.15/5.0/0.01; fb_check 0.15/5.0/0.01;
  upsample_crop_fb_check 0.20/5.0/0.01; upsample_crop_warp 0.28/5.0/0.06; warp 0.23/5.0/0.01; warp_u8 0.20/5.0/0.01;
  upsample_crop_warp_u8 0.27/5.0/0.11; interp 0.32/5.0/0.01; interp_u8 0.31/5.0/0.01; upsample_crop_interp 0.41/5.0/0.15;
  upsample_crop_interp_u8 0.39/5.0/0.09; flow_chain 0.21/5.0/0.01; track_points 0.21/5.0/0.01;
  upsample_crop_flow_chain 0.23/5.0/0.01; upsample_crop_track_points 0.23/5.0/0.01; fit_motion 0.37/5.0/0.02;
  upsample_crop_fit_motion 0.38/5.0/0.01; motion_flow 0.07/5.0/0.02; motion_layers 0.53/5.3/0.03;
  upsample_crop_motion_layers 0.49/5.0/0.01; label_components 0.31/5.0/0.14; temporal_filter 0.26/5.0/0.02;
  temporal_filter_u8 0.26/5.0/0.01; upsample_crop_temporal_filter 0.36/5.0/0.12;
  upsample_crop_temporal_filter_u8 0.42/5.0/0.23; flow_filter 0.25/5.0/0.03; flow_filter_five_buffers 0.23/5.0/0.01;
  flow_filter_u8 0.23/5.0/0.01; upsample_crop_flow_filter 0.35/5.0/0.06; upsample_crop_flow_filter_u8 0.34/5.0/0.04;
  block_motion 0.26/5.0/0.01; upsample_crop_block_motion 0.30/5.0/0.10; object_overlap 0.25/5.0/0.16;
  upsample_crop_object_overlap 0.21/5.0/0.07; object_links 0.13/5.0/0.02; object_tracks 0.17/5.0/0.01;
  motion_histograms 0.19/5.0/0.01; upsample_crop_motion_histograms 0.18/5.0/0.01; motion_blur 0.30/5.0/0.12;
  upsample_crop_motion_blur 0.32/5.0/0.04; plate 0.33/5.0/0.01; plate_u8 0.30/5.0/0.01; plate_motion 0.30/5.0/0.01;
  plate_motion_u8 0.33/5.0/0.01; upsample_crop_plate 0.41/5.0/0.12; upsample_crop_plate_u8 0.48/5.0/0.23;
  subtract 0.33/5.0/0.05; erase 0.31/5.0/0.01; subtract_u8 0.31/5.0/0.01; erase_u8 0.30/5.0/0.01;
  subtract_motion 0.32/5.0/0.01; erase_motion 0.31/5.0/0.01; subtract_motion_u8 0.32/5.0/0.01; erase_motion_u8 0.30/5.0/0.01;
  upsample_crop_subtract 0.40/5.0/0.04; upsample_crop_erase 0.37/5.0/0.04; upsample_crop_subtract_u8 0.40/5.0/0.06;
  upsample_crop_erase_u8 0.40/5.0/0.06; morph 0.12/5.0/0.03; fill 0.21/5.0/0.01; fill_u8 0.19/5.0/0.01;
  fill_flow_fused 0.16/5.0/0.01
Every row: both snapshots right, the gate pending behind the first call, every output of the first call on the sentinels (but the
one row of BEDS_MISSED); behind the last enqueue the gate had passed for exactly the 49 rows that take stream-ordered memory (the
HOST_WAIT entry points but their rows of NO_POOL).  B: every file below 0.2 s (fotg_capi.hip 0.16 s); C: 4.4 s (68 rows, 1632 calls,
634 knob flips, no mismatch, no exception); D: 0.09 s; the whole file 10.6 s."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

import stream_cases as SC
from test_gpu_warp import same_bits

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CHILD = os.path.join(HERE, "streams_child.py")
MIN_DELAY_MS = 5.0                      # a floor under ten times a host time of a few hundredths of a millisecond (it only lengthens)
SENTINEL = 0x7F                        # as float32 3.4e38: an accumulation on top of it shows

# Entry points whose header documents a host wait: entry point -> the header's line.  Only the `pending` assertion behind the LAST
# enqueue is dropped for them; that the gate is still pending behind the FIRST call is asserted for every row.  One cause, read in
# the entry points and measured: they take the memory of the call with hipMallocAsync and return it with hipFreeAsync on `stream`
# (host_call.h's Scratch) and do nothing else on the host; the runtime's hipMallocAsync blocks the calling thread when it would reuse
# a block whose hipFreeAsync on that stream has not executed yet.  malloc + free alone on a busy stream: 0.07 ms, the gate pending;
# the same twice: 20 ms = the delay, the gate passed; a larger second size, or one allocation used twice: 0.03 ms, pending.
POOL_WAIT = ("include/fotg.h, STREAM-ORDERED MEMORY: \"A further call on the same stream may wait ON THE HOST until the stream has reached "
             "the earlier call's free\"")
HOST_WAIT = {name: POOL_WAIT for name in (
    "fotg_warp", "fotg_warp_u8", "fotg_upsample_crop_warp", "fotg_upsample_crop_warp_u8",
    "fotg_interp", "fotg_interp_u8", "fotg_upsample_crop_interp", "fotg_upsample_crop_interp_u8",
    "fotg_fit_motion", "fotg_upsample_crop_fit_motion", "fotg_motion_layers", "fotg_upsample_crop_motion_layers", "fotg_label_components",
    "fotg_temporal_filter", "fotg_temporal_filter_u8", "fotg_upsample_crop_temporal_filter", "fotg_upsample_crop_temporal_filter_u8",
    "fotg_flow_filter", "fotg_flow_filter_u8", "fotg_upsample_crop_flow_filter", "fotg_upsample_crop_flow_filter_u8",
    "fotg_block_motion", "fotg_upsample_crop_block_motion", "fotg_motion_blur", "fotg_upsample_crop_motion_blur",
    "fotg_plate", "fotg_plate_u8", "fotg_plate_motion", "fotg_plate_motion_u8", "fotg_upsample_crop_plate", "fotg_upsample_crop_plate_u8",
    "fotg_subtract", "fotg_subtract_u8", "fotg_subtract_motion", "fotg_subtract_motion_u8", "fotg_upsample_crop_subtract",
    "fotg_upsample_crop_subtract_u8", "fotg_erase", "fotg_erase_u8", "fotg_erase_motion", "fotg_erase_motion_u8", "fotg_upsample_crop_erase",
    "fotg_upsample_crop_erase_u8", "fotg_fill", "fotg_fill_u8", "fotg_flow_color", "fotg_upsample_crop_color")}

# rows of a HOST_WAIT entry point that take no stream-ordered memory (the colour calls with `stats`: the keys are the caller's buffer)
NO_POOL = ("flow_color", "upsample_crop_color")
# Every output of the first call lies on memory the harness filled with sentinels behind the gate (torch's caching allocator hands the
# blocks it was just given back to the binding's torch.empty), asserted per row; the rows for which it does not hold, with the reason
BEDS_MISSED = {"fill_flow_fused": "a composition: fotg_upsample_crop's output, of the same size, takes the block meant for fotg_fill's"}

_state = {}


@pytest.fixture(scope="module", autouse=True)
def _module():
    t0 = time.perf_counter()
    yield
    torch.cuda.synchronize()
    SC.close_all()
    _state.clear()
    print("\n[streams] the whole file: %.1f s" % (time.perf_counter() - t0))


def cycles_per_ms():
    """torch.cuda._sleep calibrated once between two events"""
    if "cycles" not in _state:
        torch.cuda._sleep(1000)
        torch.cuda.synchronize()
        n = 20_000_000
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch.cuda._sleep(n)
        e1.record()
        torch.cuda.synchronize()
        _state["cycles"] = n / e0.elapsed_time(e1)
        print("\n[streams] _sleep: %.0f cycles per ms" % _state["cycles"])
    return _state["cycles"]


def delay(ms):
    torch.cuda._sleep(int(max(ms, 0.05) * cycles_per_ms()))


def upload(arrays):
    return [torch.from_numpy(a).cuda() for a in arrays]


def same(a, b):
    """byte for byte: test_gpu_warp.same_bits on the tensors' bytes (every dtype has them; torch compares few unsigned ones)"""
    return a.shape == b.shape and a.dtype == b.dtype and same_bits(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def smear(t):
    """the sentinel over every byte of t, on the current stream"""
    if t.is_contiguous() and t.dim() > 0:
        t.view(torch.uint8).fill_(SENTINEL)
    else:
        t.fill_(1)


def clones(outs):
    return [o.clone() for o in outs]


def enqueue(row, X, xa, xb, slot, pause=None, beds=None, gate=None):
    """steps of run_ordered behind the gate, on the current stream: -> (snap1, snap2).  pause: called after each clone (the rehearsal
    synchronises there); beds: the shapes and types of the outputs, to lay sentinels under them"""
    if beds:
        under = [torch.empty(shape, dtype=dtype, device="cuda") for shape, dtype in beds]       # what the caching allocator hands to the
        for u in under:                                                                         # binding's torch.empty next
            smear(u)
        ptrs = {u.data_ptr() for u in under}
        del under, u
    snaps, outs, early = [], [], []
    for src in (xa, xb):
        for x, s in zip(X, src):
            x.copy_(s, non_blocking=True)
        o = row.call(X, slot)
        outs.append(o)
        snaps.append(clones(o))
        if gate is not None:
            early.append(not gate.query())                     # still pending behind this call?
        if pause:
            pause()
    reused = sum(o.data_ptr() in ptrs for o in outs[0]) if beds else 0
    for x in X:
        smear(x)
    for o in outs:
        for t in o:
            smear(t)
    return snaps[0], snaps[1], (reused, early)


class counting:
    """counts the calls of one entry point of the loaded library while the block runs"""

    def __init__(self, entry):
        self.entry, self.n = entry, 0

    def __enter__(self):
        import flowonthego_amd as F
        self.lib, self.fn = F.lib(), getattr(F.lib(), self.entry)

        def counted(*a):
            self.n += 1
            return self.fn(*a)
        setattr(self.lib, self.entry, counted)
        return self

    def __exit__(self, *exc):
        setattr(self.lib, self.entry, self.fn)


def expected(row):
    """dict(want_a, want_b: the bytes of the row's outputs on the current stream, synchronised; host_ms: the host time of the
    rehearsed enqueue; beds), computed once per row and shared by the tests"""
    key = ("expected", row.name)
    if key in _state:
        return _state[key]
    A, B = row.build()
    xa, xb = upload(A), upload(B)
    X = [b.clone() for b in xb]
    torch.cuda.synchronize()
    import flowonthego_amd as F
    row.call(xa, 0)                                            # contexts, code objects and the pool's first blocks: not timed
    torch.cuda.synchronize()
    launches = F.lib().fotg_debug_counter(row.counter.encode()) if row.counter else 0
    with counting(row.entry) as reached:
        row.call(xa, 0)
    torch.cuda.synchronize()
    assert reached.n >= 1, "%s does not reach %s" % (row, row.entry)
    if row.counter:                                            # the solver variant the row is named after is the one that ran
        assert F.lib().fotg_debug_counter(row.counter.encode()) > launches, "%s: no launch counted by %s" % (row, row.counter)
    waited = [0.0]

    def pause():
        t = time.perf_counter()
        torch.cuda.synchronize()
        waited[0] += time.perf_counter() - t
    t0 = time.perf_counter()
    s1, s2, _ = enqueue(row, X, xa, xb, 0, pause)
    host_ms = (time.perf_counter() - t0 - waited[0]) * 1e3
    torch.cuda.synchronize()
    if row.settle:
        row.settle(0)
    want_a, want_b = s1, s2
    assert len(want_a) == len(want_b) >= 1 and all(a.shape == b.shape and a.dtype == b.dtype for a, b in zip(want_a, want_b)), row
    assert any(not same(a, b) for a, b in zip(want_a, want_b)), "%s: A and B give the same bytes, the row can detect nothing" % row
    _state[key] = dict(want_a=want_a, want_b=want_b, host_ms=host_ms, beds=[(tuple(t.shape), t.dtype) for t in s1], xa=xa, xb=xb)
    return _state[key]


def forget(row):
    _state.pop(("expected", row.name), None)


def matches(snaps, want):
    return [len(snaps) == len(want)] + [same(s, w) for s, w in zip(snaps, want)]


def run_ordered(row):
    """-> dict(first, second: per output, whether the snapshot behind the call on A / on B has the expected bytes; pending: whether
    the gate was still pending when the last enqueue returned; host_ms, delay_ms, wall_s, reused)"""
    t_wall = time.perf_counter()
    e = expected(row)
    xa, xb = e["xa"], e["xb"]
    X = [b.clone() for b in xb]                                # the persistent inputs hold B
    delay_ms = max(10.0 * e["host_ms"], MIN_DELAY_MS)
    cycles_per_ms()
    torch.cuda.synchronize()
    S = torch.cuda.Stream()
    gate = torch.cuda.Event()
    with torch.cuda.stream(S):
        delay(delay_ms)
        gate.record(S)
        s1, s2, (reused, early) = enqueue(row, X, xa, xb, 0, beds=e["beds"], gate=gate)
    pending = not gate.query()
    S.synchronize()
    if row.settle:
        row.settle(0)
    res = dict(first=matches(s1, e["want_a"]), second=matches(s2, e["want_b"]), pending=pending, pending_first=early[0], host_ms=e["host_ms"],
               delay_ms=delay_ms, reused="%d/%d" % (reused, len(s1)), on_sentinels=reused == len(s1))
    torch.cuda.synchronize()
    res["wall_s"] = time.perf_counter() - t_wall
    print("\n[streams] %-40s host %.2f ms, delay %.1f ms, wall %.2f s, outputs on sentinels %s, pending %s / %s" % (
        row.name, res["host_ms"], delay_ms, res["wall_s"], res["reused"], early[0], pending))
    return res


def assert_ordered(row):
    res = run_ordered(row)
    assert all(res["first"]), "%s: behind the call on A the outputs %s do not hold the bytes of the call on A" % (row, res["first"])
    assert all(res["second"]), "%s: behind the second call, on B, the outputs %s do not hold the bytes of the call on B" % (row, res["second"])
    late = "the gate had passed when the %s enqueue returned: either %s waited on the host or the delay of %.1f ms (ten times the rehearsed %.2f ms) was too short -- read the entry point"
    assert res["pending_first"], "%s: " % row + late % ("first call's", row.entry, res["delay_ms"], res["host_ms"])
    if row.entry in HOST_WAIT and row.name not in NO_POOL:
        assert not res["pending"], ("%s: the gate was still pending behind the second call: the runtime no longer waits on the host there -- "
                                    "take %s out of HOST_WAIT and the wait out of include/fotg.h" % (row, row.entry))
    else:
        assert res["pending"], "%s: " % row + late % ("last", row.entry, res["delay_ms"], res["host_ms"])
    if row.name not in BEDS_MISSED:
        assert res["on_sentinels"], "%s: only %s outputs of the first call lay on the sentinels" % (row, res["reused"])


# ---- the harness itself: rows of plain torch ----------------------------------------------------------------------------------------
class Fake:
    entry, file, core, settle, counter = "fake", None, False, None, None

    def __init__(self, name, call):
        self.name, self.call = name, call

    def build(self):
        rng = np.random.default_rng(1)
        return [rng.standard_normal((257, 300)).astype(np.float32)], [rng.standard_normal((257, 300)).astype(np.float32)]

    def __repr__(self):
        return self.name


class counting_nothing:
    def __init__(self, entry):
        self.n = 1

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        pass


def accumulate(x):
    """the op of every fake, as it should be: an accumulator zeroed and added to on the current stream"""
    acc = torch.empty_like(x)
    acc.zero_()
    acc.add_(x, alpha=2.0)
    return acc


def fake_good(x, slot):
    return (accumulate(x[0]),)


def fake_default_stream(x, slot):
    with torch.cuda.stream(torch.cuda.default_stream()):
        return (accumulate(x[0]),)


def fake_accumulator_zeroed_on_default(x, slot):
    """a persistent accumulator (the memory a stream-ordered pool hands out again) whose zeroing alone runs on the default stream"""
    acc = _state.setdefault("fake_acc", torch.zeros_like(x[0]))
    with torch.cuda.stream(torch.cuda.default_stream()):
        acc.zero_()
    acc.add_(x[0], alpha=2.0)
    return (acc.clone(),)


def fake_output_zeroed_on_default(x, slot):
    acc = torch.empty_like(x[0])
    with torch.cuda.stream(torch.cuda.default_stream()):
        acc.zero_()
    acc.add_(x[0], alpha=2.0)
    return (acc,)


def fake_fork_not_joined(x, slot):
    here, side = torch.cuda.current_stream(), _state.setdefault("fake_side", torch.cuda.Stream())
    out = torch.empty_like(x[0])
    side.wait_stream(here)
    with torch.cuda.stream(side):
        delay(0.2)
        out.copy_(accumulate(x[0]))
    return (out,)


def fake_host_wait(x, slot):
    out = accumulate(x[0])
    torch.cuda.current_stream().synchronize()
    return (out,)


def run_fake(name, call, monkeypatch):
    """the expected bytes are those of the correct op; then the row's call is the one under test"""
    monkeypatch.setitem(globals(), "counting", counting_nothing)
    row = Fake(name, fake_good)
    try:
        expected(row)
        row.call = call
        return run_ordered(row)
    finally:
        forget(row)
        _state.pop("fake_acc", None)


def test_the_harness_passes_a_correct_row(monkeypatch):
    res = run_fake("good", fake_good, monkeypatch)
    assert all(res["first"]) and all(res["second"]) and res["pending"], res


@pytest.mark.parametrize("name,call,where", [
    ("default-stream", fake_default_stream, "first"),
    ("accumulator-zeroed-on-default", fake_accumulator_zeroed_on_default, "second"),
    ("output-zeroed-on-default", fake_output_zeroed_on_default, "first"),
    ("fork-not-joined", fake_fork_not_joined, "first"),
    ("host-wait", fake_host_wait, "pending")])
def test_the_harness_flags_a_bad_row(name, call, where, monkeypatch):
    """each slip is flagged where the module's docstring says it is; the bytes are wrong, nothing faults"""
    res = run_fake(name, call, monkeypatch)
    if where == "pending":
        assert not res["pending"] and all(res["first"]) and all(res["second"]), res
    else:
        assert not all(res[where]), res
        assert res["pending"], res


# ---- A -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", SC.ROWS, ids=[r.name for r in SC.ROWS])
def test_inputs_pending_on_a_side_stream(row):
    assert_ordered(row)


# ---- B -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("file", SC.files())
def test_two_streams_at_once(file):
    """the rows of one file, each from one host thread on two streams at once: a delay ahead on both, so that the work piles up and
    then runs side by side; four rounds of the call on A on one stream and on B on the other (a core row: a context per stream)"""
    cycles_per_ms()
    for row in [r for r in SC.ROWS if r.file == file]:
        t0 = time.perf_counter()
        e = expected(row)
        X1, X2 = [a.clone() for a in e["xa"]], [b.clone() for b in e["xb"]]
        if row.core:
            row.call(X2, 1)                                    # the second slot's context, before anything is pending
        torch.cuda.synchronize()
        S1, S2 = torch.cuda.Stream(), torch.cuda.Stream()
        for S in (S1, S2):
            with torch.cuda.stream(S):
                delay(20.0 * e["host_ms"])
        snaps1, snaps2 = [], []
        for _ in range(4):
            with torch.cuda.stream(S1):
                snaps1.append(clones(row.call(X1, 0)))
            with torch.cuda.stream(S2):
                snaps2.append(clones(row.call(X2, 1)))
        S1.synchronize()
        S2.synchronize()
        if row.settle:
            row.settle(0), row.settle(1)
        for k in range(4):
            assert all(matches(snaps1[k], e["want_a"])), (row, "A", k, matches(snaps1[k], e["want_a"]))
            assert all(matches(snaps2[k], e["want_b"])), (row, "B", k, matches(snaps2[k], e["want_b"]))
        print("\n[streams] two streams %-40s %.2f s" % (row.name, time.perf_counter() - t0))


# ---- C -------------------------------------------------------------------------------------------------------------------------------
def test_host_threads_share_the_add_ons():
    """one fresh process, so that the first use of every kernel's dynamic-LDS opt-in, the code objects and the stream-ordered pool
    are raced, not warm: eight host threads with a stream each walk the add-on rows in their own order for three rounds while a
    ninth flips fotg_motion_ending and fotg_plate_rows; the serial results are computed afterwards in the same process"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    try:
        r = subprocess.run([sys.executable, CHILD], timeout=600, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    except subprocess.TimeoutExpired:
        pytest.fail("the child hit its timeout")
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    assert len(line) == 1, r.stdout[-2000:]
    res = json.loads(line[0][7:])
    print("\n[streams] child: %.1f s, %d rows, %d calls, knob flips %d" % (time.perf_counter() - t0, res["rows"], res["calls"], res["flips"]))
    assert res["rows"] == len(SC.ADDON_ROWS) and res["calls"] == 8 * 3 * res["rows"] and res["flips"] > 0
    assert res["knobs_restored"], res
    assert res["mismatches"] == {} and res["exceptions"] == {}, (res["mismatches"], res["exceptions"])


# ---- D -------------------------------------------------------------------------------------------------------------------------------
def test_fused_calls_share_one_context_across_streams():
    """the video loop's steady state: the fused warp, motion fit and flow filling of one batch on two streams against the SAME
    context while fotg_calc_batch of that context's next batch runs on a third.  include/fotg.h forbids none of it: the fused entry
    points and fotg_upsample_crop take the coarse flow as an argument and read the context's geometry alone."""
    ctx = SC.fused_ctx()
    rows = (SC.WARP_FUSED, SC.FIT_FUSED, SC.FILL_FLOW_FUSED)
    es = [expected(r) for r in rows]
    I0, I1 = upload(SC.pairs(SC.FUSED_H, SC.FUSED_W, (311, 312)))
    cycles_per_ms()
    want_flow = ctx.calc_batch(I0, I1).clone()
    torch.cuda.synchronize()
    S1, S2, S3 = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream()
    for S in (S1, S2):
        with torch.cuda.stream(S):
            delay(20.0 * sum(e["host_ms"] for e in es))
    got, flows = [], []
    for k in range(3):
        for j, (row, e) in enumerate(zip(rows, es)):
            with torch.cuda.stream((S1, S2)[(j + k) % 2]):
                which = "xa" if (j + k) % 2 == 0 else "xb"
                got.append((row, which, clones(row.call(e[which], 0))))
        with torch.cuda.stream(S3):
            flows.append(ctx.calc_batch(I0, I1).clone())
    for S in (S1, S2, S3):
        S.synchronize()
    assert not ctx.take_stall()
    for row, which, snaps in got:
        want = expected(row)["want_a" if which == "xa" else "want_b"]
        assert all(matches(snaps, want)), (row, which, matches(snaps, want))
    for f in flows:
        assert same(f, want_flow)
