"""The fresh process of tests/test_gpu_streams.py::test_host_threads_share_the_add_ons: nothing of the library has run when the
threads start, so the first use of every kernel's dynamic-LDS opt-in (host_call.h's g_lds_set), the code objects and the device's
stream-ordered pool are raced.  Eight host threads, a stream each, walk the add-on rows of tests/stream_cases.py in their own seeded
order for three rounds (even threads on input set A, odd ones on B); a ninth flips fotg_motion_ending and fotg_plate_rows between
their documented values throughout -- the header promises the same bits either way -- and restores both.  The serial results are
computed afterwards, in this process.  Prints one line, RESULT {json}: mismatches and exceptions per row.  Asserts nothing itself.

    python streams_child.py"""
import json
import os
import random
import sys
import threading

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import torch  # noqa: E402

import flowonthego_amd as F  # noqa: E402
import stream_cases as SC  # noqa: E402

THREADS, ROUNDS = 8, 3


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def main():
    rows = SC.ADDON_ROWS
    L = F.lib()
    inputs = {}
    for row in rows:                                           # host arrays to the device: torch alone, no call of the library
        A, B = row.build()
        inputs[row.name] = ([torch.from_numpy(a).cuda() for a in A], [torch.from_numpy(b).cuda() for b in B])
    torch.cuda.synchronize()
    ending, plate_rows = L.fotg_motion_ending(-1), L.fotg_plate_rows(-1)
    lock = threading.Lock()
    first = [dict() for _ in range(THREADS)]                   # per thread: row -> the outputs of round 0
    later = [[] for _ in range(THREADS)]                       # per thread: (row, device flag: a later round equals round 0)
    exceptions, calls = {}, [0]

    def worker(t):
        S = torch.cuda.Stream()
        order = list(rows)
        rng = random.Random(100 + t)
        for k in range(ROUNDS):
            rng.shuffle(order)
            for row in order:
                try:
                    with torch.cuda.stream(S):
                        outs = [o.clone() for o in row.call(inputs[row.name][t % 2], 0)]
                        if k == 0:
                            first[t][row.name] = outs
                        else:
                            flags = [(a.contiguous().view(torch.uint8) == b.contiguous().view(torch.uint8)).all() for a, b in zip(outs, first[t][row.name])]
                            later[t].append((row.name, torch.stack(flags).all()))
                    with lock:
                        calls[0] += 1
                except Exception as e:                         # counted, reported, never raised past the thread
                    with lock:
                        exceptions[row.name] = exceptions.get(row.name, 0) + 1
                        print("thread %d, %s: %r" % (t, row.name, e), file=sys.stderr)
        S.synchronize()

    stop, flips = threading.Event(), [0]

    def knobs():
        while not stop.is_set():
            L.fotg_motion_ending(flips[0] % 2)
            L.fotg_plate_rows((1, 2, 4)[flips[0] % 3])
            flips[0] += 1
            stop.wait(0.0005)

    SC.fused_ctx()                                             # (fotg_create launches nothing; the rows would race to build it)
    threads = [threading.Thread(target=worker, args=(t,)) for t in range(THREADS)]
    knob = threading.Thread(target=knobs)
    knob.start()
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    stop.set()
    knob.join()
    L.fotg_motion_ending(ending)
    L.fotg_plate_rows(plate_rows)
    restored = L.fotg_motion_ending(-1) == ending and L.fotg_plate_rows(-1) == plate_rows
    torch.cuda.synchronize()

    mismatches = {}
    for row in rows:                                           # the serial results, after the threads
        want = [[o.clone() for o in row.call(inputs[row.name][j], 0)] for j in (0, 1)]
        torch.cuda.synchronize()
        for t in range(THREADS):
            got = first[t].get(row.name)
            if got is None:
                continue
            bad = len(got) != len(want[t % 2]) or not all(same(a, b) for a, b in zip(got, want[t % 2]))
            bad += sum(1 for name, flag in later[t] if name == row.name and not bool(flag))
            if bad:
                mismatches[row.name] = mismatches.get(row.name, 0) + int(bad)
    SC.close_all()
    print("RESULT " + json.dumps(dict(rows=len(rows), calls=calls[0], flips=flips[0], mismatches=mismatches, exceptions=exceptions,
                                      knobs_restored=bool(restored))), flush=True)


if __name__ == "__main__":
    main()
