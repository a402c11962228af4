"""One fresh process of tests/test_gpu_pipe_queues.py: the hardware-queue budget has to be in the environment before the HIP runtime
loads, so the test starts this script with GPU_MAX_HW_QUEUES set and reads one JSON line from it.  Asserts nothing itself.

    python pipe_queues_child.py budget4 | budget16 | width [depth]

FOTG_PIPE_QUEUES is read at fotg_pipe_create, so one process creates its pipes under several values of it, one pipe at a time."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import flowonthego_amd as F  # noqa: E402
from conftest import synth_pair  # noqa: E402
from flowonthego_amd.oflow import OFClass  # noqa: E402
from flowonthego_amd.pipeline import FlowPipeline  # noqa: E402

H, W = 96, 160          # the frames of tests/test_gpu_pipe_tickets.py


def frames():
    """three frame pairs on the GPU and their flows from one plain context"""
    pairs = [synth_pair(H, W, seed=900 + k) for k in range(3)]
    A = torch.from_numpy(np.stack([p[0] for p in pairs])).cuda()
    B = torch.from_numpy(np.stack([p[1] for p in pairs])).cuda()
    op = F.operating_point(2, W, 1)
    ip = F.img_params(width=W, height=H, padding=op.patch_size)
    ofc = OFClass(op, ip, max_batch=3)
    ref = ofc.calc_batch(A, B).clone()
    torch.cuda.synchronize()
    ofc.close()
    return op, ip, A, B, ref


def make(fr, depth, queues):
    if queues is None:
        os.environ.pop("FOTG_PIPE_QUEUES", None)
    else:
        os.environ["FOTG_PIPE_QUEUES"] = queues
    return FlowPipeline(fr[0], fr[1], max_batch=2, depth=depth)


def bits(fr, pipe, nsubmit=8):
    """nsubmit submits of batch 2 (pairs t % 3 and (t + 1) % 3): per submit, is the flow the one of the plain context?"""
    _, _, A, B, ref = fr
    jobs = []
    for t in range(nsubmit):
        idx = torch.tensor([t % 3, (t + 1) % 3], device=A.device)
        i0, i1 = A[idx].contiguous(), B[idx].contiguous()
        torch.cuda.synchronize()
        jobs.append((idx, i0, i1) + pipe.submit(i0, i1))
    pipe.synchronize()
    return [bool(np.array_equal(out.cpu().numpy(), ref[idx].cpu().numpy())) for idx, _, _, _, out in jobs]


def case(fr, depth, queues, probe=False):
    pipe = make(fr, depth, queues)
    try:
        r = {"info": pipe.queue_info()}
        if probe:
            r["probe"] = pipe.probe_overlap()
        r["bits"] = bits(fr, pipe)
        return r
    finally:
        pipe.close()


def outstanding(fr):
    """the probe with a ticket that no host wait has settled: its status, and the ticket's flow afterwards"""
    _, _, A, B, ref = fr
    pipe = make(fr, 4, None)
    try:
        i0, i1 = A[:2].contiguous(), B[:2].contiguous()
        torch.cuda.synchronize()
        ticket, out = pipe.submit(i0, i1)
        import ctypes as C
        width = C.c_float(-1.0)
        status = F.lib().fotg_pipe_probe_overlap(pipe._h, width)
        pipe.wait(ticket, host=True)
        intact = bool(np.array_equal(out.cpu().numpy(), ref[:2].cpu().numpy()))
        after = pipe.probe_overlap()          # settled: the probe runs again
        return {"status": status, "width_untouched": width.value == -1.0, "intact": intact, "probe_after_wait": after}
    finally:
        pipe.close()


def main(which):
    fr = frames()
    res = {"budget_env": os.environ.get("GPU_MAX_HW_QUEUES")}
    if which == "budget4":
        res["auto4"] = case(fr, 4, None, probe=True)          # first: the layout a process gets for its first pipe
        res["outstanding"] = outstanding(fr)
        res["high4"] = case(fr, 4, "high")
        res["split4"] = case(fr, 4, "split")
        res["auto6"] = case(fr, 6, None)
        res["auto8"] = case(fr, 8, None)
    elif which == "budget16":
        res["auto4"] = case(fr, 4, None, probe=True)
    elif which == "width":          # the figures of the test's docstring: the layout in FOTG_PIPE_QUEUES as the caller set it
        res["case"] = case(fr, int(sys.argv[2]) if len(sys.argv) > 2 else 4, os.environ.get("FOTG_PIPE_QUEUES"), probe=True)
    else:
        raise SystemExit("unknown case %r" % which)
    print("RESULT " + json.dumps(res), flush=True)


if __name__ == "__main__":
    main(sys.argv[1])
