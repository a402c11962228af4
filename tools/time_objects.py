#!/usr/bin/env python3
"""Times of the connected-component labelling, HIP events, after a warm-up, the routes alternated within one
process (rounds of A, B, C, ...; the median per route is reported with min .. max), on a batch of 64 code maps of 1920 x 1080, through
the C-ABI into outputs allocated once.  Inputs:
  realistic       the code of fit_motion on a synthetic scene: an affine camera flow, a dozen rectangles moving on their own, 1 % of
                  the pixels with a vector of their own (speckle); values = the fit's residual
  all foreground  one component per image: every reduction lands on one record
  checkerboard    at 4-connectivity: w h / 2 single-pixel components per image, the most roots possible
Routes per input: labels (labels and objects, no values) and full (labels, ids, stats, objects with values), at 8-connectivity except
the checkerboard; and, on the realistic input,
  torch           the same labelling by iterated 3 x 3 minimum propagation in torch operations, run to its fixed point (checked
                  every 16 passes) -- the only formulation available without this feature
Each call is reported against its algorithmic bytes per pixel: 1 B of code read, 4 B of label written, re-read and rewritten by the
flatten pass (13 B; the merge touches tile borders only), plus 8 B of values in the full route (21 B).  What the seven launches
move beyond that (the area entries, the labels re-read by the count, emit and reduce passes, ids) is the implementation's.
usage: python tools/time_objects.py [rounds] [n]"""
import ctypes as C
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import flowonthego_amd as F                                   # noqa: E402
from flowonthego_amd.oflow import _ptr, _stream                # noqa: E402
from time_bidir import timed                                  # noqa: E402

WINDOW_MS = 200.0
BIG = float(1 << 24)


def realistic(n, w, h):
    g = torch.Generator(device="cuda").manual_seed(16)
    ys, xs = torch.meshgrid(torch.arange(h, device="cuda", dtype=torch.float32), torch.arange(w, device="cuda", dtype=torch.float32), indexing="ij")
    flow = torch.stack([0.002 * xs - 0.004 * ys + 1.5, 0.003 * xs + 0.001 * ys - 2.0], -1)[None].repeat(n, 1, 1, 1)
    for i in range(n):
        for k in range(12):
            rw, rh = 60 + (37 * k + 11 * i) % 240, 40 + (53 * k + 7 * i) % 160
            x0, y0 = (131 * k + 17 * i) % (w - rw), (89 * k + 29 * i) % (h - rh)
            flow[i, y0:y0 + rh, x0:x0 + rw] = torch.tensor([6.0 - k, k - 5.5], device="cuda")
    speckle = torch.rand((n, h, w), device="cuda", generator=g) < 0.01
    flow[speckle] += 8.0
    return flow.contiguous()


def torch_labels(code, passes=16):
    n, h, w = code.shape
    fg = code == 1
    lin = torch.arange(h * w, device="cuda", dtype=torch.float32).reshape(1, h, w).expand(n, h, w)
    lab = torch.where(fg, lin, BIG)
    total = 0
    while True:
        prev = lab
        for _ in range(passes):
            lab = torch.where(fg, -torch.nn.functional.max_pool2d(-lab[:, None], 3, 1, 1)[:, 0], BIG)
        total += passes
        if torch.equal(lab, prev):
            return lab, total


def case(w, h, n, rounds):
    L, st_ = F.lib(), _stream(torch.device("cuda", 0))
    flow = realistic(n, w, h)
    _, code_r, res = F.fit_motion(flow, code=True, residual=True)
    del flow
    ys, xs = torch.meshgrid(torch.arange(h, device="cuda"), torch.arange(w, device="cuda"), indexing="ij")
    inputs = {"realistic": (code_r, 8), "all foreground": (torch.ones_like(code_r), 8),
              "checkerboard": ((((xs + ys) % 2) == 0).to(torch.uint8)[None].repeat(n, 1, 1).contiguous(), 4)}
    mo = 256
    obj = torch.empty((n, mo, 11), dtype=torch.int64, device="cuda")
    lab = torch.empty((n, h, w), dtype=torch.int32, device="cuda")
    ids = torch.empty((n, h, w), dtype=torch.int32, device="cuda")
    st = torch.empty((n, 4), dtype=torch.int64, device="cuda")

    def call(code, conn, full):
        assert L.fotg_label_components(0, n, _ptr(code), w, h, 2, conn, _ptr(res) if full else None, 1, mo, _ptr(lab), _ptr(ids) if full else None,
                                       _ptr(obj), _ptr(st) if full else None, st_) == 0

    variants = {}
    for name, (code, conn) in inputs.items():
        variants[name + " labels"] = lambda code=code, conn=conn: call(code, conn, False)
        variants[name + " full"] = lambda code=code, conn=conn: call(code, conn, True)
    passes = {}

    def torch_route():
        passes["n"] = torch_labels(code_r)[1]
    variants["realistic torch"] = torch_route
    reps = {}
    for k, fn in variants.items():                           # warm-up (first-call allocations, code object loads), then the window's size
        fn()
        fn()
        torch.cuda.synchronize()
        reps[k] = max(1 if "torch" in k else 3, math.ceil(WINDOW_MS / timed(fn, 1 if "torch" in k else 3)))
    t = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            t[k].append(timed(fn, reps[k]))
    med = {k: statistics.median(v) for k, v in t.items()}
    px = n * h * w
    print("%d x %dx%d code maps, max_objects %d" % (n, w, h, mo))
    for k in variants:
        note = ""
        if "torch" not in k:
            by = 13 + (8 if k.endswith("full") else 0)
            note = "   %.0f GB/s of %d B per pixel" % (px * by / med[k] / 1e6, by)
        else:
            note = "   %d passes" % passes["n"]
        print("  %-24s %9.4f ms   (min %.4f .. max %.4f, %d calls per window)%s" % (k, med[k], min(t[k]), max(t[k]), reps[k], note), flush=True)
    call(code_r, 8, True)
    torch.cuda.synchronize()
    print("  realistic: %s components, %s foreground pixels in image 0; worst case / realistic (full): %.2f"
          % (st[0, 1].item(), st[0, 0].item(), max(med[k] for k in med if k.endswith("full")) / med["realistic full"]))
    ref, _ = torch_labels(code_r[:1])
    same = torch.equal(torch.where(ref[0] == BIG, -1, ref[0].to(torch.int32)).to(torch.int32), lab[0])
    print("  torch labels == fotg labels on image 0: %s" % same)


if __name__ == "__main__":
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    case(1920, 1080, n, rounds)
