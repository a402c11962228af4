#!/usr/bin/env python3
"""Times of the binary morphology, HIP events, warm repeated calls: after a warm-up the routes are alternated
within one process (rounds of A, B, C, ...; the median per route is reported with min .. max), on 64 maps of 1920 x 1080 bytes through
the C-ABI into an out allocated once.  Maps: empty, a dozen rectangles per map plus 1 % speckle, full, 50 % noise.  Operations:
dilate r = 2, open r = 1, close r = 8 and clean_mask(1, 2).  Routes:
  morph     fotg_morph, one launch per operation (two for clean_mask)
  2 x 1     the same opening or closing as two one-stage launches through a map in memory: what fusing the stages saves
  grow      the same bytes from what there was before: grow_mask on the map for a dilation, grow_mask on the complement for an
            erosion, with the torch complement and compare counted in
  torch     the same bytes from a disc-shaped conv2d on a float copy of the map, the conversions counted in (rects only)
morph is reported against its algorithmic bytes per pixel: one byte read and one written per launch.
usage: python tools/time_morph.py [rounds] [maps] [library]     library: another build of fotg_morph (a tile of another height) to time, morph and 2 x 1 only"""
import ctypes as C
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import flowonthego_amd as F                                   # noqa: E402
from flowonthego_amd._args import _ptr, _stream               # noqa: E402
from time_bidir import timed                                  # noqa: E402

WINDOW_MS = 200.0
ERODE, DILATE = 0, 1
OPS = (("dilate 2", ((DILATE, 2),)), ("open 1", ((ERODE, 1), (DILATE, 1))), ("close 8", ((DILATE, 8), (ERODE, 8))),
       ("clean 1 2", ((ERODE, 1), (DILATE, 1), (DILATE, 2), (ERODE, 2))))


def maps(n, h, w, g):
    rects = torch.zeros((n, h, w), dtype=torch.uint8, device="cuda")
    for i in range(n):
        for _ in range(12):
            rw, rh = (int(v) for v in torch.randint(40, 200, (2,), generator=g, device="cuda"))
            x, y = int(torch.randint(0, w - rw, (1,), generator=g, device="cuda")), int(torch.randint(0, h - rh, (1,), generator=g, device="cuda"))
            rects[i, y:y + rh, x:x + rw] = 1
    rects ^= (torch.rand((n, h, w), device="cuda", generator=g) < 0.01).to(torch.uint8)
    return {"empty": torch.zeros_like(rects), "rects": rects, "full": torch.ones_like(rects),
            "noise": (torch.rand((n, h, w), device="cuda", generator=g) < 0.5).to(torch.uint8)}


def disc_kernel(r):
    yy, xx = torch.meshgrid(torch.arange(-r, r + 1), torch.arange(-r, r + 1), indexing="ij")
    return ((xx * xx + yy * yy) <= r * r).float().cuda()[None, None]


def torch_chain(x, stages):
    """zero padding: in a dilation what lies outside the frame is clear, in an erosion its complement is"""
    y = (x != 0).float()[:, None]
    for op, r in stages:
        k = disc_kernel(r)
        if op == DILATE:
            y = (torch.nn.functional.conv2d(y, k, padding=r) > 0).float()
        else:
            y = (torch.nn.functional.conv2d(1.0 - y, k, padding=r) == 0).float()
    return y[:, 0].to(torch.uint8)


def grow_chain(x, stages):
    for op, r in stages:
        x = F.grow_mask(x, r) if op == DILATE else (F.grow_mask((x == 0).to(torch.uint8), r) == 0).to(torch.uint8)
    return x


def main(rounds, n, library=None):
    w, h = 1920, 1080
    if library:
        L = C.CDLL(library)
        L.fotg_morph.restype = C.c_int
        L.fotg_morph.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                 C.c_void_p, C.c_void_p, C.c_void_p]
    else:
        L = F.lib()
    st_ = _stream(torch.device("cuda", 0))
    g = torch.Generator(device="cuda").manual_seed(41)
    x = maps(n, h, w, g)
    out, tmp = torch.empty((n, h, w), dtype=torch.uint8, device="cuda"), torch.empty((n, h, w), dtype=torch.uint8, device="cuda")

    def launch(src, stages, dst):
        ops, radii = (C.c_int * len(stages))(*(s[0] for s in stages)), (C.c_int * len(stages))(*(s[1] for s in stages))
        assert L.fotg_morph(0, n, _ptr(src), w, h, 0, len(stages), ops, radii, _ptr(dst), None, st_) == 0

    def morph(src, stages):                                   # two stages per launch
        for k in range(0, len(stages), 2):
            last = k + 2 >= len(stages)
            launch(src, stages[k:k + 2], out if last else tmp)
            src = tmp

    def singly(src, stages):                                  # one stage per launch, ping-pong
        bufs = (tmp, out) if len(stages) % 2 == 0 else (out, tmp)
        for k, s in enumerate(stages):
            launch(src, (s,), bufs[k % 2])
            src = bufs[k % 2]

    # the routes write the same bytes
    for name, stages in OPS:
        morph(x["rects"], stages)
        a = out.clone()
        singly(x["rects"], stages)
        assert torch.equal(a, out) and torch.equal(a, grow_chain(x["rects"], stages)), name
        if not library:
            assert torch.equal(a, torch_chain(x["rects"], stages)), name
    variants, launches = {}, {}
    for name, stages in OPS:
        for case in x:
            variants["%s %s morph" % (name, case)] = lambda case=case, stages=stages: morph(x[case], stages)
            launches["%s %s morph" % (name, case)] = (len(stages) + 1) // 2
            if len(stages) > 1:
                variants["%s %s 2 x 1" % (name, case)] = lambda case=case, stages=stages: singly(x[case], stages)
            if not library:
                variants["%s %s grow" % (name, case)] = lambda case=case, stages=stages: grow_chain(x[case], stages)
        if not library:
            variants["%s rects torch" % name] = lambda stages=stages: torch_chain(x["rects"], stages)
    reps = {}
    for k, fn in variants.items():                           # warm-up (first-call allocations, code object loads), then the window's size
        fn()
        fn()
        torch.cuda.synchronize()
        reps[k] = max(2, math.ceil(WINDOW_MS / timed(fn, 2))) if "torch" not in k else 2
    t = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            t[k].append(timed(fn, reps[k]))
    med = {k: statistics.median(v) for k, v in t.items()}
    print("%d maps of %dx%d%s" % (n, w, h, "; fotg_morph of %s" % library if library else ""))
    for k in variants:
        note = ""
        if k in launches:
            note = "   %.2f TB/s of %d B per pixel" % (n * w * h * 2 * launches[k] / med[k] / 1e9, 2 * launches[k])
        print("  %-26s %9.4f ms   (min %.4f .. max %.4f, %d calls per window)%s" % (k, med[k], min(t[k]), max(t[k]), reps[k], note), flush=True)
    for name, stages in OPS if not library else ():
        m = med["%s rects morph" % name]
        print("  %-10s rects: morph is %.1f x grow_mask's way, %.1f x the torch composition%s"
              % (name, med["%s rects grow" % name] / m, med["%s rects torch" % name] / m,
                 ", %.2f x two one-stage launches" % (med["%s rects 2 x 1" % name] / m) if len(stages) > 1 else ""))


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 3, int(sys.argv[2]) if len(sys.argv) > 2 else 64, sys.argv[3] if len(sys.argv) > 3 else None)
