#!/usr/bin/env python3
"""Times of the background subtraction, HIP events, after a warm-up, the routes alternated within one process
(rounds of A, B, C, ...; the median per route is reported with min .. max), on 64 frames of 1920 x 1080, 8-bit RGB and f32 gray,
against one plate on the frame grid, a pan of 6 px per frame with a slight rotation, through the C-ABI into outputs allocated once.
Routes, each at window r = 0, 1, 2, with the code alone and with all four outputs:
  motion   fotg_subtract_motion on six parameters per frame
  dense    fotg_subtract on the flows fotg_motion_flow wrote
  fused    fotg_upsample_crop_subtract on a context's coarse flows (the vectors are not the pan's)
  torch    the code map composed from public calls and torch operations: motion_flow, warp of the plate, abs, amax over the
           channels, avg_pool2d, two comparisons (code alone; 8-bit samples are rounded by the warp, so not always the same bytes)
Each route is reported against the kernel's algorithmic bytes per frame pixel: the frame, the plate's four taps gathered through L2
counted once, the vectors (8 bytes dense, half a byte fused), and the outputs (1 byte of code; 11 with diff and evidence).
usage: python tools/time_subtract.py [rounds] [frames]"""
import ctypes as C
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import flowonthego_amd as F                                   # noqa: E402
from flowonthego_amd.oflow import OFClass, _ptr, _stream       # noqa: E402
from time_bidir import timed                                  # noqa: E402
from time_plate import shot_motions                           # noqa: E402

WINDOW_MS = 200.0
LOW, HIGH = 8.0, 24.0


def torch_code(frames, plates_n, back, w, h, r):
    flows = F.motion_flow(back, w, h)
    wd, code, _ = F.warp(plates_n, flows, stats=True)
    d = (frames.float() - wd.float()).abs().reshape(frames.shape[0], h, w, -1).amax(-1)
    d = torch.where(code == 0, d, torch.zeros_like(d))
    if r:
        ok = (code == 0).float()
        m = torch.nn.functional.avg_pool2d(d[:, None], 2 * r + 1, 1, r, divisor_override=1)[:, 0]
        c = torch.nn.functional.avg_pool2d(ok[:, None], 2 * r + 1, 1, r, divisor_override=1)[:, 0]
    else:
        m, c = d, (code == 0).float()
    out = (m >= LOW * c).to(torch.uint8) + 3 * (m >= HIGH * c).to(torch.uint8)
    return torch.where(code == 0, out, code)


def main(rounds, n):
    w, h = 1920, 1080
    L, st_ = F.lib(), _stream(torch.device("cuda", 0))
    g = torch.Generator(device="cuda").manual_seed(31)
    frames = {"u8 rgb": (torch.rand((n, h, w, 3), device="cuda", generator=g) * 255).to(torch.uint8),
              "f32 gray": torch.rand((n, h, w), device="cuda", generator=g) * 255}
    plates = {k: v[:1].clone() for k, v in frames.items()}
    back = F.frame_motions(shot_motions(n, w, h))
    flows = F.motion_flow(back, w, h).contiguous()
    ofc = OFClass(F.operating_point(2, w, 1), F.img_params(width=w, height=h), max_batch=n)
    wl, hl = ofc.out_size()
    coarse = (torch.randn((n, hl, wl, 2), device="cuda", generator=g) * 2.0).contiguous()
    code = torch.empty((n, h, w), dtype=torch.uint8, device="cuda")
    diff = torch.empty((n, h, w), dtype=torch.int16, device="cuda")
    evidence = torch.empty((n, h, w, 2), dtype=torch.float32, device="cuda")
    stats = torch.empty((n, 7), dtype=torch.int64, device="cuda")

    def run(kind, src, r, full):
        fr, ch, u8 = frames[kind], 3 if kind == "u8 rgb" else 1, kind == "u8 rgb"
        tail = (None, None, C.c_float(LOW), C.c_float(HIGH), r, _ptr(code)) + ((_ptr(diff), _ptr(evidence), _ptr(stats)) if full else (None,) * 3) + (st_,)
        if src == "fused":
            fn = L.fotg_upsample_crop_subtract_u8 if u8 else L.fotg_upsample_crop_subtract
            s = fn(ofc._h, n, _ptr(coarse), _ptr(fr), ch, 1, _ptr(plates[kind]), w, h, 0, 0, None, *tail)
        else:
            fn = {("motion", True): L.fotg_subtract_motion_u8, ("motion", False): L.fotg_subtract_motion, ("dense", True): L.fotg_subtract_u8,
                  ("dense", False): L.fotg_subtract}[src, u8]
            s = fn(0, n, _ptr(fr), w, h, ch, 1, _ptr(plates[kind]), w, h, 0, 0, None, _ptr(back if src == "motion" else flows), *tail)
        assert s == 0

    variants, nbytes = {}, {}
    for kind in frames:
        el = 3 if kind == "u8 rgb" else 4
        plates_n = plates[kind].expand((n,) + tuple(plates[kind].shape[1:])).contiguous()
        for r in (0, 1, 2):
            for src, vec in (("motion", 0.0), ("dense", 8.0), ("fused", 0.5)):
                for full in (False, True):
                    name = "%s r%d %s %s" % (kind, r, src, "all" if full else "code")
                    variants[name] = lambda kind=kind, src=src, r=r, full=full: run(kind, src, r, full)
                    nbytes[name] = 2 * el + vec + (11 if full else 1)
            variants["%s r%d torch code" % (kind, r)] = lambda kind=kind, r=r, p=plates_n: torch_code(frames[kind], p, back, w, h, r)
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
    print("%d frames of %dx%d against one plate, thresholds %.0f / %.0f" % (n, w, h, LOW, HIGH))
    for k in variants:
        note = ""
        if k in nbytes:
            note = "   %.2f TB/s of %.1f B per pixel" % (n * w * h * nbytes[k] / med[k] / 1e9, nbytes[k])
            tk = k.rsplit(" ", 2)[0] + " torch code"
            if k.endswith("code") and tk in med:
                note += ", %.1f x torch" % (med[tk] / med[k])
        print("  %-28s %9.4f ms   (min %.4f .. max %.4f, %d calls per window)%s" % (k, med[k], min(t[k]), max(t[k]), reps[k], note), flush=True)
    for kind in frames:
        print("  %-10s motion, code alone: r = 2 takes %.2f x r = 0 (the halo re-evaluates 1360 positions per 1024 pixels)"
              % (kind, med["%s r2 motion code" % kind] / med["%s r0 motion code" % kind]))
        run(kind, "motion", 1, False)
        p = plates[kind].expand((n,) + tuple(plates[kind].shape[1:])).contiguous()
        same = (code == torch_code(frames[kind], p, back, w, h, 1)).float().mean().item()
        print("  %-10s the torch composition gives the kernel's code at %.4f of the pixels" % (kind, same))
    ofc.close()


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 3, int(sys.argv[2]) if len(sys.argv) > 2 else 64)
