#!/usr/bin/env python3
"""Times of the global-motion fit, HIP events, after a warm-up, the routes alternated within one process
(rounds of A, B, C, ...; the median per route is reported), on a batch of 64 flows of 1920 x 1080 (the affine model; the passes do
the same work for every model).  Every timed window is a few hundred milliseconds of back-to-back calls through the C-ABI into
outputs allocated once.  Routes: form (dense: fotg_fit_motion on full-resolution flows that already exist; fused:
fotg_upsample_crop_fit_motion on the context's coarse flows) x iters (0, 3) x final pass (none: params only; final: code, residual
and counts) x ending of the reduction (atomic: one 64-bit integer atomic per workgroup and sum; fold: per-workgroup partials and a
second launch), and
  torch    the same algorithm in torch operations: masked float64 sums and torch.linalg.solve per round, no final pass
Each pass is reported against its algorithmic bytes: the flows once, 8 B per pixel (1.06 GB for the batch, more than the
last-level cache holds: every pass streams from HBM), plus 9 B per pixel written by the final pass.
usage: python tools/time_motion.py [rounds] [n]"""
import ctypes as C
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import flowonthego_amd as F                                   # noqa: E402
from flowonthego_amd.oflow import OFClass, _ptr, _stream      # noqa: E402
from time_bidir import timed                                  # noqa: E402

WINDOW_MS = 200.0


def torch_route(flow, iters, thresh=1.0):
    n, h, w, _ = flow.shape
    x = torch.arange(w, device="cuda", dtype=torch.float64)[None, None, :]
    y = torch.arange(h, device="cuda", dtype=torch.float64)[None, :, None]
    u, v = flow[..., 0].double(), flow[..., 1].double()
    known = (u.abs() <= 4096) & (v.abs() <= 4096)
    sel, P = known, None
    for _ in range(iters + 1):
        m = sel.double()
        s = lambda a: a.sum(dim=(1, 2))
        mx, my = m * x, m * y
        A = torch.stack([torch.stack([s(mx * x), s(mx * y), s(mx)], -1), torch.stack([s(mx * y), s(my * y), s(my)], -1),
                         torch.stack([s(mx), s(my), s(m)], -1)], -2)
        mu, mv = torch.where(sel, u, 0.0), torch.where(sel, v, 0.0)
        b = torch.stack([torch.stack([s(mu * x), s(mu * y), s(mu)], -1), torch.stack([s(mv * x), s(mv * y), s(mv)], -1)], -1)
        P = torch.linalg.solve(A, b)                                           # (n, 3, 2)
        du = u - (P[:, 0, 0, None, None] * x + P[:, 1, 0, None, None] * y + P[:, 2, 0, None, None])
        dv = v - (P[:, 0, 1, None, None] * x + P[:, 1, 1, None, None] * y + P[:, 2, 1, None, None])
        sel = known & (du * du + dv * dv <= thresh * thresh)
    return P


def case(w, h, n, rounds):
    op = F.operating_point(2, w, 1)
    ofc = OFClass(op, F.img_params(width=w, height=h), max_batch=n)
    wl, hl = ofc.out_size()
    g = torch.Generator(device="cuda").manual_seed(5)
    sc = float(1 << op.finest_scale)
    ys, xs = torch.meshgrid(torch.arange(hl, device="cuda", dtype=torch.float32) * sc, torch.arange(wl, device="cuda", dtype=torch.float32) * sc, indexing="ij")
    cf = torch.stack([0.002 * xs - 0.004 * ys + 1.5, 0.003 * xs + 0.001 * ys - 2.0], -1)[None].repeat(n, 1, 1, 1)
    cf += 0.2 * torch.randn(cf.shape, device="cuda", generator=g)
    cf[:, hl // 4:hl // 2, wl // 4:3 * wl // 4] += 6.0                       # a quarter of the frame moving on its own
    cf = (cf / sc).contiguous()
    full = ofc.upsample_crop(cf)
    L, st_, th = F.lib(), _stream(ofc.device), C.c_float(1.0)
    prm = torch.empty((n, 6), dtype=torch.float64, device="cuda")
    code = torch.empty((n, h, w), dtype=torch.uint8, device="cuda")
    res = torch.empty((n, h, w, 2), device="cuda")
    st = torch.empty((n, 6), dtype=torch.int64, device="cuda")

    def dense(iters, final):
        assert L.fotg_fit_motion(0, n, _ptr(full), None, w, h, 2, iters, th, _ptr(prm), *((_ptr(code), _ptr(res), _ptr(st)) if final else (None,) * 3),
                                 None, st_) == 0

    def fused(iters, final):
        assert L.fotg_upsample_crop_fit_motion(ofc._h, n, _ptr(cf), None, 2, iters, th, _ptr(prm),
                                               *((_ptr(code), _ptr(res), _ptr(st)) if final else (None,) * 3), None, st_) == 0

    def with_ending(e, fn, *a):
        def run():
            L.fotg_motion_ending(e)
            fn(*a)
        return run

    variants = {}
    for form, fn in (("dense", dense), ("fused", fused)):
        for iters in (0, 3):
            for final in (False, True):
                for e, en in ((0, "atomic"), (1, "fold")):
                    variants["%s iters=%d %s %s" % (form, iters, "final" if final else "none", en)] = with_ending(e, fn, iters, final)
    variants["upsample_crop"] = lambda: ofc.upsample_crop(cf, out=full)
    variants["torch iters=0"] = lambda: torch_route(full, 0)
    variants["torch iters=3"] = lambda: torch_route(full, 3)
    before = L.fotg_motion_ending(-1)
    reps = {}
    for k, fn in variants.items():                           # warm-up (first-call allocations, code object loads), then the window's size
        fn()
        fn()
        torch.cuda.synchronize()
        reps[k] = max(3, math.ceil(WINDOW_MS / timed(fn, 3)))
    t = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            t[k].append(timed(fn, reps[k]))
    L.fotg_motion_ending(before)
    med = {k: statistics.median(v) for k, v in t.items()}
    gb = n * h * w * 8 / 1e9
    print("%d x %dx%d flows, affine, %.3f GB of flow per pass" % (n, w, h, gb))
    for k in variants:
        print("  %-32s %9.4f ms   (min %.4f .. max %.4f, %d calls per window)" % (k, med[k], min(t[k]), max(t[k]), reps[k]), flush=True)
    for form in ("dense", "fused"):
        for en in ("atomic", "fold"):
            t0, t3 = med["%s iters=0 none %s" % (form, en)], med["%s iters=3 none %s" % (form, en)]
            tf = med["%s iters=3 final %s" % (form, en)] - t3
            later = (t3 - t0) / 3
            print("  %s %s: round 0 %.4f ms (%.0f GB/s), a later round %.4f ms (%.0f GB/s), the final pass %.4f ms (%.0f GB/s of %.3f GB)"
                  % (form, en, t0, gb / t0 * 1e3, later, gb / later * 1e3, tf, gb * 17 / 8 / tf * 1e3, gb * 17 / 8), flush=True)
    ofc.close()


if __name__ == "__main__":
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    case(1920, 1080, n, rounds)
