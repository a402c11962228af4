#!/usr/bin/env python3
"""Times of the background plate, HIP events, after a warm-up, the routes alternated within one process
(rounds of A, B, C, ...; the median per route is reported with min .. max), on a 1920 x 1080 shot of K = 9 and K = 32 frames, 8-bit RGB
and f32 gray, a pan of 6 px per frame with a slight rotation, on the frame grid and on the mosaic canvas of the shot, through the
C-ABI into outputs allocated once.  Routes:
  motion r1 | r2 | r4   fotg_plate_motion with 1, 2 or 4 canvas rows (64, 128, 256 lanes) per workgroup (fotg_plate_rows)
  dense                 fotg_plate on the flows fotg_motion_flow wrote (frame grid only)
  fused                 fotg_upsample_crop_plate on a context's coarse flows (frame grid only; the vectors are not the pan's)
  torch                 the same structure composed from public calls: motion_flow, warp with codes, a NaN mask and torch.nanmedian
                        (frame grid only; the lower median for an even count, so not always the same bytes)
Each route is reported against the kernel's algorithmic bytes per canvas pixel: K samples of four taps gathered through L2 count
once each (the frame's bytes), the dense source adds 8 K bytes, and the pixel is written once.
usage: python tools/time_plate.py [rounds]"""
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

WINDOW_MS = 200.0


def shot_motions(K, w, h):
    """reference (frame 0) -> frame k: a pan of 6 px per frame to the right, 1 px down, and a rotation of 0.0004 rad per frame"""
    rows = []
    for k in range(K):
        a = 0.0004 * k
        rows.append([math.cos(a) - 1.0, -math.sin(a), 6.0 * k, math.sin(a), math.cos(a) - 1.0, 1.0 * k])
    return torch.tensor(rows, dtype=torch.float64, device="cuda")


def torch_plate(frames, motions, w, h):
    flows = F.motion_flow(motions, w, h)
    wd, code, _ = F.warp(frames, flows, stats=True)
    v = wd.float().reshape(wd.shape[0], h, w, -1)
    v = torch.where((code == 0)[..., None], v, torch.full_like(v, float("nan")))
    m = torch.nanmedian(v, dim=0).values.reshape(frames.shape[1:])
    return m.round().clamp(0, 255).to(torch.uint8) if frames.dtype == torch.uint8 else m


def case(w, h, K, rounds):
    L, st_ = F.lib(), _stream(torch.device("cuda", 0))
    g = torch.Generator(device="cuda").manual_seed(29)
    frames = {"u8 rgb": (torch.rand((K, h, w, 3), device="cuda", generator=g) * 255).to(torch.uint8),
              "f32 gray": torch.rand((K, h, w), device="cuda", generator=g) * 255}
    motions = shot_motions(K, w, h)
    canvases = {"grid": (w, h, 0, 0), "mosaic": F.mosaic_canvas(motions, w, h)}
    index = (C.c_int * K)(*range(K))
    flows = F.motion_flow(motions, w, h).contiguous()
    ofc = OFClass(F.operating_point(2, w, 1), F.img_params(width=w, height=h), max_batch=K)
    wl, hl = ofc.out_size()
    coarse = (torch.randn((K, hl, wl, 2), device="cuda", generator=g) * 2.0).contiguous()
    outs = {(kind, cv): torch.empty((1, H, W) + tuple(fr.shape[3:]), dtype=fr.dtype, device="cuda")
            for kind, fr in frames.items() for cv, (W, H, _, _) in canvases.items()}

    def run(kind, cv, src, rows=None):
        fr, ch = frames[kind], 3 if kind == "u8 rgb" else 1
        u8 = kind == "u8 rgb"
        W, H, ox, oy = canvases[cv]
        if rows:
            L.fotg_plate_rows(rows)
        tail = (None, None, 0, 1, C.c_float(0.0), None, _ptr(outs[kind, cv]), None, None, None, st_)
        if src == "fused":
            fn = L.fotg_upsample_crop_plate_u8 if u8 else L.fotg_upsample_crop_plate
            r = fn(ofc._h, 1, K, K, _ptr(coarse), _ptr(fr), ch, index, *tail)
        else:
            fn = {("motion", True): L.fotg_plate_motion_u8, ("motion", False): L.fotg_plate_motion, ("dense", True): L.fotg_plate_u8,
                  ("dense", False): L.fotg_plate}[src, u8]
            r = fn(0, 1, K, K, _ptr(fr), w, h, ch, index, _ptr(motions if src == "motion" else flows), W, H, ox, oy, *tail)
        assert r == 0

    default_rows = L.fotg_plate_rows(0)
    variants, nbytes = {}, {}
    for kind in frames:
        el = 3 if kind == "u8 rgb" else 4
        for cv in canvases:
            name = "%s, %s" % (kind, cv)
            for rows in (1, 2, 4):
                variants["%s motion r%d" % (name, rows)] = lambda kind=kind, cv=cv, rows=rows: run(kind, cv, "motion", rows)
                nbytes["%s motion r%d" % (name, rows)] = K * el + el
            if cv == "grid":
                variants[name + " dense"] = lambda kind=kind, cv=cv: run(kind, cv, "dense", default_rows)
                variants[name + " fused"] = lambda kind=kind, cv=cv: run(kind, cv, "fused", default_rows)
                variants[name + " torch"] = lambda kind=kind: torch_plate(frames[kind], motions, w, h)
                nbytes[name + " dense"] = K * (el + 8) + el
                nbytes[name + " fused"] = K * el + K // 2 + el           # a coarse vector per four pixels
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
    L.fotg_plate_rows(default_rows)
    med = {k: statistics.median(v) for k, v in t.items()}
    print("K = %d frames of %dx%d, mosaic canvas %dx%d, default rows %d" % ((K, w, h) + tuple(canvases["mosaic"][:2]) + (default_rows,)))
    for k in variants:
        note = ""
        if k in nbytes:
            W, H = canvases["mosaic" if "mosaic" in k else "grid"][:2]
            note = "   %.2f TB/s of %d B per canvas pixel" % (W * H * nbytes[k] / med[k] / 1e9, nbytes[k])
            tk = k.rsplit(" ", 2 if " r" in k[-3:] else 1)[0] + " torch"
            if tk in med:
                note += ", %.1f x torch" % (med[tk] / med[k])
        print("  %-30s %9.4f ms   (min %.4f .. max %.4f, %d calls per window)%s" % (k, med[k], min(t[k]), max(t[k]), reps[k], note), flush=True)
    # the composed route against the kernel on the frame grid
    for kind in frames:
        run(kind, "grid", "motion", default_rows)
        ref = torch_plate(frames[kind], motions, w, h)
        d = (outs[kind, "grid"][0].float() - ref.float()).abs()
        print("  %-10s |fotg - torch| mean %.4f max %.1f (lower median for an even count, 8-bit samples rounded before it)"
              % (kind, d.nan_to_num().mean().item(), d.nan_to_num().max().item()))
    ofc.close()


if __name__ == "__main__":
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    for K in (9, 32):
        case(1920, 1080, K, rounds)
