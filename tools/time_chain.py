#!/usr/bin/env python3
"""Times of flow chaining, HIP events, after a warm-up, the routes alternated within one process (rounds of
A, B, C, ...; the median per route is reported), for one 1080p gray sequence of T = 8 flows at op-pt 2, forward only and with the
backward flows.  Every timed window is a few hundred milliseconds of back-to-back calls (the number of calls per window is sized
from a first estimate of the route's time), and the chain routes write into outputs allocated once, through the C-ABI, so a
window holds launches and nothing else:
  dense    fotg_flow_chain on full-resolution flows that already exist (one launch)
  unfused  fotg_upsample_crop of the T flows + fotg_flow_chain (what fused=False runs)
  fused    fotg_upsample_crop_flow_chain (one launch, no full-resolution flow)
  torch    what a user does without the chain: per step upsample_crop of one flow, torch.nn.functional.grid_sample of it at the
           current positions (bilinear, border, align_corners=True), the in-frame test and the position update
Prints the algorithmic bytes of the chain next to the times.  Run it under `rocprofv3 --kernel-trace --stats -- python
tools/time_chain.py` for the kernel split.
usage: python tools/time_chain.py [rounds]"""
import ctypes as C
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import flowonthego_amd as F                                   # noqa: E402
from flowonthego_amd.chain import chain                       # noqa: E402
from flowonthego_amd.oflow import OFClass, _ptr, _stream      # noqa: E402
from time_bidir import timed                                  # noqa: E402


def torch_route(ofc, cf, cb):
    T = cf.shape[0]
    h, w = ofc.height_org, ofc.width_org
    ys, xs = torch.meshgrid(torch.arange(h, device="cuda", dtype=torch.float32), torch.arange(w, device="cuda", dtype=torch.float32), indexing="ij")
    X, Y = xs.clone(), ys.clone()
    live = torch.ones((h, w), dtype=torch.bool, device="cuda")
    sx, sy = 2.0 / (w - 1), 2.0 / (h - 1)
    sample = lambda fl, X, Y: torch.nn.functional.grid_sample(fl.permute(0, 3, 1, 2), torch.stack([X * sx - 1.0, Y * sy - 1.0], -1)[None],
                                                              mode="bilinear", padding_mode="border", align_corners=True)[0]
    for k in range(T):
        uv = sample(ofc.upsample_crop(cf[k:k + 1]), X, Y)
        Xn, Yn = X + uv[0], Y + uv[1]
        ok = live & (Xn >= 0) & (Xn <= w - 1) & (Yn >= 0) & (Yn <= h - 1)
        if cb is not None:
            b = sample(ofc.upsample_crop(cb[k:k + 1]), torch.where(ok, Xn, X), torch.where(ok, Yn, Y))
            du, dv = uv[0] + b[0], uv[1] + b[1]
            ok &= du * du + dv * dv < 0.01 * (uv[0] * uv[0] + uv[1] * uv[1] + b[0] * b[0] + b[1] * b[1]) + 0.5
        X, Y, live = torch.where(ok, Xn, X), torch.where(ok, Yn, Y), ok
    return X - xs, Y - ys, live


WINDOW_MS = 300.0                                             # the least length of a timed window


def case(w, h, op_pt, T, rounds):
    op = F.operating_point(op_pt, w, 1)
    op.bidir = True
    ofc = OFClass(op, F.img_params(width=w, height=h), max_batch=T)
    g = torch.Generator(device="cuda").manual_seed(3)
    base = torch.randint(0, 256, (1, h // 8 + 1, w // 8 + 1), device="cuda", generator=g, dtype=torch.uint8).float()
    img = torch.nn.functional.interpolate(base[None], size=(h, w), mode="bilinear", align_corners=False)[0, 0]
    frames = torch.stack([torch.roll(img, (k, 3 * k), (0, 1)) for k in range(T + 1)]).round().contiguous()
    cf, cb = ofc.calc_sequence_bidirectional(frames)
    full, full_bw = ofc.upsample_crop(cf), ofc.upsample_crop(cb)
    L, a1, a2, st_ = F.lib(), C.c_float(0.01), C.c_float(0.5), _stream(ofc.device)
    # outputs allocated once; the unfused route upsamples into buffers of its own, so the dense route's inputs stay as they are
    total = torch.empty((h, w, 2), device="cuda")
    code = torch.empty((h, w), dtype=torch.uint8, device="cuda")
    steps = torch.empty((h, w), dtype=torch.int32, device="cuda")
    st = torch.empty((5,), dtype=torch.int64, device="cuda")
    up, up_bw = torch.empty_like(full), torch.empty_like(full_bw)
    outs = (_ptr(total), _ptr(code), _ptr(steps), _ptr(st))

    def dense(f, b):
        assert L.fotg_flow_chain(0, 1, T, _ptr(f), _ptr(b), w, h, a1, a2, *outs, st_) == 0

    def unfused(b):
        ofc.upsample_crop(cf, out=up)
        if b is not None:
            ofc.upsample_crop(b, out=up_bw)
        dense(up, None if b is None else up_bw)

    def fused(b):
        assert L.fotg_upsample_crop_flow_chain(ofc._h, T, _ptr(cf), _ptr(b), a1, a2, *outs, st_) == 0

    for label, b, fb in (("forward only", None, None), ("with backward flows", cb, full_bw)):
        variants = {
            "dense": lambda: dense(full, fb),
            "unfused": lambda: unfused(b),
            "fused": lambda: fused(b),
            "torch": lambda: torch_route(ofc, cf, b),
        }
        reps = {}
        for k, fn in variants.items():                       # warm-up (first-call allocations, code object loads), then the window's size
            fn()
            fn()
            torch.cuda.synchronize()
            reps[k] = max(10, math.ceil(WINDOW_MS / timed(fn, 20)))
        t = {k: [] for k in variants}
        for _ in range(rounds):
            for k, fn in variants.items():
                t[k].append(timed(fn, reps[k]))
        med = {k: statistics.median(v) for k, v in t.items()}
        _, _, _, s5 = chain(full, fb, stats=True)
        rd = int(s5[4].item()) * (16 if fb is not None else 8)
        print("%dx%d op-pt %d T=%d %s  " % (w, h, op_pt, T, label) + "  ".join("%s %.4f ms" % kv for kv in med.items()), flush=True)
        print("  spread (min .. max): " + "  ".join("%s %.4f .. %.4f" % (k, min(v), max(v)) for k, v in t.items()), flush=True)
        print("  calls per window: " + "  ".join("%s %d (%.0f ms)" % (k, reps[k], reps[k] * med[k]) for k in variants), flush=True)
        print("  chains valid %.4f, mean steps %.3f; algorithmic bytes: read <= %.1f MB (T x %d B per pixel; %.1f MB for the steps taken), "
              "written %.1f MB (13 B per pixel); dense %.1f GB/s of them"
              % (s5[0].item() / (h * w), s5[4].item() / (h * w), T * (16 if fb is not None else 8) * h * w / 1e6, 16 if fb is not None else 8,
                 rd / 1e6, 13 * h * w / 1e6, (rd + 13 * h * w) / med["dense"] / 1e6), flush=True)
    ofc.close()


if __name__ == "__main__":
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    case(1920, 1080, 2, 8, rounds)
