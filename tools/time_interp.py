#!/usr/bin/env python3
"""Times of the frame interpolation, HIP events, after a warm-up, the variants alternated within one process
(rounds of A, B, C, ...; the median per variant is reported), for 64 x 1080p gray at op-pt 2 and one 4K pair at op-pt 4, t = 0.5:
  warp         the yardstick: fotg_warp on a full-resolution flow that already exists (f32, ref + code + stats)
  dense        fotg_interp on full-resolution flows and masks that already exist (f32, ref + code + stats)
  dense_plain  the same without ref, code and stats
  dense_check  fotg_interp without masks: the call runs the consistency check itself
  unfused      2 x fotg_upsample_crop + fotg_fb_check + fotg_interp (what fused=False runs)
  fused        fotg_upsample_crop_interp without masks (ref + code + stats): upsampling and check inside the call
  fused_u8     the same on 8-bit frames
It also prints the candidates per call (pixels whose mask code is 0 or 1, both directions), from which section 13 derives the rate
of 64-bit atomic minima.  Run it under `rocprofv3 --kernel-trace --stats -- python tools/time_interp.py` for the kernel split.
usage: python tools/time_interp.py [rounds]"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import flowonthego_amd as F                                   # noqa: E402
from flowonthego_amd.consistency import fb_check              # noqa: E402
from flowonthego_amd.interp import interpolate                # noqa: E402
from flowonthego_amd.oflow import OFClass                     # noqa: E402
from flowonthego_amd.warp import warp                         # noqa: E402
from time_bidir import frames, timed                          # noqa: E402


def case(w, h, op_pt, n, rounds, reps):
    op = F.operating_point(op_pt, w, 1)
    op.bidir = True
    ofc = OFClass(op, F.img_params(width=w, height=h), max_batch=n)
    I0, I1 = frames(w, h, n, torch.Generator(device="cuda").manual_seed(3))
    B0, B1 = I0.to(torch.uint8), I1.to(torch.uint8)
    cfw, cbw = ofc.calc_bidirectional(I0, I1)
    fw, bw = ofc.upsample_crop(cfw), ofc.upsample_crop(cbw)
    m, mb, cnt = fb_check(fw, bw, stats=True)
    cand = int(cnt[:, :, :2].sum().item())
    variants = {
        "warp": lambda: warp(I1, fw, ref=I0, stats=True),
        "dense": lambda: interpolate(I0, I1, fw, bw, 0.5, mask_fw=m, mask_bw=mb, ref=I0, stats=True),
        "dense_plain": lambda: interpolate(I0, I1, fw, bw, 0.5, mask_fw=m, mask_bw=mb),
        "dense_check": lambda: interpolate(I0, I1, fw, bw, 0.5, ref=I0, stats=True),
        "unfused": lambda: ofc.upsample_crop_interpolate(cfw, cbw, I0, I1, 0.5, ref=I0, stats=True, fused=False),
        "fused": lambda: ofc.upsample_crop_interpolate(cfw, cbw, I0, I1, 0.5, ref=I0, stats=True),
        "fused_u8": lambda: ofc.upsample_crop_interpolate(cfw, cbw, B0, B1, 0.5, ref=B0, stats=True),
    }
    for fn in variants.values():                             # warm-up (first-call allocations, code object loads)
        fn()
        fn()
    torch.cuda.synchronize()
    t = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            t[k].append(timed(fn, reps))
    med = {k: statistics.median(v) for k, v in t.items()}
    print("%dx%d op-pt %d n=%d  " % (w, h, op_pt, n) + "  ".join("%s %.3f ms" % kv for kv in med.items()), flush=True)
    print("  candidates %d (%.4f of 2 n w h)  ratios: dense/warp %.3f  fused/unfused %.3f  fused/dense_check %.3f"
          % (cand, cand / (2.0 * n * w * h), med["dense"] / med["warp"], med["fused"] / med["unfused"], med["fused"] / med["dense_check"]),
          flush=True)
    ofc.close()


if __name__ == "__main__":
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    case(1920, 1080, 2, 64, rounds, 5)
    case(3840, 2160, 4, 1, rounds, 10)
