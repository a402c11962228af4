#!/usr/bin/env python3
"""Times of the frame warp, HIP events, after a warm-up, the variants alternated within one process
(rounds of A, B, C, ...; the median per variant is reported), for 64 x 1080p gray at op-pt 2 and one 4K pair at op-pt 4:
  dense        fotg_warp on a full-resolution flow that already exists (f32, ref + code + stats)
  dense_plain  the same without ref, code and stats
  unfused      fotg_upsample_crop + fotg_warp (what fused=False runs)
  fused        fotg_upsample_crop_warp (ref + code + stats)
  fused_plain  the same without ref, code and stats
  fused_u8     fused, 8-bit frames (ref + code + stats)
  torch        what a user does without the warp: upsample_crop + a normalised grid + torch.nn.functional.grid_sample(bilinear,
               border, align_corners=True) + the validity mask + the two masked abs().sum() reductions
Run it under `rocprofv3 --kernel-trace --stats -- python tools/time_warp.py` for the kernel split.
usage: python tools/time_warp.py [rounds]"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import flowonthego_amd as F                                   # noqa: E402
from flowonthego_amd.oflow import OFClass                     # noqa: E402
from flowonthego_amd.warp import warp                         # noqa: E402
from time_bidir import frames, timed                          # noqa: E402


def torch_route(ofc, cf, I0, I1):
    n, h, w = I1.shape
    flow = ofc.upsample_crop(cf)
    ys, xs = torch.meshgrid(torch.arange(h, device="cuda", dtype=torch.float32), torch.arange(w, device="cuda", dtype=torch.float32), indexing="ij")
    X, Y = xs + flow[..., 0], ys + flow[..., 1]
    grid = torch.stack([X * (2.0 / (w - 1)) - 1.0, Y * (2.0 / (h - 1)) - 1.0], -1)
    dst = torch.nn.functional.grid_sample(I1[:, None], grid, mode="bilinear", padding_mode="border", align_corners=True)[:, 0]
    ok = (X >= 0) & (X <= w - 1) & (Y >= 0) & (Y <= h - 1)
    return dst, ok.sum((1, 2)), ((I0 - dst).abs() * ok).sum((1, 2), dtype=torch.float64), ((I0 - I1).abs() * ok).sum((1, 2), dtype=torch.float64)


def case(w, h, op_pt, n, rounds, reps):
    ofc = OFClass(F.operating_point(op_pt, w, 1), F.img_params(width=w, height=h), max_batch=n)
    I0, I1 = frames(w, h, n, torch.Generator(device="cuda").manual_seed(3))
    B0, B1 = I0.to(torch.uint8), I1.to(torch.uint8)
    cf = ofc.calc_batch(I0, I1)
    full = ofc.upsample_crop(cf)
    variants = {
        "dense": lambda: warp(I1, full, ref=I0, stats=True),
        "dense_plain": lambda: warp(I1, full),
        "unfused": lambda: ofc.upsample_crop_warp(cf, I1, ref=I0, stats=True, fused=False),
        "fused": lambda: ofc.upsample_crop_warp(cf, I1, ref=I0, stats=True),
        "fused_plain": lambda: ofc.upsample_crop_warp(cf, I1),
        "fused_u8": lambda: ofc.upsample_crop_warp(cf, B1, ref=B0, stats=True),
        "torch": lambda: torch_route(ofc, cf, I0, I1),
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
    print("  ratios: fused/unfused %.3f  fused/dense %.3f  fused/torch %.3f  unfused/torch %.3f"
          % (med["fused"] / med["unfused"], med["fused"] / med["dense"], med["fused"] / med["torch"], med["unfused"] / med["torch"]), flush=True)
    ofc.close()


if __name__ == "__main__":
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    case(1920, 1080, 2, 64, rounds, 5)
    case(3840, 2160, 4, 1, rounds, 10)
