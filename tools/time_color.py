#!/usr/bin/env python3
"""Kernel times of the flow colour code: a batch of 64 at 1080p op-pt 2 and one 4K op-pt-4 pair, fused
(fotg_upsample_crop_color from the coarse flow) and unfused (fotg_upsample_crop, then fotg_flow_color).  Meant to run under
`rocprofv3 --kernel-trace --stats -- python tools/time_color.py`; also prints host-timed milliseconds per call.
usage: python tools/time_color.py [repeats]"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import flowonthego_amd as F                                   # noqa: E402
from flowonthego_amd.color import flow_to_color               # noqa: E402
from flowonthego_amd.oflow import OFClass                     # noqa: E402


def case(w, h, op_pt, n, reps):
    op = F.operating_point(op_pt, w, 1)
    ofc = OFClass(op, F.img_params(width=w, height=h, padding=op.patch_size), max_batch=n)
    cw, ch = ofc.out_size()
    g = torch.Generator(device="cuda").manual_seed(3)
    coarse = torch.randn((n, ch, cw, 2), device="cuda", generator=g) * 8
    rgb = torch.empty((n, h, w, 3), dtype=torch.uint8, device="cuda")
    full = torch.empty((n, h, w, 2), dtype=torch.float32, device="cuda")

    def fused():
        ofc.upsample_crop_color(coarse, out=rgb)

    def unfused():
        ofc.upsample_crop(coarse, out=full)
        flow_to_color(full, out=rgb)

    for name, fn in (("fused", fused), ("unfused", unfused)):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        print("%dx%d op-pt %d n=%d %-8s %.3f ms per call" % (w, h, op_pt, n, name, e0.elapsed_time(e1) / reps), flush=True)
    ofc.close()


if __name__ == "__main__":
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    case(1920, 1080, 2, 64, reps)
    case(3840, 2160, 4, 1, reps)
