#!/usr/bin/env python3
"""Times of bidirectional flow and the consistency check, HIP events, after a warm-up, the variants
alternated within one process (rounds of A, B, A, B, ...; the median per variant is reported):
  1. 64 x 1080p op-pt 2 (parity): fotg_calc_bidir against two fotg_calc_batch calls (I0 -> I1, I1 -> I0)
  2. the same for one 4K op-pt-4 pair
  3. 64 x 1080p op-pt 2: the fused check (fotg_upsample_crop_fb_check) against fotg_upsample_crop x 2 + fotg_fb_check
Run it under `rocprofv3 --kernel-trace --stats -- python tools/time_bidir.py` for the kernel split.
usage: python tools/time_bidir.py [rounds]"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import flowonthego_amd as F                                   # noqa: E402
from flowonthego_amd.consistency import fb_check              # noqa: E402
from flowonthego_amd.oflow import OFClass                     # noqa: E402


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def compare(label, variants, rounds, reps):
    for fn in variants.values():                             # warm-up (first-call allocations, code object loads)
        fn()
        fn()
    torch.cuda.synchronize()
    t = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            t[k].append(timed(fn, reps))
    med = {k: statistics.median(v) for k, v in t.items()}
    names = list(variants)
    print("%-28s " % label + "  ".join("%s %.3f ms" % (k, med[k]) for k in names) +
          "  ratio %s/%s %.3f" % (names[0], names[1], med[names[0]] / med[names[1]]), flush=True)
    return med


def frames(w, h, n, g):
    base = torch.randint(0, 256, (1, h // 8 + 1, w // 8 + 1), device="cuda", generator=g, dtype=torch.uint8).float()
    img = torch.nn.functional.interpolate(base[None], size=(h, w), mode="bilinear", align_corners=False)[0, 0]
    I0 = torch.stack([torch.roll(img, 3 * k, 1) for k in range(n)]).round().contiguous()
    I1 = torch.stack([torch.roll(img, (k % 5 - 2, 3 * k + 2), (0, 1)) for k in range(n)]).round().contiguous()
    return I0, I1


def flow_case(w, h, op_pt, n, rounds, reps):
    op = F.operating_point(op_pt, w, 1)
    op.bidir = True
    ofc = OFClass(op, F.img_params(width=w, height=h), max_batch=n)
    I0, I1 = frames(w, h, n, torch.Generator(device="cuda").manual_seed(1))
    fw, bw, fw2, bw2 = (ofc.new_outflow(n) for _ in range(4))
    compare("%dx%d op-pt %d n=%d" % (w, h, op_pt, n),
            {"bidir": lambda: ofc.calc_bidirectional(I0, I1, outflow=fw, outflow_bw=bw),
             "two_calls": lambda: (ofc.calc_batch(I0, I1, outflow=fw2), ofc.calc_batch(I1, I0, outflow=bw2))}, rounds, reps)
    ofc.close()


def check_case(w, h, op_pt, n, rounds, reps):
    op = F.operating_point(op_pt, w, 1)
    op.bidir = True
    ofc = OFClass(op, F.img_params(width=w, height=h), max_batch=n)
    I0, I1 = frames(w, h, n, torch.Generator(device="cuda").manual_seed(2))
    fw, bw = ofc.calc_bidirectional(I0, I1)
    full, full_bw = (torch.empty((n, h, w, 2), device="cuda") for _ in range(2))

    def unfused():
        ofc.upsample_crop(fw, out=full)
        ofc.upsample_crop(bw, out=full_bw)
        fb_check(full, full_bw, stats=True)

    compare("check %dx%d op-pt %d n=%d" % (w, h, op_pt, n),
            {"fused": lambda: ofc.upsample_crop_fb_check(fw, bw, stats=True, fused=True), "unfused": unfused}, rounds, reps)
    ofc.close()


if __name__ == "__main__":
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    flow_case(1920, 1080, 2, 64, rounds, 5)
    flow_case(3840, 2160, 4, 1, rounds, 5)
    check_case(1920, 1080, 2, 64, rounds, 10)
