#!/usr/bin/env python3
"""Times of the object removal, HIP events, warm repeated calls: after a warm-up the routes are alternated within
one process (rounds of A, B, C, ...; the median per route is reported with min .. max), on 64 frames of 1920 x 1080, 8-bit RGB and
f32 gray, against one plate on the frame grid, a pan of 6 px per frame with a slight rotation, through the C-ABI into a dst allocated
once.  Masks: empty (every workgroup takes the copy path), a dozen rectangles per frame at the defaults grow 2, feather 3, and full
at grow 8, feather 8 (every pixel is sampled after the widest distance transform).  Routes:
  motion    fotg_erase_motion on six parameters per frame
  dense     fotg_erase on the flows fotg_motion_flow wrote
  fused     fotg_upsample_crop_erase on a context's coarse flows (the vectors are not the pan's), against
  up+dense  upsample_crop, then fotg_erase on its flows
  torch     about the same values from public calls and torch operations: motion_flow, warp of the plate, the mask dilated by
            max_pool2d and feathered by avg_pool2d, a blend (a box, not a disc, and a float ramp: never the same bytes)
  warp      plain warp of the plate stack along the flows: one tap per pixel, the floor for anything that samples everywhere
  subtract  subtract_background(window=0), code alone, on the motion source: the nearest sibling
Each erase route is reported against its algorithmic bytes per frame pixel: the mask (1 byte), the frame and dst (once each), and,
at the share of pixels with alpha > 0, the plate's taps counted once and the vectors (8 bytes dense, none for motion).
usage: python tools/time_erase.py [rounds] [frames]"""
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
CASES = (("empty", 2, 3), ("rects", 2, 3), ("full", 8, 8))


def masks(n, h, w, g):
    """the three masks: nothing, a dozen rectangles of 40 .. 200 pixels a side per frame, everything"""
    rects = torch.zeros((n, h, w), dtype=torch.uint8, device="cuda")
    for i in range(n):
        for _ in range(12):
            rw, rh = (int(v) for v in torch.randint(40, 200, (2,), generator=g, device="cuda"))
            x, y = int(torch.randint(0, w - rw, (1,), generator=g, device="cuda")), int(torch.randint(0, h - rh, (1,), generator=g, device="cuda"))
            rects[i, y:y + rh, x:x + rw] = 1
    return {"empty": torch.zeros_like(rects), "rects": rects, "full": torch.ones_like(rects)}


def torch_remove(frames, plates_n, remove, back, w, h, G, Fe):
    flows = F.motion_flow(back, w, h)
    wd, code, _ = F.warp(plates_n, flows, stats=True)
    m = torch.nn.functional.max_pool2d(remove[:, None].float(), 2 * G + 1, 1, G) if G else remove[:, None].float()
    a = torch.nn.functional.avg_pool2d(m, 2 * Fe + 1, 1, Fe)[:, 0] if Fe else m[:, 0]
    a = torch.where(code == 0, a, torch.zeros_like(a)).reshape(a.shape + (1,) * (frames.dim() - 3))
    f = frames.float()
    out = f + (wd.float() - f) * a
    return out.round().clamp(0, 255).to(torch.uint8) if frames.dtype == torch.uint8 else out


def main(rounds, n):
    w, h = 1920, 1080
    L, st_ = F.lib(), _stream(torch.device("cuda", 0))
    g = torch.Generator(device="cuda").manual_seed(37)
    frames = {"u8 rgb": (torch.rand((n, h, w, 3), device="cuda", generator=g) * 255).to(torch.uint8),
              "f32 gray": torch.rand((n, h, w), device="cuda", generator=g) * 255}
    plates = {k: v[:1].clone() for k, v in frames.items()}
    dsts = {k: torch.empty_like(v) for k, v in frames.items()}
    rm = masks(n, h, w, g)
    back = F.frame_motions(shot_motions(n, w, h))
    flows = F.motion_flow(back, w, h).contiguous()
    ofc = OFClass(F.operating_point(2, w, 1), F.img_params(width=w, height=h), max_batch=n)
    wl, hl = ofc.out_size()
    coarse = (torch.randn((n, hl, wl, 2), device="cuda", generator=g) * 2.0).contiguous()
    code = torch.empty((n, h, w), dtype=torch.uint8, device="cuda")

    def run(kind, src, case, G, Fe, fl=None):
        fr, ch, u8 = frames[kind], 3 if kind == "u8 rgb" else 1, kind == "u8 rgb"
        tail = (None, None, _ptr(rm[case]), G, Fe, _ptr(dsts[kind]), None, None, None, st_)
        if src == "fused":
            fn = L.fotg_upsample_crop_erase_u8 if u8 else L.fotg_upsample_crop_erase
            s = fn(ofc._h, n, _ptr(coarse), _ptr(fr), ch, 1, _ptr(plates[kind]), w, h, 0, 0, None, *tail)
        else:
            fn = {("motion", True): L.fotg_erase_motion_u8, ("motion", False): L.fotg_erase_motion, ("dense", True): L.fotg_erase_u8,
                  ("dense", False): L.fotg_erase}[src, u8]
            vec = back if src == "motion" else (flows if fl is None else fl)
            s = fn(0, n, _ptr(fr), w, h, ch, 1, _ptr(plates[kind]), w, h, 0, 0, None, _ptr(vec), *tail)
        assert s == 0

    def up_dense(kind, case, G, Fe):
        run(kind, "dense", case, G, Fe, ofc.upsample_crop(coarse))

    share = {}
    for case, G, Fe in CASES:
        share[case] = float((F.remove_objects(frames["f32 gray"][:4], plates["f32 gray"], rm[case][:4], motions=back[:4], grow=G, feather=Fe,
                                              dst=False, alpha=True) > 0).float().mean())
    variants, nbytes = {}, {}
    for kind in frames:
        el = 3 if kind == "u8 rgb" else 4
        plates_n = plates[kind].expand((n,) + tuple(plates[kind].shape[1:])).contiguous()
        for case, G, Fe in CASES:
            for src, vec in (("motion", 0.0), ("dense", 8.0)):
                name = "%s %s %s" % (kind, case, src)
                variants[name] = lambda kind=kind, src=src, case=case, G=G, Fe=Fe: run(kind, src, case, G, Fe)
                nbytes[name] = 1 + 2 * el + share[case] * (el + vec)
        variants["%s rects fused" % kind] = lambda kind=kind: run(kind, "fused", "rects", 2, 3)
        nbytes["%s rects fused" % kind] = 1 + 2 * el + share["rects"] * (el + 0.5)
        variants["%s rects up+dense" % kind] = lambda kind=kind: up_dense(kind, "rects", 2, 3)
        variants["%s rects torch" % kind] = lambda kind=kind, p=plates_n: torch_remove(frames[kind], p, rm["rects"], back, w, h, 2, 3)
        variants["%s warp" % kind] = lambda p=plates_n: F.warp(p, flows)
        variants["%s subtract r0 code" % kind] = lambda kind=kind: F.subtract_background(frames[kind], plates[kind], motions=back, window=0)
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
    print("%d frames of %dx%d against one plate; share of pixels with alpha > 0: %s" % (n, w, h, ", ".join("%s %.4f" % kv for kv in share.items())))
    for k in variants:
        note = ""
        if k in nbytes:
            note = "   %.2f TB/s of %.2f B per pixel" % (n * w * h * nbytes[k] / med[k] / 1e9, nbytes[k])
        print("  %-26s %9.4f ms   (min %.4f .. max %.4f, %d calls per window)%s" % (k, med[k], min(t[k]), max(t[k]), reps[k], note), flush=True)
    for kind in frames:
        print("  %-10s rects: motion is %.1f x the torch composition, %.2f x plain warp, %.2f x subtract r0; fused is %.2f x up+dense"
              % (kind, med["%s rects torch" % kind] / med["%s rects motion" % kind], med["%s warp" % kind] / med["%s rects motion" % kind],
                 med["%s subtract r0 code" % kind] / med["%s rects motion" % kind], med["%s rects up+dense" % kind] / med["%s rects fused" % kind]))
    ofc.close()


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 3, int(sys.argv[2]) if len(sys.argv) > 2 else 64)
