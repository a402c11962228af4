#!/usr/bin/env python3
"""Times of the pull-push hole filling, HIP events, warm repeated calls: after a warm-up the routes are
alternated within one process (rounds of A, B, C, ...; the median per route is reported with min .. max), on 64 frames of 1920 x 1080
through the C-ABI into a dst allocated once.  Frames: 8-bit RGB, float32 gray, float32 two-channel flows.  Holes:
  none      no hole at all
  rects     a dozen rectangles of 40 .. 200 pixels per frame, a third of each left as holes: what remove_objects leaves where the
            plate knows nothing
  fb        the fb_check mask of a real pair: two 1920 x 1080 crops of yosemite_4k 7 x 3 pixels apart, a patch moving by (20, 12) on top
  sparse    97 % holes: a sparse set of values made dense
  square    one 400 x 400 hole per frame
Routes:
  fill      fotg_fill / fotg_fill_u8: three launches (pull, top, push)
  clone     torch.clone of the frames: the floor, one read and one write of the frame
  torch     the same quantity from torch operations in float: an avg_pool2d pyramid of value * known and of known, pushed back down
            with interpolate(bilinear) -- not the same bytes (its sums are float, its weights those of align_corners=False)
fill is reported against its algorithmic bytes per pixel: the frame and the hole byte read twice (pull, push), the frame written
once.  The share of each launch is not timed here: `rocprofv3 --kernel-trace --stats -- python tools/time_fill.py 1 64` lists the
three kernels.
usage: python tools/time_fill.py [rounds] [frames]"""
import math
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import flowonthego_amd as F                                   # noqa: E402
import flowonthego_amd.fill                                   # noqa: E402,F401
from flowonthego_amd._args import _ptr, _stream               # noqa: E402
from time_bidir import timed                                  # noqa: E402

WINDOW_MS = 200.0


def real_mask(h, w):
    """the forward consistency mask of two crops of yosemite_4k with a moving patch"""
    from flowonthego_amd.oflow import OFClass
    img = np.load(os.path.join(ROOT, "tests", "golden", "natural_images.npz"))["yosemite_4k"]
    a, b = img[500:500 + h, 900:900 + w].copy(), img[503:503 + h, 907:907 + w].copy()
    a[300:460, 700:940] = img[1700:1860, 300:540]
    b[312:472, 720:960] = img[1700:1860, 300:540]
    op = F.operating_point(2, w, 1)
    op.bidir = True
    o = OFClass(op, F.img_params(width=w, height=h), max_batch=1)
    fw, bw = o.bidirectional_flows(torch.from_numpy(a)[None].cuda(), torch.from_numpy(b)[None].cuda())
    m = o.upsample_crop_fb_check(fw, bw)[0]
    flow = o.upsample_crop(fw)
    torch.cuda.synchronize()
    o.close()
    return m[0].clone(), flow[0].clone()


def hole_maps(n, h, w, g, fb):
    Z = lambda: torch.zeros((n, h, w), dtype=torch.uint8, device="cuda")
    rects = Z()
    for i in range(n):
        for _ in range(12):
            rw, rh = (int(v) for v in torch.randint(40, 200, (2,), generator=g, device="cuda"))
            x, y = int(torch.randint(0, w - rw, (1,), generator=g, device="cuda")), int(torch.randint(0, h - rh, (1,), generator=g, device="cuda"))
            rects[i, y:y + rh, x:x + rw // 3] = 1
    square = Z()
    square[:, 300:700, 800:1200] = 1
    return {"none": Z(), "rects": rects, "fb": fb[None].expand(n, h, w).contiguous(),
            "sparse": (torch.rand((n, h, w), device="cuda", generator=g) < 0.97).to(torch.uint8), "square": square}


def torch_fill(x, hole):
    """x (n, h, w, c) any type, hole (n, h, w) uint8 -> float (n, h, w, c)"""
    P = torch.nn.functional
    v = x.permute(0, 3, 1, 2).float()
    k = (hole == 0).float()[:, None]
    levels = [(v * k, k)]
    while levels[-1][1].shape[-2:] != (1, 1):
        s, c = levels[-1]
        levels.append((P.avg_pool2d(s, 2, ceil_mode=True), P.avg_pool2d(c, 2, ceil_mode=True)))
    s, c = levels[-1]
    f = s / c.clamp_min(1e-20)
    for s, c in reversed(levels[:-1]):
        up = P.interpolate(f, size=s.shape[-2:], mode="bilinear", align_corners=False)
        f = torch.where(c > 0, s / c.clamp_min(1e-20), up)
    return torch.where(k > 0, v, f).permute(0, 2, 3, 1)


def main(rounds, n):
    w, h = 1920, 1080
    L = F.lib()
    st_ = _stream(torch.device("cuda", 0))
    g = torch.Generator(device="cuda").manual_seed(43)
    fb, flow = real_mask(h, w)
    holes = hole_maps(n, h, w, g, fb)
    frames = {"u8 rgb": torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device="cuda", generator=g),
              "f32 gray": torch.rand((n, h, w, 1), device="cuda", generator=g) * 255,
              "f32 flow": flow[None].expand(n, h, w, 2).contiguous()}
    dst = {k: torch.empty_like(v) for k, v in frames.items()}
    px_bytes = {"u8 rgb": 3, "f32 gray": 4, "f32 flow": 8}
    for name, m in holes.items():
        print("holes %-7s %.2f %% of the pixels" % (name, 100.0 * float(m.float().mean())))
    print("stream-ordered memory of a call: " + ", ".join("%s %.0f MiB" % (k, F.fill.scratch_bytes(n, w, h, v.shape[3]) / 2 ** 20) for k, v in frames.items()))

    def fill(kind, case):
        x = frames[kind]
        fn = L.fotg_fill_u8 if x.dtype == torch.uint8 else L.fotg_fill
        assert fn(0, n, _ptr(x), w, h, x.shape[3], _ptr(holes[case]), 0, _ptr(dst[kind]), None, None, st_) == 0

    # the torch composition is the same quantity: the two agree to float rounding and the weights at the borders
    fill("f32 gray", "rects")
    d = (dst["f32 gray"][:4] - torch_fill(frames["f32 gray"][:4], holes["rects"][:4])).abs() if n >= 4 else None
    if d is not None:
        print("fill against the torch composition, f32 gray, rects: mean |d| %.3f, max %.3f grey levels" % (float(d[:4].mean()), float(d[:4].max())))
    variants = {}
    for kind in frames:
        variants["%s clone" % kind] = lambda kind=kind: frames[kind].clone()
        for case in holes:
            variants["%s %s fill" % (kind, case)] = lambda kind=kind, case=case: fill(kind, case)
            variants["%s %s torch" % (kind, case)] = lambda kind=kind, case=case: torch_fill(frames[kind][:8], holes[case][:8])
    reps = {}
    for k, fn in variants.items():
        fn()
        fn()
        torch.cuda.synchronize()
        reps[k] = max(2, math.ceil(WINDOW_MS / timed(fn, 2))) if "torch" not in k else 2
    t = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            t[k].append(timed(fn, reps[k]))
    med = {k: statistics.median(v) for k, v in t.items()}
    print("%d frames of %dx%d (the torch route on 8 of them, scaled to %d)" % (n, w, h, n))
    for k in variants:
        kind = " ".join(k.split()[:2])
        scale = n / 8.0 if k.endswith("torch") else 1.0
        ms = med[k] * scale
        note = ""
        if k.endswith("fill"):
            b = 2 * (px_bytes[kind] + 1) + px_bytes[kind]
            note = "   %.2f TB/s of %d B per pixel, %.2f x clone" % (n * w * h * b / ms / 1e9, b, ms / med["%s clone" % kind])
        elif k.endswith("clone"):
            note = "   %.2f TB/s of %d B per pixel" % (n * w * h * 2 * px_bytes[kind] / ms / 1e9, 2 * px_bytes[kind])
        else:
            note = "   %.1f x fill" % (ms / med[k.replace("torch", "fill")])
        print("  %-24s %9.4f ms   (min %.4f .. max %.4f, %d calls per window)%s" % (k, ms, min(t[k]) * scale, max(t[k]) * scale, reps[k], note), flush=True)


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 3, int(sys.argv[2]) if len(sys.argv) > 2 else 64)
