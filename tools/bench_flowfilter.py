#!/usr/bin/env python3
"""Times of the edge- and occlusion-aware flow filter, HIP events, after a warm-up, warm repeated calls on the
same buffers, the variants alternated within one process (rounds of A, B, C; the median per variant is reported).  64 flows of 1080p
(the engine's own at op-pt 2 on a drifting texture), guide = frame 0 as gray float32 or as 8-bit RGB, a mask that rejects one pixel
in eight, out + code + statistics on:
  dense     fotg_flow_filter on a full-resolution flow that already exists
  fused     fotg_upsample_crop_flow_filter on the coarse flow (the unfiltered full-resolution flow is never written or read)
  unfused   fotg_upsample_crop + fotg_flow_filter (what fused=False runs)
  composed  the same values from torch operations: one shifted slice per window offset, the weights, the masked accumulation and
            the division, on the first COMPOSED_N images only (it is slow); its time is scaled to 64 images
for R = 3 and R = 7, one and two passes.  The composed result is compared with the kernel's before anything is timed.  The bytes a
pixel needs from memory (flow or nothing, guide, mask, out, code; the passes between count out + code written and read) over the time
give the achieved HBM rate, the LDS bytes a thread reads in its window loop over the time the achieved LDS rate.  The data set
(1.06 GB of vectors in, 1.06 GB out) is far beyond the 256 MB Infinity Cache: the times are memory-resident, not cache-resident.
Run it under `rocprofv3 --kernel-trace --stats -- python tools/bench_flowfilter.py` for the kernel split.
usage: python tools/bench_flowfilter.py [rounds] [n]"""
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import flowonthego_amd as F                                   # noqa: E402
from flowonthego_amd.flowfilter import filter_flow, spatial_table, upsample_crop_filter_flow  # noqa: E402
from flowonthego_amd.oflow import OFClass                     # noqa: E402
from time_bidir import timed                                  # noqa: E402

COMPOSED_N = 4


def frames(w, h, n, g):
    """n + 1 frames of one band-limited RGB texture drifting by (3, 1) pixels per frame, 8-bit valued: (n + 1, h, w, 3) uint8"""
    base = torch.randint(0, 256, (3, h // 8 + 1, w // 8 + 1), device="cuda", generator=g, dtype=torch.uint8).float()
    img = torch.nn.functional.interpolate(base[None], size=(h, w), mode="bilinear", align_corners=False)[0]
    fr = torch.stack([torch.roll(img, (k, 3 * k), (1, 2)) for k in range(n + 1)])
    return fr.round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def composed(flow, guide, mask, radius, s, tau, iters):
    """filter_flow's out and code from torch operations, in the definition's order"""
    n, h, w = flow.shape[:3]
    G = guide.float().reshape(n, h, w, -1)
    ch = G.shape[3]
    scale = float(np.float32(1) / (np.float32(tau) * np.float32(ch)))
    R = radius
    Gp = torch.nn.functional.pad(G, (0, 0, R, R, R, R))
    cur, invalid, first = flow, mask != 0, None
    for _ in range(iters):
        valid = torch.isfinite(cur).all(-1) & ~invalid
        Vp = torch.nn.functional.pad(valid, (R, R, R, R))
        Fp = torch.nn.functional.pad(torch.where(valid[..., None], cur, torch.zeros_like(cur)), (0, 0, R, R, R, R))
        nu, nv, den = (torch.zeros((n, h, w), device=flow.device) for _ in range(3))
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                ys, xs = slice(R + dy, R + dy + h), slice(R + dx, R + dx + w)
                d = (G - Gp[:, ys, xs]).abs()
                d = d[..., 0] if ch == 1 else (d[..., 0] + d[..., 1]) + d[..., 2]
                wt = (s[abs(dy)] * s[abs(dx)]) * (1.0 - d * scale)
                wz = torch.where(Vp[:, ys, xs] & (wt > 0), wt, torch.zeros_like(wt))
                nu = nu + wz * Fp[:, ys, xs, 0]
                nv = nv + wz * Fp[:, ys, xs, 1]
                den = den + wz
        has = den > 0
        cur = torch.where(has[..., None], torch.stack([nu / den, nv / den], -1), cur)
        code = torch.where(has, (~valid).to(torch.uint8), torch.full_like(mask, 3))
        first = code if first is None else first
        invalid = code == 3
    return cur, torch.where(code == 3, code, (first != 0).to(torch.uint8))


def case(ofc, cf, full, guide, mask, radius, iters, rounds, reps, tau=20.0):
    n, h, w = full.shape[:3]
    s = spatial_table(radius, radius / 2.0)
    kw = dict(mask=mask, radius=radius, spatial=s, tau=tau, iters=iters, stats=True)
    m = COMPOSED_N
    variants = {
        "dense": lambda: filter_flow(full, guide, **kw),
        "fused": lambda: upsample_crop_filter_flow(ofc, cf, guide, **kw),
        "unfused": lambda: upsample_crop_filter_flow(ofc, cf, guide, fused=False, **kw),
    }
    a, b = variants["dense"](), variants["fused"]()
    c = composed(full[:m], guide[:m], mask[:m], radius, s, tau, iters)
    torch.cuda.synchronize()
    same = all(torch.equal(x, y) for x, y in zip(a, b))
    eq = (a[0][:m].view(torch.int32) == c[0].view(torch.int32)).float().mean().item()
    print("  fused == dense bit for bit: %s;  composed vs dense (%d images): out equal at %.6f of the values, code at %.6f"
          % (same, m, eq, (a[1][:m] == c[1]).float().mean().item()), flush=True)
    del a, b, c
    for fn in variants.values():                             # warm-up (first-call allocations, code object loads)
        fn()
        fn()
    torch.cuda.synchronize()
    t = {k: [] for k in list(variants) + ["composed"]}
    for _ in range(rounds):
        for k, fn in variants.items():
            t[k].append(timed(fn, reps))
        t["composed"].append(timed(lambda: composed(full[:m], guide[:m], mask[:m], radius, s, tau, iters), 1) * n / m)
    med = {k: statistics.median(v) for k, v in t.items()}
    rgb = guide.dim() == 4
    es = guide.element_size() * (3 if rgb else 1)
    between = (iters - 1) * 2 * (8 + 1)                      # out + code written by a pass, read by the next
    bpp = {"dense": 8 + es + 1 + 8 + 1 + between, "fused": es + 1 + 8 + 1 + between}
    gw = 1 if guide.dtype == torch.uint8 else (3 if rgb else 1)
    lds = iters * (2 * radius + 1) * (4 + 2 * radius) / 4.0 * (4 * (2 + gw) + 1 + 4)
    px = n * h * w
    print("%dx%d x %d %s %s R=%d iters=%d  " % (w, h, n, "rgb" if rgb else "gray", "u8" if guide.dtype == torch.uint8 else "f32", radius, iters)
          + "  ".join("%s %.3f ms" % kv for kv in med.items()), flush=True)
    print("  ratios: fused/dense %.3f  fused/unfused %.3f  dense/composed %.4f  fused/composed %.4f;  HBM: dense %d B/pixel = %.0f GB/s, "
          "fused %d B/pixel = %.0f GB/s;  LDS reads: %.0f B/pixel = %.1f TB/s (dense)"
          % (med["fused"] / med["dense"], med["fused"] / med["unfused"], med["dense"] / med["composed"], med["fused"] / med["composed"],
             bpp["dense"], bpp["dense"] * px / med["dense"] / 1e6, bpp["fused"], bpp["fused"] * px / med["fused"] / 1e6,
             lds, lds * px / med["dense"] / 1e9), flush=True)


if __name__ == "__main__":
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    if not torch.cuda.is_available():
        sys.exit("bench_flowfilter: no GPU")
    w, h = 1920, 1080
    g = torch.Generator(device="cuda").manual_seed(3)
    rgb8 = frames(w, h, n, g)
    gray = ((rgb8[..., 0].float() + rgb8[..., 1].float()) + rgb8[..., 2].float()) / 3.0
    ofc = OFClass(F.operating_point(2, w, 1), F.img_params(width=w, height=h), max_batch=n)
    cf = ofc.calc_batch(gray[:-1].contiguous(), gray[1:].contiguous())
    full = ofc.upsample_crop(cf)
    mask = (torch.rand((n, h, w), device="cuda", generator=g) < 0.125).to(torch.uint8)
    for guide in (gray[:-1].contiguous(), rgb8[:-1].contiguous()):
        for radius in (3, 7):
            for iters in (1, 2):
                case(ofc, cf, full, guide, mask, radius, iters, rounds, 5)
    ofc.close()
