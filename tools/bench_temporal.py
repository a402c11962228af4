#!/usr/bin/env python3
"""Times of the motion-compensated temporal filter, HIP events, after a warm-up, the variants alternated
within one process (rounds of A, B, C, D; the median per variant is reported).  A stack of 16 frames of 1080p, every frame a centre,
neighbours at distance +-1 (K = 2) or +-1, +-2 (K = 4), the engine's own flows at op-pt 2, ref and statistics on:
  dense     fotg_temporal_filter on full-resolution flows that already exist
  fused     fotg_upsample_crop_temporal_filter on the coarse flows (no full-resolution flow is written or read)
  unfused   fotg_upsample_crop + fotg_temporal_filter (what fused=False runs)
  composed  the same result from what existed before: K x flowonthego_amd.warp(..., stats=True) on the full-resolution flows, torch
            operations for the differences, the box sums (replicate padding), the weights and the accumulation, and the division
for gray float32 (K = 2 and K = 4) and RGB 8-bit (K = 2).  The composed result is compared with the kernel's before anything is
timed.  The bytes per pixel the algorithm needs (centre + ref + K x (flow + taps) + dst, each tap counted once) over the time give the
achieved bytes/s.
Run it under `rocprofv3 --kernel-trace --stats -- python tools/bench_temporal.py` for the kernel split.
usage: python tools/bench_temporal.py [rounds]"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import flowonthego_amd as F                                   # noqa: E402
from flowonthego_amd.oflow import OFClass                     # noqa: E402
from flowonthego_amd.temporal import neighbor_table, temporal_filter, upsample_crop_temporal_filter  # noqa: E402
from flowonthego_amd.warp import warp                         # noqa: E402
from time_bidir import timed                                  # noqa: E402


def sequence(w, h, T, rgb, g):
    """T frames of one band-limited texture drifting by (3, 1) pixels per frame, with noise sigma 5; 8-bit valued float32"""
    base = torch.randint(0, 256, (3 if rgb else 1, h // 8 + 1, w // 8 + 1), device="cuda", generator=g, dtype=torch.uint8).float()
    img = torch.nn.functional.interpolate(base[None], size=(h, w), mode="bilinear", align_corners=False)[0]
    fr = torch.stack([torch.roll(img, (k, 3 * k), (1, 2)) for k in range(T)])
    clean = fr.round()
    noisy = (fr + 5.0 * torch.randn(fr.shape, device="cuda", generator=g)).round().clamp(0, 255)
    shape = (lambda t: t.permute(0, 2, 3, 1).contiguous()) if rgb else (lambda t: t[:, 0].contiguous())
    return shape(clean), shape(noisy)


def composed(frames, center, neighbors, flows, tau, ref):
    """temporal_filter's dst, used and two residual sums from warp() and torch operations"""
    u8 = frames.dtype == torch.uint8
    S = frames.float() if u8 else frames
    ch = 1 if S.dim() == 3 else S.shape[3]
    cen = torch.tensor(center, device=S.device)
    Cf = S[cen]
    C4 = Cf if S.dim() == 4 else Cf[..., None]
    scale = 1.0 / (torch.tensor(tau, dtype=torch.float32) * float(9 * ch))
    scale = float(scale)
    num, den = C4.clone(), torch.ones(Cf.shape[:3], device=S.device)
    used = torch.zeros(Cf.shape[:3], dtype=torch.uint8, device=S.device)
    for k in range(len(neighbors[0])):
        nb = torch.tensor([row[k] for row in neighbors], device=S.device)
        present = (nb >= 0)[:, None, None]
        Wk, code, _ = warp(S[torch.where(nb >= 0, nb, cen)], flows[:, k].contiguous(), stats=True)
        W4 = Wk if S.dim() == 4 else Wk[..., None]
        d = (C4 - W4).abs()
        d = d[..., 0] if ch == 1 else (d[..., 0] + d[..., 1]) + d[..., 2]
        p = torch.nn.functional.pad(d[:, None], (1, 1, 0, 0), mode="replicate")[:, 0]
        r = (p[:, :, :-2] + p[:, :, 1:-1]) + p[:, :, 2:]
        p = torch.nn.functional.pad(r[:, None], (0, 0, 1, 1), mode="replicate")[:, 0]
        e = (p[:, :-2] + p[:, 1:-1]) + p[:, 2:]
        wt = 1.0 - e * scale
        use = (code == 0) & (wt > 0) & present
        wz = torch.where(use, wt, torch.zeros_like(wt))
        num = num + wz[..., None] * W4
        den = den + wz
        used += use.to(torch.uint8)
    value = num / den[..., None]
    R4 = ref.float().reshape(C4.shape)
    s_val = (R4 - value).abs().sum((1, 2, 3), dtype=torch.float64)
    s_ctr = (R4 - C4).abs().sum((1, 2, 3), dtype=torch.float64)
    dst = value.reshape(Cf.shape)
    if u8:
        dst = dst.round().clamp(0, 255).to(torch.uint8)
    return dst, used, s_val, s_ctr


def case(w, h, T, radius, rgb, u8, rounds, reps, tau=30.0):
    K = 2 * radius
    op = F.operating_point(2, w, 3 if rgb and not u8 else 1)
    if rgb and u8:
        op.u8_color = 2
    ofc = OFClass(op, F.img_params(width=w, height=h), max_batch=T * K)
    clean, noisy = sequence(w, h, T, rgb, torch.Generator(device="cuda").manual_seed(3))
    if u8:
        clean, noisy = clean.to(torch.uint8), noisy.to(torch.uint8)
    center, neighbors = neighbor_table(T, radius)
    i0 = torch.tensor([c for c in center for _ in range(K)], device="cuda")
    i1 = torch.tensor([b if b >= 0 else c for c, row in zip(center, neighbors) for b in row], device="cuda")
    calc = ofc.calc_batch_u8 if u8 else ofc.calc_batch
    cf = calc(noisy[i0], noisy[i1])
    full = ofc.upsample_crop(cf).view(T, K, h, w, 2)
    del i0, i1
    variants = {
        "dense": lambda: temporal_filter(noisy, center, neighbors, full, tau=tau, ref=clean, stats=True),
        "fused": lambda: upsample_crop_temporal_filter(ofc, cf, noisy, center, neighbors, tau=tau, ref=clean, stats=True),
        "unfused": lambda: upsample_crop_temporal_filter(ofc, cf, noisy, center, neighbors, tau=tau, ref=clean, stats=True, fused=False),
        "composed": lambda: composed(noisy, center, neighbors, full, tau, clean),
    }
    # the three compute the same thing
    a, b, c = (variants[k]() for k in ("dense", "fused", "composed"))
    torch.cuda.synchronize()
    same = all(torch.equal(x, y) for x, y in zip(a, b))
    diff = (a[0].float() - c[0].float()).abs()
    print("  fused == dense bit for bit: %s;  composed vs dense: dst equal at %.6f of the values (max |d| %.3g), used equal at %.6f, "
          "sums rel. %.2e %.2e" % (same, (diff == 0).float().mean().item(), diff.max().item(), (a[1] == c[1]).float().mean().item(),
                                   ((a[2][:, 2] - c[2]) / a[2][:, 2]).abs().max().item(), ((a[2][:, 3] - c[3]) / a[2][:, 3]).abs().max().item()),
          flush=True)
    del a, b, c
    for fn in variants.values():                             # warm-up (first-call allocations, code object loads)
        fn()
        fn()
    torch.cuda.synchronize()
    t = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            t[k].append(timed(fn, reps))
    med = {k: statistics.median(v) for k, v in t.items()}
    es = (1 if u8 else 4) * (3 if rgb else 1)                # bytes of a pixel of a frame
    present = sum(b >= 0 for row in neighbors for b in row) / float(T)
    bpp = {"dense": es + present * (8 + es) + es + es, "fused": es + present * es + es + es}     # centre, flows + taps, ref, dst
    print("%dx%d x %d %s %s K=%d  " % (w, h, T, "rgb" if rgb else "gray", "u8" if u8 else "f32", K)
          + "  ".join("%s %.3f ms" % kv for kv in med.items()), flush=True)
    print("  ratios: fused/dense %.3f  fused/unfused %.3f  dense/composed %.3f  fused/composed %.3f;  algorithmic bytes: dense %.1f B/pixel = %.0f GB/s, "
          "fused %.1f B/pixel = %.0f GB/s" % (med["fused"] / med["dense"], med["fused"] / med["unfused"], med["dense"] / med["composed"], med["fused"] / med["composed"],
                                             bpp["dense"], bpp["dense"] * T * h * w / med["dense"] / 1e6,
                                             bpp["fused"], bpp["fused"] * T * h * w / med["fused"] / 1e6), flush=True)
    ofc.close()


if __name__ == "__main__":
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    if not torch.cuda.is_available():
        sys.exit("bench_temporal: no GPU")
    case(1920, 1080, 16, 1, False, False, rounds, 40)
    case(1920, 1080, 16, 2, False, False, rounds, 40)
    case(1920, 1080, 16, 1, True, True, rounds, 40)
