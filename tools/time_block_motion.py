#!/usr/bin/env python3
"""Times of the block motion vectors, HIP events, after a warm-up, warm repeated calls on the same buffers, the
routes alternated within one process (rounds of A, B, C; the median and the spread per route are reported).  64 pairs of 1080p 8-bit
gray frames (a band-limited texture drifting by (3, 1) pixels per frame), the engine's own flow at op-pt 2, block 16, refine 0 and 2,
mv + cost + kind out:
  dense     fotg_block_motion on a full-resolution flow that already exists
  unfused   fotg_upsample_crop + fotg_block_motion (what fused=False runs)
  fused     fotg_upsample_crop_block_motion on the coarse flow (the full-resolution flow is never written or read)
  composed  (refine 0 only) the same mv and cost from torch operations: the quantised vectors, the block and quadrant means by
            reshaped sums, and per candidate four gathers of ref, the bilinear prediction and a reshaped block sum; on the first
            COMPOSED_N pairs only, its time scaled to 64 pairs
The composed mv and cost are asserted equal to the kernel's, and the fused outputs to the dense ones, before anything is timed.  The
bytes a pixel needs from memory (cur, ref once, the flow or its coarse form; the 13 bytes per block that leave are counted too) over
the time give the achieved HBM rate.  usage: python tools/time_block_motion.py [rounds] [n]"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import flowonthego_amd as F                                   # noqa: E402
from flowonthego_amd.blockmotion import block_motion, upsample_crop_block_motion  # noqa: E402
from flowonthego_amd.oflow import OFClass                     # noqa: E402
from bench_flowfilter import frames                           # noqa: E402
from time_bidir import timed                                  # noqa: E402

COMPOSED_N = 4
BIG = 1 << 30


def block_sum(t, B):
    """(n, h, w) integers -> (n, ceil(h / B), ceil(w / B)) sums over B x B blocks clipped to the frame"""
    n, h, w = t.shape
    bh, bw = -(-h // B), -(-w // B)
    p = torch.nn.functional.pad(t, (0, bw * B - w, 0, bh * B - h))
    return p.view(n, bh, B, bw, B).sum(dim=(2, 4))


def composed(cur, ref, flow, B):
    """block_motion(refine=0)'s mv and cost from torch operations, in the definition's order"""
    n, h, w = cur.shape
    bh, bw = -(-h // B), -(-w // B)
    known = (flow.abs() <= 4096.0).all(-1)
    Q = torch.where(known[..., None], flow, torch.zeros_like(flow)).mul(4.0).round().to(torch.int32)     # round: to nearest even
    half = [block_sum(t, B // 2) for t in (Q[..., 0] * known, Q[..., 1] * known, known.to(torch.int32))]
    half = [torch.nn.functional.pad(t, (0, 2 * bw - t.shape[2], 0, 2 * bh - t.shape[1])) for t in half]
    quad = [[t[:, qy::2, qx::2] for t in half] for qy in (0, 1) for qx in (0, 1)]
    whole = [sum(q[j] for q in quad) for j in range(3)]

    def mean(sx, sy, m):
        d = (2 * m).clamp(min=1)
        return torch.stack([torch.div(2 * sx + m, d, rounding_mode="floor"), torch.div(2 * sy + m, d, rounding_mode="floor")], -1), m > 0

    cy = (torch.arange(bh, device=cur.device) * B + B // 2).clamp(max=h - 1)
    cx = (torch.arange(bw, device=cur.device) * B + B // 2).clamp(max=w - 1)
    zero = torch.zeros((n, bh, bw, 2), dtype=torch.int32, device=cur.device)
    cands = [(zero, torch.ones((n, bh, bw), dtype=torch.bool, device=cur.device)), mean(*whole),
             (Q[:, cy][:, :, cx], known[:, cy][:, :, cx])] + [mean(*q) for q in quad]
    ys = torch.arange(h, device=cur.device, dtype=torch.int32)[None, :, None]
    xs = torch.arange(w, device=cur.device, dtype=torch.int32)[None, None, :]
    rf = ref.reshape(n, h * w).to(torch.int32)
    ci = cur.to(torch.int32)
    best = bs = zs = None
    for k, (v, present) in enumerate(cands):
        pix = v.repeat_interleave(B, 1).repeat_interleave(B, 2)[:, :h, :w]
        ix, iy = 4 * xs + pix[..., 0], 4 * ys + pix[..., 1]
        X0, Y0, fx, fy = ix >> 2, iy >> 2, ix & 3, iy & 3
        xa, xb, ya, yb = X0.clamp(0, w - 1), (X0 + 1).clamp(0, w - 1), Y0.clamp(0, h - 1), (Y0 + 1).clamp(0, h - 1)
        tap = lambda y, x: torch.gather(rf, 1, (y * w + x).reshape(n, h * w).long()).view(n, h, w)
        p = ((4 - fx) * (4 - fy) * tap(ya, xa) + fx * (4 - fy) * tap(ya, xb) + (4 - fx) * fy * tap(yb, xa) + fx * fy * tap(yb, xb) + 8) >> 4
        sad = torch.where(present, block_sum((ci - p).abs(), B), torch.full((n, bh, bw), BIG, dtype=torch.int32, device=cur.device))
        if k == 0:
            best, bs, zs = v, sad, sad
        else:
            better = sad < bs
            best, bs = torch.where(better[..., None], v, best), torch.where(better, sad, bs)
    return best.to(torch.int16), torch.stack([bs, zs], -1)


def case(ofc, cf, full, cur, ref, B, refine, rounds, reps):
    n, h, w = cur.shape
    kw = dict(block=B, refine=refine)
    m = min(COMPOSED_N, n)
    routes = {
        "dense": lambda: block_motion(cur, ref, full, **kw),
        "unfused": lambda: upsample_crop_block_motion(ofc, cf, cur, ref, fused=False, **kw),
        "fused": lambda: upsample_crop_block_motion(ofc, cf, cur, ref, **kw),
    }
    a, b = routes["dense"](), routes["fused"]()
    torch.cuda.synchronize()
    assert all(torch.equal(x.view(torch.int32) if x.dtype == torch.uint32 else x, y.view(torch.int32) if y.dtype == torch.uint32 else y)
               for x, y in zip(a, b)), "fused differs from dense"
    if refine == 0:
        cm, cc = composed(cur[:m], ref[:m], full[:m], B)
        torch.cuda.synchronize()
        assert torch.equal(cm, a[0][:m]) and torch.equal(cc, a[1][:m].view(torch.int32)), "the composition differs from the kernel"
        routes_c = lambda: composed(cur[:m], ref[:m], full[:m], B)
        del cm, cc
    st = block_motion(cur, ref, full, stats=True, **kw)[3].sum(0).tolist()
    print("%dx%d x %d gray u8 block %d refine %d: fused == dense bit for bit%s;  SAD %d, zero-vector SAD %d, moved %d, winners %s"
          % (w, h, n, B, refine, ", composed == dense in mv and cost (%d pairs)" % m if refine == 0 else "", st[0], st[1], st[3], st[4:]),
          flush=True)
    del a, b
    for fn in routes.values():                               # warm-up (first-call allocations, code object loads)
        fn()
        fn()
    torch.cuda.synchronize()
    t = {k: [] for k in routes}
    if refine == 0:
        t["composed"] = []
    for _ in range(rounds):
        for k, fn in routes.items():
            t[k].append(timed(fn, reps))
        if refine == 0:
            t["composed"].append(timed(routes_c, 1) * n / m)
    med = {k: statistics.median(v) for k, v in t.items()}
    print("  " + "  ".join("%s %.3f ms (%.3f .. %.3f)" % (k, med[k], min(v), max(v)) for k, v in t.items()), flush=True)
    blocks = -(-h // B) * -(-w // B)
    out = 13.0 * blocks / (h * w)
    bpp = {"dense": 1 + 1 + 8 + out, "fused": 1 + 1 + cf[0].numel() * 4.0 / (h * w) + out}
    px = n * h * w
    print("  ratios: fused/dense %.3f  fused/unfused %.3f%s;  HBM: dense %.2f B/pixel = %.0f GB/s, fused %.2f B/pixel = %.0f GB/s;  "
          "%.1f ns per block (dense)"
          % (med["fused"] / med["dense"], med["fused"] / med["unfused"],
             "  dense/composed %.4f" % (med["dense"] / med["composed"]) if refine == 0 else "",
             bpp["dense"], bpp["dense"] * px / med["dense"] / 1e6, bpp["fused"], bpp["fused"] * px / med["fused"] / 1e6,
             med["dense"] * 1e6 / (n * blocks)), flush=True)


if __name__ == "__main__":
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    if not torch.cuda.is_available():
        sys.exit("time_block_motion: no GPU")
    w, h = 1920, 1080
    g = torch.Generator(device="cuda").manual_seed(3)
    rgb8 = frames(w, h, n, g)
    gray = (((rgb8[..., 0].float() + rgb8[..., 1].float()) + rgb8[..., 2].float()) / 3.0).round().to(torch.uint8)
    del rgb8
    cur, ref = gray[:-1].contiguous(), gray[1:].contiguous()
    ofc = OFClass(F.operating_point(2, w, 1), F.img_params(width=w, height=h), max_batch=n)
    cf = ofc.calc_batch_u8(cur, ref)
    # on the drifting texture nearly every block's candidates coincide and the duplicates are skipped: the second data set adds noise
    # of sigma 1 px to the coarse vectors, so that the seven candidates of a block differ and every one is evaluated
    noisy = cf + torch.randn(cf.shape, device="cuda", generator=g)
    for label, c in (("the engine's flow", cf), ("the engine's flow + noise of sigma 1 px on the coarse vectors", noisy)):
        print(label, flush=True)
        full = ofc.upsample_crop(c)
        for refine in (0, 2):
            case(ofc, c, full, cur, ref, 16, refine, rounds, 5)
        del full
    ofc.close()
