#!/usr/bin/env python3
"""Times of the motion histograms, HIP events, after a warm-up, the routes alternated within one process
(rounds of A, B, C, ...; the median per route is reported with min .. max), on 64 flows of 1920 x 1080, through the C-ABI into
outputs allocated once, with a mask (5 % rejected) and the affine parameters of fit_motion.  Flows:
  noisy       tools/time_objects.py's synthetic scene (an affine camera flow, a dozen rectangles moving on their own, 1 % speckle)
              plus Gaussian noise of half a pixel: neighbouring lanes fall into different bins
  uniform     one vector everywhere and no parameters: every lane of every wave adds to the same two bins, the worst contention
Object maps: realistic, the ids of label_components (min_area 64, 256 rows) on fit_motion's code of the scene, most pixels background;
one object covering every frame.
Routes: dense (fotg_motion_histograms on a full-resolution flow) and fused (fotg_upsample_crop_motion_histograms on a context's coarse
flow), each for cells only (cell 16), objects only, and both; and torch, the same quantities (residual, magnitude, angle, soft
binning, scatter_add per cell and per object) composed from torch operations in float: the same structure, not the same bytes.
Each pass is reported against its algorithmic bytes per pixel: flow 8 B, mask 1 B, ids 4 B where objects are asked for.
usage: python tools/time_histograms.py [rounds] [flows]"""
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import flowonthego_amd as F                                   # noqa: E402
from flowonthego_amd.oflow import OFClass, _ptr, _stream       # noqa: E402
from time_bidir import timed                                  # noqa: E402
from time_objects import realistic                            # noqa: E402

WINDOW_MS = 200.0
CELL, ROWS, T256 = 16, 256, 102


def torch_histograms(flow, mask, params, ids, cells, objects):
    """HOF, MBHx and MBHy with the zero bin and the pixel count, float32, per cell (n, gh, gw, 26) and/or per object (n, ROWS, 26)"""
    n, h, w = flow.shape[:3]
    ys, xs = torch.meshgrid(torch.arange(h, device="cuda", dtype=torch.float32), torch.arange(w, device="cuda", dtype=torch.float32), indexing="ij")
    if params is not None:
        p = params.to(torch.float32).reshape(n, 6, 1, 1)
        flow = flow - torch.stack([p[:, 0] * xs + p[:, 1] * ys + p[:, 2], p[:, 3] * xs + p[:, 4] * ys + p[:, 5]], -1)
    u, v = flow[..., 0] * 256.0, flow[..., 1] * 256.0
    ok = (u.abs() <= 1048576.0) & (v.abs() <= 1048576.0) & (mask == 0)
    u, v = torch.where(ok, u, 0.0), torch.where(ok, v, 0.0)
    feat = torch.zeros((n, h, w, 26), device="cuda")

    def soft(off, a, b, sel):
        m = torch.hypot(a, b)
        pos = torch.remainder(torch.atan2(b, a) * (4.0 / math.pi), 8.0)
        b0 = pos.floor()
        fr = pos - b0
        b0 = b0.to(torch.int64) % 8
        m = torch.where(sel, m, 0.0)
        feat.scatter_add_(3, (off + b0).unsqueeze(-1), (m * (1.0 - fr)).unsqueeze(-1))
        feat.scatter_add_(3, (off + (b0 + 1) % 8).unsqueeze(-1), (m * fr).unsqueeze(-1))

    m = torch.hypot(u, v)
    zero = ok & (m < T256)
    feat[..., 24] = zero
    feat[..., 25] = ok
    soft(0, u, v, ok & ~zero)
    okp = torch.nn.functional.pad(ok[:, None].float(), (1, 1, 1, 1), mode="replicate")[:, 0] > 0
    part = ok & okp[:, 1:-1, :-2] & okp[:, 1:-1, 2:] & okp[:, :-2, 1:-1] & okp[:, 2:, 1:-1]
    for k, c in enumerate((u, v)):
        cp = torch.nn.functional.pad(c[:, None], (1, 1, 1, 1), mode="replicate")[:, 0]
        soft(8 + 8 * k, cp[:, 1:-1, 2:] - cp[:, 1:-1, :-2], cp[:, 2:, 1:-1] - cp[:, :-2, 1:-1], part)
    out = []
    if cells:
        gh, gw = (h + CELL - 1) // CELL, (w + CELL - 1) // CELL
        idx = ((torch.arange(h, device="cuda") // CELL)[:, None] * gw + (torch.arange(w, device="cuda") // CELL)[None, :]).reshape(1, h * w, 1)
        out.append(torch.zeros((n, gh * gw, 26), device="cuda").scatter_add_(1, idx.expand(n, h * w, 26), feat.reshape(n, h * w, 26)))
    if objects:
        inside = (ids >= 0) & (ids < ROWS)
        idx = torch.where(inside, ids, ROWS).to(torch.int64).reshape(n, h * w, 1)
        out.append(torch.zeros((n, ROWS + 1, 26), device="cuda").scatter_add_(1, idx.expand(n, h * w, 26), feat.reshape(n, h * w, 26))[:, :ROWS])
    return out


def case(w, h, n, rounds):
    L, st_ = F.lib(), _stream(torch.device("cuda", 0))
    g = torch.Generator(device="cuda").manual_seed(22)
    scene = realistic(n, w, h)
    params, code, res = F.fit_motion(scene, code=True, residual=True)
    _, ids_r = F.label_components(code, (1,), 8, res, 64, ROWS, ids=True)
    del code, res
    flows = {"noisy": (scene + 0.5 * torch.randn(scene.shape, device="cuda", generator=g)).contiguous(),
             "uniform": torch.tensor([3.25, -1.5], device="cuda").repeat(n, h, w, 1).contiguous()}
    del scene
    prm = {"noisy": params, "uniform": None}
    maps = {"realistic": ids_r, "one object": torch.zeros_like(ids_r)}
    mask = (torch.rand((n, h, w), device="cuda", generator=g) < 0.05).to(torch.uint8)
    op = F.operating_point(2, w, 1)
    ofc = OFClass(op, F.img_params(width=w, height=h), max_batch=n)
    wl, hl = ofc.out_size()
    coarse = {k: (torch.nn.functional.interpolate(f.permute(0, 3, 1, 2), size=(hl, wl), mode="bilinear", align_corners=False)
                  .permute(0, 2, 3, 1) / float(1 << ofc.op.finest_scale)).contiguous() for k, f in flows.items()}
    cells = torch.empty((n, (h + CELL - 1) // CELL, (w + CELL - 1) // CELL, 32), dtype=torch.int64, device="cuda")
    objs = torch.empty((n, ROWS, 32), dtype=torch.int64, device="cuda")

    def run(fl, mp, c, o, fused):
        ids = maps[mp] if o else None
        if fused:
            st = L.fotg_upsample_crop_motion_histograms(ofc._h, n, _ptr(coarse[fl]), _ptr(mask), _ptr(prm[fl]), CELL, T256, _ptr(cells) if c else None,
                                                        _ptr(ids), ROWS, _ptr(objs) if o else None, st_)
        else:
            st = L.fotg_motion_histograms(0, n, _ptr(flows[fl]), w, h, _ptr(mask), _ptr(prm[fl]), CELL, T256, _ptr(cells) if c else None, _ptr(ids),
                                          ROWS, _ptr(objs) if o else None, st_)
        assert st == 0

    variants, nbytes = {}, {}
    for fl, mp, c, o in (("noisy", "realistic", True, False), ("noisy", "realistic", False, True), ("noisy", "realistic", True, True),
                         ("noisy", "one object", True, True), ("uniform", "realistic", True, False), ("uniform", "one object", True, True),
                         ("uniform", "one object", False, True)):
        name = "%s, %s%s" % (fl, "cells" if c and not o else ("objects" if o and not c else "both"), "" if not o else " (%s)" % mp)
        for route in ("dense", "fused", "torch"):
            if route == "torch":
                variants[name + " torch"] = lambda fl=fl, mp=mp, c=c, o=o: torch_histograms(flows[fl], mask, prm[fl], maps[mp], c, o)
            else:
                variants[name + " " + route] = lambda fl=fl, mp=mp, c=c, o=o, fu=route == "fused": run(fl, mp, c, o, fu)
            nbytes[name + " " + route] = 9 + (4 if o else 0)

    reps = {}
    for k, fn in variants.items():                           # warm-up (first-call allocations, code object loads), then the window's size
        fn()
        fn()
        torch.cuda.synchronize()
        reps[k] = max(2, math.ceil(WINDOW_MS / timed(fn, 2))) if "torch" not in k else 1
    t = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            t[k].append(timed(fn, reps[k]))
    med = {k: statistics.median(v) for k, v in t.items()}
    px = n * h * w
    print("%d flows of %dx%d, cell %d, %d rows, mask with 5 %% rejected" % (n, w, h, CELL, ROWS))
    for k in variants:
        note = ""
        if not k.endswith("torch"):
            note = "   %.0f GB/s of %d B per pixel, %.1f x torch" % (px * nbytes[k] / med[k] / 1e6, nbytes[k], med[k.rsplit(" ", 1)[0] + " torch"] / med[k])
        print("  %-44s %9.4f ms   (min %.4f .. max %.4f, %d calls per window)%s" % (k, med[k], min(t[k]), max(t[k]), reps[k], note), flush=True)
    # the float form agrees with the integer one in structure: the relative L1 distance of the image's summed bins
    run("noisy", "realistic", True, True, False)
    ref = torch_histograms(flows["noisy"], mask, prm["noisy"], maps["realistic"], True, True)
    torch.cuda.synchronize()
    got = cells.reshape(-1, 32).sum(0).double()
    want = ref[0].reshape(-1, 26).sum(0).double()
    for nm, a, b in (("HOF", got[0:8], want[0:8]), ("MBHx", got[9:17], want[8:16]), ("MBHy", got[17:25], want[16:24])):
        print("  %s: |fotg - torch|_1 / |torch|_1 = %.2e" % (nm, ((a - b).abs().sum() / b.abs().sum()).item()))
    fg = ((ids_r >= 0) & (ids_r < ROWS)).float().mean().item()
    print("  zero bin: fotg %d, torch %d of %d admissible; realistic map: %.1f %% foreground" % (got[8].item(), want[24].item(), got[25].item(), 100 * fg))


if __name__ == "__main__":
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    flows = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    case(1920, 1080, flows, rounds)
