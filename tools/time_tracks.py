#!/usr/bin/env python3
"""Times of the object tracks, HIP events, after a warm-up, the routes alternated within one process (rounds
of A, B, C, ...; the median per route is reported with min .. max), on a sequence of 16 frames of 1920 x 1080 = 15 pairs, through the
C-ABI into outputs allocated once.  Object maps:
  realistic       the ids of label_components (min_area 64, 256 rows) on fit_motion's code of tools/time_objects.py's synthetic
                  scene: an affine camera flow, a dozen rectangles moving on their own, 1 % speckle; most pixels are background
  all foreground  one object covering every frame: every lane of every wave shares one key, all votes land on one counter
  checkerboard    at 4-connectivity with 1024 rows: single-pixel objects, a wave holds up to 128 distinct keys per row; all but the
                  first 1024 components of a frame are background
Routes per map: dense (fotg_object_overlap on a full-resolution flow) and fused (fotg_upsample_crop_object_overlap on a context's
coarse flow); and, on each map,
  torch           the same votes composed from torch operations: index arithmetic, a gather and a bincount over i kb + j
then fotg_object_links and fotg_object_tracks on the realistic votes.  The vote pass is reported against its algorithmic bytes per
pixel: ids 4 B, flow 8 B, mask 1 B and a 4-byte gather = 17 B.
usage: python tools/time_tracks.py [rounds] [frames]"""
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
BYTES = 17


def torch_votes(ids_a, ids_b, flow, mask, ka, kb):
    """votes (n, ka, kb) int64 by index arithmetic and one bincount"""
    n, h, w = ids_a.shape
    ys, xs = torch.meshgrid(torch.arange(h, device="cuda"), torch.arange(w, device="cuda"), indexing="ij")
    u, v = flow[..., 0], flow[..., 1]
    ok = (ids_a >= 0) & (ids_a < ka) & (u.abs() <= 4096) & (v.abs() <= 4096)
    if mask is not None:
        ok &= mask == 0
    xq = xs + torch.where(ok, torch.round(u), 0).to(torch.int64)
    yq = ys + torch.where(ok, torch.round(v), 0).to(torch.int64)
    ok &= (xq >= 0) & (xq < w) & (yq >= 0) & (yq < h)
    lin = (yq.clamp(0, h - 1) * w + xq.clamp(0, w - 1)).reshape(n, -1)
    j = torch.gather(ids_b.reshape(n, -1), 1, lin).reshape(n, h, w)
    ok &= (j >= 0) & (j < kb)
    pair = torch.arange(n, device="cuda").reshape(n, 1, 1)
    key = (pair * ka + ids_a) * kb + j
    return torch.bincount(key[ok], minlength=n * ka * kb).reshape(n, ka, kb)


def case(w, h, frames, rounds):
    L, st_ = F.lib(), _stream(torch.device("cuda", 0))
    n = frames - 1
    flow = realistic(frames, w, h)
    _, code, res = F.fit_motion(flow, code=True, residual=True)
    obj_r, ids_r = F.label_components(code, (1,), 8, res, 64, 256, ids=True)
    del code, res
    ys, xs = torch.meshgrid(torch.arange(h, device="cuda"), torch.arange(w, device="cuda"), indexing="ij")
    board = (((xs + ys) % 2) == 0).to(torch.uint8)[None].repeat(frames, 1, 1).contiguous()
    _, ids_c = F.label_components(board, (1,), 4, None, 1, 1024, ids=True)
    del board
    maps = {"realistic": (ids_r, 256), "all foreground": (torch.zeros_like(ids_r), 256), "checkerboard": (ids_c, 1024)}
    flows = flow[:-1].contiguous()
    mask = (torch.rand((n, h, w), device="cuda", generator=torch.Generator(device="cuda").manual_seed(20)) < 0.05).to(torch.uint8)
    op = F.operating_point(2, w, 1)
    ofc = OFClass(op, F.img_params(width=w, height=h), max_batch=n)
    wl, hl = ofc.out_size()
    coarse = (torch.nn.functional.interpolate(flows.permute(0, 3, 1, 2), size=(hl, wl), mode="bilinear", align_corners=False)
              .permute(0, 2, 3, 1) / float(1 << ofc.op.finest_scale)).contiguous()
    votes = {k: torch.empty((n, kk, kk), dtype=torch.int32, device="cuda") for k, (_, kk) in maps.items()}
    sent = torch.empty((n, 1024, 4), dtype=torch.int64, device="cuda")

    def dense(name):
        ids, kk = maps[name]
        assert L.fotg_object_overlap(0, n, _ptr(ids), _ptr(ids[1:]), w, h, _ptr(flows), _ptr(mask), kk, kk, _ptr(votes[name]), _ptr(sent), st_) == 0

    def fused(name):
        ids, kk = maps[name]
        assert L.fotg_upsample_crop_object_overlap(ofc._h, n, _ptr(coarse), _ptr(ids), _ptr(ids[1:]), _ptr(mask), kk, kk, _ptr(votes[name]),
                                                   _ptr(sent), st_) == 0

    variants = {}
    for name in maps:
        variants[name + " dense"] = lambda name=name: dense(name)
        variants[name + " fused"] = lambda name=name: fused(name)
        variants[name + " torch"] = lambda name=name: torch_votes(maps[name][0][:-1], maps[name][0][1:], flows, mask, maps[name][1], maps[name][1])
    ab = torch.empty((n, 256, 3), dtype=torch.int32, device="cuda")
    ba = torch.empty((n, 256, 3), dtype=torch.int32, device="cuda")
    track = torch.empty((frames, 256), dtype=torch.int32, device="cuda")
    table = torch.empty((1024, 8), dtype=torch.int64, device="cuda")
    tst = torch.empty((4,), dtype=torch.int64, device="cuda")
    dense("realistic")
    variants["links (256 x 256)"] = lambda: L.fotg_object_links(0, n, _ptr(votes["realistic"]), _ptr(obj_r), _ptr(obj_r[1:]), 256, 256, 16, 64,
                                                               _ptr(ab), _ptr(ba), st_)
    variants["links (256 x 256)"]()
    variants["tracks (K 256)"] = lambda: L.fotg_object_tracks(0, n, 256, _ptr(obj_r), _ptr(ab), _ptr(ba), 1024, _ptr(track), _ptr(table), _ptr(tst), st_)

    reps = {}
    for k, fn in variants.items():                           # warm-up (first-call allocations, code object loads), then the window's size
        fn()
        fn()
        torch.cuda.synchronize()
        reps[k] = max(2 if "torch" in k else 3, math.ceil(WINDOW_MS / timed(fn, 2 if "torch" in k else 3)))
    t = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            t[k].append(timed(fn, reps[k]))
    med = {k: statistics.median(v) for k, v in t.items()}
    px = n * h * w
    print("%d pairs of %dx%d, mask with 5 %% rejected" % (n, w, h))
    for k in variants:
        note = ""
        if k.endswith("dense") or k.endswith("fused"):
            name = k.rsplit(" ", 1)[0]
            note = "   %.0f GB/s of %d B per pixel, %.1f x torch" % (px * BYTES / med[k] / 1e6, BYTES, med[name + " torch"] / med[k])
        print("  %-24s %9.4f ms   (min %.4f .. max %.4f, %d calls per window)%s" % (k, med[k], min(t[k]), max(t[k]), reps[k], note), flush=True)
    for name, (ids, kk) in maps.items():
        dense(name)
        ref = torch_votes(ids[:-1], ids[1:], flows, mask, kk, kk)
        torch.cuda.synchronize()
        fg = ((ids[:-1] >= 0) & (ids[:-1] < kk)).float().mean().item()
        print("  %s: %.1f %% foreground, %d votes, torch votes == fotg votes: %s" % (name, 100 * fg, int(ref.sum()), torch.equal(ref.to(torch.int32), votes[name])))
    print("  realistic: %s tracks started, %s links, %s alive at the end" % (tst[0].item(), tst[2].item(), tst[3].item()))


if __name__ == "__main__":
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    frames = int(sys.argv[2]) if len(sys.argv) > 2 else 16
    case(1920, 1080, frames, rounds)
