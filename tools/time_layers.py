#!/usr/bin/env python3
"""Times of the motion layers, HIP events, after a warm-up, the routes alternated within one process (rounds
of A, B, C, ...; the median per route is reported), on a batch of 64 flows of 1920 x 1080, the affine model, iters 3, rounds 3.
Every timed window is a few hundred milliseconds of back-to-back calls through the C-ABI into outputs allocated once.
Scenes: three (the three-motion scene of tests/layers_ref.py at this size), uniform (one translation), board (4 x 4 squares of two
translations: every wave holds two layers; seeded, every layer of it dies at the mean of the two, so it is run from the two
translations as init only, without the call and seed routes).  The shares of the pixels the layers hold are printed and asserted
per scene.  Routes per scene and K in (2, 4, 8):
  call         the whole call with labels, residual, records and stats
  seeded r=R   from init (the call's own result), R refinement rounds, no final pass: (r=4 - r=1) / 3 is one assign round
               (assign pass, fold, solve)
  seed i=I     no init, no refinement, no final pass, iters I: (i=3 - i=0) / (3 K) is one seeding round; with K = 2 and K = 1,
               (K=2 i=0) - (K=1 i=0) - one seeding round is the tile pass with its selection
  final        from init, no rounds: the final pass alone
  fit pass     fotg_fit_motion, iters 0, params only: one streaming pass over the flows, the floor of a pass
  torch        one assignment and the K x 12 sums composed from torch operations (f32 residuals, argmin, masked int64 sums), on
               8 of the flows; the ratio printed scales it to the batch
  fused/dense  the whole call through the context, both settings of `fused`
Each pass is reported against its algorithmic bytes: the flows once, 8 B per pixel (1.06 GB for the batch).
usage: python tools/time_layers.py [rounds] [n]"""
import ctypes as C
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import flowonthego_amd as F                                   # noqa: E402
from flowonthego_amd.oflow import OFClass, _ptr, _stream      # noqa: E402
from time_bidir import timed                                  # noqa: E402

WINDOW_MS = 200.0
TORCH_N = 8                    # the torch route runs on this many of the flows (its temporaries are twelve int64 images per flow)
P_BG = (0.004, -0.011, 1.75, 0.009, 0.006, -2.5)
P_B = (0.03 / 6, -0.02 / 6, -7.0, 0.02 / 6, 0.03 / 6, 3.0)          # the scene's affine object, its slopes scaled with the size


def scene(kind, n, w, h):
    g = torch.Generator(device="cuda").manual_seed(5)
    ys, xs = torch.meshgrid(torch.arange(h, device="cuda", dtype=torch.float32), torch.arange(w, device="cuda", dtype=torch.float32), indexing="ij")
    aff = lambda P: torch.stack([P[0] * xs + P[1] * ys + P[2], P[3] * xs + P[4] * ys + P[5]], -1)
    if kind == "uniform":
        f = torch.empty((h, w, 2), device="cuda")
        f[..., 0], f[..., 1] = 1.25, -0.5
        return f[None].repeat(n, 1, 1, 1).contiguous()
    if kind == "board":
        sq = ((ys.long() // 4 + xs.long() // 4) % 2).bool()[..., None]
        f = torch.where(sq, torch.tensor([2.0, 0.0], device="cuda"), torch.tensor([-1.0, 3.0], device="cuda"))
        return f[None].repeat(n, 1, 1, 1).contiguous()
    f = aff(P_BG)
    f[h // 8:h // 8 + h // 3, w // 10:w // 10 + w // 4] = torch.tensor([6.5, -4.0], device="cuda")
    f[h // 2:h // 2 + h // 3, w // 2:w // 2 + w // 3] = aff(P_B)[h // 2:h // 2 + h // 3, w // 2:w // 2 + w // 3]
    f = f[None].repeat(n, 1, 1, 1)
    return (f + 0.2 * torch.randn(f.shape, device="cuda", generator=g)).contiguous()


def torch_route(flow, params, thresh=1.0):
    """one assignment and the twelve sums per layer"""
    n, h, w, _ = flow.shape
    K = params.shape[1]
    X = (2 * torch.arange(w, device="cuda") - (w - 1))[None, None, :]
    Y = (2 * torch.arange(h, device="cuda") - (h - 1))[None, :, None]
    u, v = flow[..., 0], flow[..., 1]
    adm = (u.abs() <= 4096) & (v.abs() <= 4096)
    x, y = ((X + (w - 1)) / 2).float(), ((Y + (h - 1)) / 2).float()
    p = params.float()
    r = torch.stack([(u - (p[:, k, 0, None, None] * x + p[:, k, 1, None, None] * y + p[:, k, 2, None, None])) ** 2 +
                     (v - (p[:, k, 3, None, None] * x + p[:, k, 4, None, None] * y + p[:, k, 5, None, None])) ** 2 for k in range(K)], 1)
    rb, best = r.min(1)
    joined = adm & (rb <= thresh * thresh)
    U, V = torch.round(u * 256).long(), torch.round(v * 256).long()
    terms = (torch.ones_like(U), X + 0 * U, Y + 0 * U, X * X + 0 * U, X * Y + 0 * U, Y * Y + 0 * U, U, X * U, Y * U, V, X * V, Y * V)
    sums = torch.stack([torch.stack([(t * (joined & (best == k))).sum(dim=(1, 2)) for t in terms], -1) for k in range(K)], 1)
    return torch.where(joined, best, 253).to(torch.uint8), sums


def case(w, h, n, rounds):
    L, th = F.lib(), C.c_float(1.0)
    op = F.operating_point(2, w, 1)
    ofc = OFClass(op, F.img_params(width=w, height=h), max_batch=n)
    st_ = _stream(ofc.device)
    gb = n * h * w * 8 / 1e9
    print("%d x %dx%d flows, affine, iters 3, rounds 3, %.3f GB of flow per pass" % (n, w, h, gb))
    lab = torch.empty((n, h, w), dtype=torch.uint8, device="cuda")
    res = torch.empty((n, h, w, 2), device="cuda")
    st = torch.empty((n, 4), dtype=torch.int64, device="cuda")
    fit_prm = torch.empty((n, 6), dtype=torch.float64, device="cuda")
    for kind in ("three", "uniform", "board"):
        flow = scene(kind, n, w, h)
        variants = {}
        for K in (1, 2, 4, 8):
            prm = torch.empty((n, K, 6), dtype=torch.float64, device="cuda")
            rec = torch.empty((n, K, 8), dtype=torch.int64, device="cuda")
            if kind == "board":                              # (seeded, every layer of the board dies at the mean of the two motions)
                init = torch.tensor([[0, 0, 2.0, 0, 0, 0.0], [0, 0, -1.0, 0, 0, 3.0]] + [[0, 0, 50.0 + k, 0, 0, 50.0] for k in range(2, K)],
                                    dtype=torch.float64, device="cuda")[:K][None].repeat(n, 1, 1).contiguous()
            else:
                init = F.motion_layers(flow, layers=K).clone()
            # what the seeded routes measure, from the records of the call they repeat: the share of the pixels each layer holds
            share = F.motion_layers(flow, layers=K, init=init, records=True)[1][:, :, 0].double().mean(0) / (h * w)
            print("scene %s K=%d: shares of the layers after init + 3 rounds: %s" % (kind, K, " ".join("%.3f" % s for s in share.tolist())), flush=True)
            if kind == "board" and K > 1:
                assert 0.45 < share[0] < 0.55 and 0.45 < share[1] < 0.55, "the board's two layers must hold half the pixels each"
            if kind == "uniform":
                assert share[0] > 0.999, "the uniform flow's layer 0 must hold every pixel"
            if kind == "three" and K > 1:
                assert int((share > 0.03).sum()) == min(K, 3), "the scene's motions must each be a layer"

            def call(K=K, prm=prm, rec=rec, init=None, iters=3, rnds=3, final=True):
                assert L.fotg_motion_layers(0, n, _ptr(flow), None, w, h, K, 2, iters, rnds, th, _ptr(init), _ptr(prm),
                                            *((_ptr(lab), _ptr(res), _ptr(rec), _ptr(st)) if final else (None,) * 4), None, st_) == 0

            if K > 1:
                if kind != "board":
                    variants["K=%d call" % K] = call
                for R in (1, 4):
                    variants["K=%d seeded r=%d" % (K, R)] = lambda call=call, init=init, R=R: call(init=init, rnds=R, final=False)
                variants["K=%d final" % K] = lambda call=call, init=init: call(init=init, rnds=0)
                variants["K=%d torch" % K] = lambda init=init: torch_route(flow[:TORCH_N], init[:TORCH_N])
            if kind != "board" and (K <= 2 or kind == "three"):
                for I in (0, 3):
                    variants["K=%d seed i=%d" % (K, I)] = lambda call=call, I=I: call(iters=I, rnds=0, final=False)
        variants["fit pass"] = lambda: L.fotg_fit_motion(0, n, _ptr(flow), None, w, h, 2, 0, th, _ptr(fit_prm), None, None, None, None, st_)
        reps = {}
        for k, fn in variants.items():                           # warm-up (first-call allocations, code object loads), then the window's size
            fn()
            fn()
            torch.cuda.synchronize()
            reps[k] = max(3, math.ceil(WINDOW_MS / timed(fn, 3)))
        t = {k: [] for k in variants}
        for _ in range(rounds):
            for k, fn in variants.items():
                t[k].append(timed(fn, reps[k]))
        med = {k: statistics.median(v) for k, v in t.items()}
        print("scene %s" % kind)
        for k in variants:
            print("  %-22s %9.4f ms   (min %.4f .. max %.4f, %d calls per window)" % (k, med[k], min(t[k]), max(t[k]), reps[k]), flush=True)
        fp = med["fit pass"]
        for K in (2, 4, 8):
            a = (med["K=%d seeded r=4" % K] - med["K=%d seeded r=1" % K]) / 3
            print("  K=%d: an assign round %.4f ms (%.0f GB/s, %.2f fit passes), the final pass %.4f ms, torch %.1f x an assign round"
                  % (K, a, gb / a * 1e3, a / fp, med["K=%d final" % K], med["K=%d torch" % K] * (n / min(n, TORCH_N)) / a), flush=True)
        if kind == "board":
            continue
        ks = (1, 2, 4, 8) if kind == "three" else (1, 2)
        sr = {K: (med["K=%d seed i=3" % K] - med["K=%d seed i=0" % K]) / (3 * K) for K in ks}
        print("  a seeding round: " + ", ".join("K=%d %.4f ms" % (K, sr[K]) for K in ks)
              + "; the tile pass and selection of layer 1: %.4f ms" % (med["K=2 seed i=0"] - med["K=1 seed i=0"] - sr[2]), flush=True)
    # the context's forms, on the three-motion scene's coarse flows
    wl, hl = ofc.out_size()
    sc = float(1 << op.finest_scale)
    cf = (torch.nn.functional.interpolate(scene("three", n, w, h).permute(0, 3, 1, 2), size=(hl, wl), mode="bilinear").permute(0, 2, 3, 1) / sc).contiguous()
    variants = {"%s K=%d" % ("fused" if fu else "dense", K): (lambda fu=fu, K=K: ofc.upsample_crop_motion_layers(cf, layers=K, labels=True, fused=fu))
                for K in (2, 4, 8) for fu in (False, True)}
    reps = {}
    for k, fn in variants.items():
        fn()
        fn()
        torch.cuda.synchronize()
        reps[k] = max(3, math.ceil(WINDOW_MS / timed(fn, 3)))
    t = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            t[k].append(timed(fn, reps[k]))
    print("through the context (upsample_crop_motion_layers, labels)")
    for k in variants:
        print("  %-22s %9.4f ms   (min %.4f .. max %.4f)" % (k, statistics.median(t[k]), min(t[k]), max(t[k])), flush=True)
    ofc.close()


if __name__ == "__main__":
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    case(1920, 1080, n, rounds)
