#!/usr/bin/env python3
"""Times of the motion blur along a flow, HIP events, after a warm-up, the routes alternated within one process
(rounds of A, B, C, ...; the median per route is reported with min .. max), on 64 frames of 1920 x 1080, 8-bit RGB and f32 gray,
shutter 0.5, through the C-ABI into outputs allocated once.  Scenes:
  zero        no motion: every tile takes the copy path
  pan         a uniform pan of 16 px: L = 4, nine taps everywhere
  rectangles  a dozen rectangles moving on their own over a still background
  cap         200 px everywhere: every tile at the cap of 32 px, 65 taps
Routes: dense (fotg_motion_blur on a full-resolution flow), fused (fotg_upsample_crop_motion_blur on a context's coarse flow), warp
(fotg_warp along the same flow: the one-tap floor), and torch, the same filter (half-vectors, tile and neighbour maxima, the tap loop
with both-ended weights, gathers by index) composed from torch operations in float on the first 16 frames, scaled to 64: the same
structure, not the same bytes.  Each pass is reported against its algorithmic bytes per pixel.
With `quality` as the first argument: alley_1 frames 1 .. 3 of tests/golden, motion_blur(frame 2, flow 2 -> 3, shutter 1) against the
mean of eight interpolated frames at sub-frame times spanning [-0.5, 0.5] around frame 2, as PSNR, next to the unblurred frame 2.
usage: python tools/time_motionblur.py [rounds] [frames] | quality"""
import math
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import flowonthego_amd as F                                   # noqa: E402
from flowonthego_amd.oflow import OFClass, _ptr, _stream       # noqa: E402
from time_bidir import timed                                  # noqa: E402

WINDOW_MS = 200.0
S256, MAX_BLUR, TORCH_N = 128, 32, 16


def scenes(n, w, h):
    z = torch.zeros((n, h, w, 2), device="cuda")
    pan = torch.tensor([16.0, 0.0], device="cuda").repeat(n, h, w, 1).contiguous()
    rect = torch.zeros((n, h, w, 2), device="cuda")
    for i in range(n):
        for k in range(12):
            rw, rh = 60 + (37 * k + 11 * i) % 240, 40 + (53 * k + 7 * i) % 160
            x0, y0 = (131 * k + 17 * i) % (w - rw), (89 * k + 29 * i) % (h - rh)
            rect[i, y0:y0 + rh, x0:x0 + rw] = torch.tensor([4.0 * (6.0 - k), 4.0 * (k - 5.5)], device="cuda")
    cap = torch.tensor([200.0, 0.0], device="cuda").repeat(n, h, w, 1).contiguous()
    return {"zero": z, "pan": pan, "rectangles": rect, "cap": cap}


def torch_blur(frame, flow):
    """the filter in float: frame (n, h, w[, c]), flow (n, h, w, 2) -> the blurred frame, float32"""
    n, h, w = flow.shape[:3]
    img = frame.reshape(n, h, w, -1).float()
    s = S256 / 32.0
    H = torch.round(flow * s)
    ln = torch.linalg.vector_norm(H, dim=-1, keepdim=True)
    H = torch.where(ln > 16.0 * MAX_BLUR, H * (16.0 * MAX_BLUR) / ln.clamp(min=1.0), H)
    sq = (H * H).sum(-1)
    th, tw = -(-h // 32), -(-w // 32)
    pad = torch.nn.functional.pad(sq, (0, tw * 32 - w, 0, th * 32 - h), value=-1.0)
    tsq, arg = pad.reshape(n, th, 32, tw, 32).permute(0, 1, 3, 2, 4).reshape(n, th, tw, 1024).max(-1)
    Hp = torch.nn.functional.pad(H, (0, 0, 0, tw * 32 - w, 0, th * 32 - h))
    tm = torch.gather(Hp.reshape(n, th, 32, tw, 32, 2).permute(0, 1, 3, 2, 4, 5).reshape(n, th, tw, 1024, 2), 3,
                      arg[..., None, None].expand(n, th, tw, 1, 2))[..., 0, :]
    nsq, narg = torch.nn.functional.max_pool2d(tsq[:, None], 3, 1, 1, return_indices=True)
    D = torch.gather(tm.reshape(n, th * tw, 2), 1, narg.reshape(n, th * tw, 1).expand(n, th * tw, 2)).reshape(n, th, tw, 2)
    D = D.repeat_interleave(32, 1).repeat_interleave(32, 2)[:, :h, :w]
    lenD = torch.linalg.vector_norm(D, dim=-1)
    L = torch.ceil(lenD / 16.0)
    Ls, lens = L.clamp(min=1.0), lenD.clamp(min=1.0)
    ys, xs = torch.meshgrid(torch.arange(h, device="cuda"), torch.arange(w, device="cuda"), indexing="ij")
    base = (torch.arange(n, device="cuda") * (h * w)).reshape(n, 1, 1)
    Hf, imf = H.reshape(-1, 2), img.reshape(n * h * w, -1)
    rX = (H * D).sum(-1).abs() / lens
    acc, W = torch.zeros_like(img), torch.zeros((n, h, w), device="cuda")
    for k in range(-int(L.max().item()), int(L.max().item()) + 1):
        o = torch.round(D * (k / Ls)[..., None])
        cx = (xs + torch.floor((o[..., 0] + 8.0) / 16.0).long()).clamp(0, w - 1)
        cy = (ys + torch.floor((o[..., 1] + 8.0) / 16.0).long()).clamp(0, h - 1)
        idx = (base + cy * w + cx).reshape(-1)
        rY = ((Hf[idx].reshape(n, h, w, 2) * D).sum(-1).abs() / lens)
        wk = (torch.maximum(rY, rX) + 16.0 - lenD * abs(k) / Ls).clamp(0.0, 16.0)
        wk = torch.where((abs(k) <= L) & (lenD >= 8.0), wk, 16.0 if k == 0 else 0.0)
        acc += wk[..., None] * imf[idx].reshape(n, h, w, -1)
        W += wk
    return (acc / W[..., None]).reshape(frame.shape)


def case(w, h, n, rounds):
    L, st_ = F.lib(), _stream(torch.device("cuda", 0))
    g = torch.Generator(device="cuda").manual_seed(23)
    flows = scenes(n, w, h)
    frames = {"u8 rgb": (torch.rand((n, h, w, 3), device="cuda", generator=g) * 255).to(torch.uint8),
              "f32 gray": torch.rand((n, h, w), device="cuda", generator=g) * 255}
    op = F.operating_point(2, w, 1)
    ofc = OFClass(op, F.img_params(width=w, height=h), max_batch=n)
    wl, hl = ofc.out_size()
    coarse = {k: (torch.nn.functional.interpolate(f.permute(0, 3, 1, 2), size=(hl, wl), mode="bilinear", align_corners=False)
                  .permute(0, 2, 3, 1) / float(1 << ofc.op.finest_scale)).contiguous() for k, f in flows.items()}
    outs = {k: torch.empty_like(v) for k, v in frames.items()}
    stats = torch.empty((n, 8), dtype=torch.int64, device="cuda")

    def run(sc, kind, fused, st=None):
        fr, ty, ch = frames[kind], 0 if kind == "u8 rgb" else 1, 3 if kind == "u8 rgb" else 1
        if fused:
            r = L.fotg_upsample_crop_motion_blur(ofc._h, n, _ptr(fr), ty, ch, _ptr(coarse[sc]), None, S256, MAX_BLUR, _ptr(outs[kind]), None, None, _ptr(st), st_)
        else:
            r = L.fotg_motion_blur(0, n, _ptr(fr), ty, ch, _ptr(flows[sc]), w, h, None, S256, MAX_BLUR, _ptr(outs[kind]), None, None, _ptr(st), st_)
        assert r == 0

    def warp(sc, kind):
        fr = frames[kind]
        fn = L.fotg_warp_u8 if kind == "u8 rgb" else L.fotg_warp
        import ctypes as C
        assert fn(0, n, _ptr(fr), _ptr(flows[sc]), w, h, 3 if kind == "u8 rgb" else 1, None, None, 0, C.c_float(0.0), _ptr(outs[kind]), None, None, st_) == 0

    variants, nbytes = {}, {}
    for sc in flows:
        for kind in frames:
            el = 3 if kind == "u8 rgb" else 4
            name = "%s, %s" % (sc, kind)
            variants[name + " dense"] = lambda sc=sc, kind=kind: run(sc, kind, False)
            variants[name + " fused"] = lambda sc=sc, kind=kind: run(sc, kind, True)
            variants[name + " warp"] = lambda sc=sc, kind=kind: warp(sc, kind)
            variants[name + " torch"] = lambda sc=sc, kind=kind: torch_blur(frames[kind][:TORCH_N], flows[sc][:TORCH_N])
            nbytes[name + " dense"] = 8 + 4 + 4 + 2 * el           # flow in, H out and in, the frame in and out
            nbytes[name + " fused"] = 2 + 4 + 4 + 2 * el           # a coarse vector per four pixels instead
            nbytes[name + " warp"] = 8 + 2 * el
    reps = {}
    for k, fn in variants.items():                           # warm-up (first-call allocations, code object loads), then the window's size
        fn()
        fn()
        torch.cuda.synchronize()
        reps[k] = max(2, math.ceil(WINDOW_MS / timed(fn, 2))) if "torch" not in k else 1
    t = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            t[k].append(timed(fn, reps[k]) * (n / TORCH_N if k.endswith("torch") else 1.0))
    med = {k: statistics.median(v) for k, v in t.items()}
    px = n * h * w
    print("%d frames of %dx%d, shutter256 %d, max_blur %d (torch: %d frames, scaled)" % (n, w, h, S256, MAX_BLUR, TORCH_N))
    for k in variants:
        note = ""
        if not k.endswith("torch"):
            note = "   %.2f TB/s of %d B per pixel, %.1f x torch" % (px * nbytes[k] / med[k] / 1e9, nbytes[k], med[k.rsplit(" ", 1)[0] + " torch"] / med[k])
        print("  %-32s %9.4f ms   (min %.4f .. max %.4f, %d calls per window)%s" % (k, med[k], min(t[k]), max(t[k]), reps[k], note), flush=True)
    for sc in flows:
        run(sc, "u8 rgb", False, stats)
        torch.cuda.synchronize()
        s = stats.sum(0).tolist()
        ref = torch_blur(frames["u8 rgb"][:2], flows[sc][:2])
        d = (outs["u8 rgb"][:2].float() - ref).abs()
        print("  %-10s codes %s  taps per pixel %.2f  copy tiles %d  |fotg - torch| mean %.4f max %.1f" % (sc, s[:4], s[4] / px, s[5], d.mean().item(), d.max().item()))
    ofc.close()


def quality():
    def psnr(a, b):
        mse = float(((a.double() - b.double()) ** 2).mean().item())
        return float("inf") if mse == 0 else 10.0 * math.log10(255.0 ** 2 / mse)

    g = os.path.join(ROOT, "tests", "golden")
    z, more = np.load(os.path.join(g, "alley_1_gray.npz")), np.load(os.path.join(g, "alley_1_more.npz"))
    f1, f2, f3 = (torch.from_numpy(a).cuda() for a in (z["frame_0001"], z["frame_0002"], more["frame_0003"]))
    h, w = f2.shape
    op = F.operating_point(2, w, 1)
    op.bidir = True
    ofc = OFClass(op, F.img_params(width=w, height=h), max_batch=2)
    fw, bw = ofc.calc_sequence_bidirectional(torch.stack([f1, f2, f3]))
    dfw, dbw = ofc.upsample_crop(fw).clone(), ofc.upsample_crop(bw).clone()
    # sub-frame times -0.4375 .. 0.4375 around frame 2: four between frames 1 and 2, four between frames 2 and 3
    ts = [(-0.5 + (j + 0.5) / 8.0) for j in range(8)]
    subs = [F.interpolate(f1, f2, dfw[0], dbw[0], 1.0 + t_) if t_ < 0 else F.interpolate(f2, f3, dfw[1], dbw[1], t_) for t_ in ts]
    target = torch.stack([s.float() for s in subs]).mean(0)
    blurred, st = F.motion_blur(f2, dfw[1], None, 1.0, 32, stats=True)
    print("alley_1 frame 2, %dx%d, shutter 1: PSNR against the mean of eight interpolated sub-frames: blurred %.3f dB, unblurred %.3f dB"
          % (w, h, psnr(blurred, target), psnr(f2, target)))
    print("  codes %s  taps per pixel %.2f  copy tiles %d  longest half-streak %.2f px" % (st[:4].tolist(), st[4].item() / (h * w), st[5].item(), st[6].item() / 16.0))
    ofc.close()


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "quality":
        quality()
    else:
        rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
        frames = int(sys.argv[2]) if len(sys.argv) > 2 else 64
        case(1920, 1080, frames, rounds)
