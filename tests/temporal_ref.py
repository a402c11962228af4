"""numpy float32 restatement of the motion-compensated temporal filter (csrc/temporal.hip.h, include/fotg.h fotg_temporal_filter) on
top of warp_ref.warp: every operation separately rounded to f32, in the kernel's order, so the GPU's dst and used equal these byte
for byte.  The 3 x 3 window with replicated edges is np.pad(..., mode="edge"), summed separably: rows first, then columns."""
import math
import os

import numpy as np

import warp_ref as W

f32 = np.float32


def scale_of(tau, channels):
    """1.0f / (tau * (float)(9 channels)) in f32"""
    return f32(1) / (f32(tau) * f32(9 * channels))


def box3(d):
    """e = the separable 3 x 3 box sum of d (h, w) f32 with replicated edges, in the definition's order"""
    p = np.pad(d, ((0, 0), (1, 1)), mode="edge")
    r = (p[:, :-2] + p[:, 1:-1]) + p[:, 2:]
    p = np.pad(r, ((1, 1), (0, 0)), mode="edge")
    e = (p[:-2] + p[1:-1]) + p[2:]
    assert e.dtype == f32
    return e


def filter_one(frames, c, nbrs, flows, masks=None, tau=30.0, gains=None, ref=None, terms=False):
    """frames: (T, h, w) or (T, h, w, ch) float32 or uint8; c: the centre's index; nbrs: K indices (-1 = absent); flows: (K, h, w, 2);
    masks: None or (K, h, w) uint8; gains: None or K floats; ref: None or one image of frames' layout.
    Returns dst (a frame's shape and dtype), used (h, w) uint8, stats (4,) float64 [sums added with math.fsum] and, with terms=True,
    the two lists of residual terms (float64 arrays, each term an f32 widened exactly)."""
    frames = np.asarray(frames)
    u8 = frames.dtype == np.uint8
    T, h, w = frames.shape[:3]
    Cf = frames[c].astype(f32).reshape(h, w, -1)
    noc = Cf.shape[2]
    K = len(nbrs)
    scale = scale_of(tau, noc)
    num, den = Cf.copy(), np.ones((h, w), f32)
    used = np.zeros((h, w), np.uint8)
    with np.errstate(all="ignore"):
        for k in range(K):
            b = int(nbrs[k])
            if b < 0:
                continue
            g = f32(1 if gains is None else gains[k])
            # fotg_warp in its reference fill mode with fill 0: the value of the clamped taps wherever own != 3, else 0
            Wk, code, _ = W.warp(frames[b].astype(f32), flows[k], None, None if masks is None else masks[k], 0, 0.0)
            Wk = Wk.reshape(h, w, noc)
            d = np.abs(Cf[..., 0] - Wk[..., 0])
            for ch in range(1, noc):
                d = d + np.abs(Cf[..., ch] - Wk[..., ch])
            e = box3(d.astype(f32))
            wt = g * (f32(1) - e * scale)
            assert wt.dtype == f32
            use = (code == 0) & (wt > 0)
            wz = np.where(use, wt, f32(0))
            num = np.where(use[..., None], num + wz[..., None] * Wk, num)
            den = np.where(use, den + wz, den)
            used += use.astype(np.uint8)
        value = (num / den[..., None]).astype(f32)
    assert num.dtype == f32 and den.dtype == f32
    dst = (W.to_u8(value) if u8 else value).reshape(frames.shape[1:])
    stats = np.zeros(4, np.float64)
    stats[0], stats[1] = float(used.sum(dtype=np.int64)), float((used == 0).sum())
    tv = tc = np.zeros(0, np.float64)
    if ref is not None:
        R = np.asarray(ref).astype(f32).reshape(h, w, noc)
        tv = np.abs(R - value).astype(np.float64).ravel()
        tc = np.abs(R - Cf).astype(np.float64).ravel()
        stats[2], stats[3] = math.fsum(tv), math.fsum(tc)
    return (dst, used, stats, tv, tc) if terms else (dst, used, stats)


def filter_batch(frames, center, neighbors, flows, masks=None, tau=30.0, gains=None, ref=None):
    """n output images: center (n,), neighbors (n, K), flows (n, K, h, w, 2), masks (n, K, h, w) -> dst, used (n, h, w), stats (n, 4)"""
    outs = [filter_one(frames, center[i], neighbors[i], flows[i], None if masks is None else masks[i], tau, gains,
                       None if ref is None else ref[i]) for i in range(len(center))]
    return np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs]), np.stack([o[2] for o in outs])


def psnr(a, clean):
    """of an 8-bit valued image against the clean one, in dB"""
    mse = np.mean((np.asarray(a, np.float64) - np.asarray(clean, np.float64)) ** 2)
    return 10.0 * math.log10(255.0 ** 2 / mse)


# ---- the quality case (tests/test_temporal.py on the restatement, tests/test_gpu_temporal.py through OFClass.temporal_filter) -----
QUALITY_CROP = (slice(100, 356), slice(300, 812))
QUALITY_SIGMA, QUALITY_SEED, QUALITY_TAU = 10.0, 7, 30.0


def quality_frames(first=1):
    """(clean, noisy): (3, 256, 512) float32, the crop of the golden alley_1 frames first .. first + 2 (1 or 20) and the same with
    Gaussian noise sigma 10 of default_rng(7), clipped to [0, 255]"""
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    z = {}
    for name in ("alley_1_gray.npz", "alley_1_more.npz"):
        with np.load(os.path.join(golden, name)) as f:
            z.update({k: f[k] for k in f.files if k.startswith("frame_")})
    clean = np.stack([np.asarray(z["frame_%04d" % (first + k)], np.float64)[QUALITY_CROP] for k in range(3)])
    rng = np.random.default_rng(QUALITY_SEED)
    noisy = np.clip(clean + rng.normal(0.0, QUALITY_SIGMA, clean.shape), 0.0, 255.0)
    return clean.astype(f32), noisy.astype(f32)
