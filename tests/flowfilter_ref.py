"""numpy float32 restatement of the edge- and occlusion-aware flow filter (csrc/flowfilter.hip.h, include/fotg.h fotg_flow_filter):
every operation separately rounded to f32, the window walked dy ascending and inside it dx ascending, so the GPU's out and code
equal these byte for byte (a NaN apart: the default NaN of the GPU and of the host differ in sign).  Positions outside the image
are padded as invalid, which is "skipped"."""
import math

import numpy as np

f32 = np.float32


def spatial_table(radius, sigma):
    """s[i] = exp(-i^2 / (2 sigma^2)), i = 0 .. radius, evaluated in f64 and rounded to f32 (flowonthego_amd.flowfilter's table)"""
    return np.array([math.exp(-(i * i) / (2.0 * float(sigma) * float(sigma))) for i in range(radius + 1)], np.float64).astype(f32)


def scale_of(tau, channels):
    """1.0f / (tau * (float)channels) in f32"""
    return f32(1) / (f32(tau) * f32(channels))


def one_pass(flow, guide, invalid, radius, s, scale):
    """flow (h, w, 2) f32, guide (h, w, ch) f32, invalid (h, w) bool (the mask's part of validity) -> out (h, w, 2), code (h, w)"""
    h, w = flow.shape[:2]
    R = radius
    valid = np.isfinite(flow[..., 0]) & np.isfinite(flow[..., 1]) & ~invalid
    pad2 = ((R, R), (R, R))
    Fu, Fv = np.pad(flow[..., 0], pad2), np.pad(flow[..., 1], pad2)
    V = np.pad(valid, pad2)                                # False outside the image
    G = np.pad(guide, pad2 + ((0, 0),))
    nu, nv, den = (np.zeros((h, w), f32) for _ in range(3))
    with np.errstate(all="ignore"):
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                win = (slice(R + dy, R + dy + h), slice(R + dx, R + dx + w))
                d = np.abs(guide[..., 0] - G[win][..., 0])
                for ch in range(1, guide.shape[2]):
                    d = d + np.abs(guide[..., ch] - G[win][..., ch])
                wt = f32(s[abs(dy)] * s[abs(dx)]) * (f32(1) - d * scale)
                assert wt.dtype == f32
                use = V[win] & (wt > 0)
                nu = np.where(use, nu + wt * Fu[win], nu)
                nv = np.where(use, nv + wt * Fv[win], nv)
                den = np.where(use, den + wt, den)
        has = den > 0
        out = np.stack([np.where(has, nu / den, flow[..., 0]), np.where(has, nv / den, flow[..., 1])], -1)
    assert out.dtype == f32 and den.dtype == f32
    # the passed-through vectors bit for bit (np.where may quieten nothing, but be explicit)
    out.view(np.uint32)[~has] = np.ascontiguousarray(flow).view(np.uint32)[~has]
    code = np.where(has, np.where(valid, 0, 1), 3).astype(np.uint8)
    return out, code


def filter_one(flow, guide, mask=None, radius=3, spatial=None, tau=20.0, iters=1, terms=False):
    """flow (h, w, 2) f32; guide (h, w) or (h, w, ch) f32 or uint8; mask None or (h, w) uint8; spatial None (all ones) or radius + 1
    f32.  Returns out (h, w, 2) f32, code (h, w) uint8, stats (4,) float64 [the change sum added with math.fsum] and, with
    terms=True, the change terms (a float64 array, each an f32 widened exactly, the non-finite ones left out)."""
    flow = np.ascontiguousarray(flow, f32)
    h, w = flow.shape[:2]
    G = np.asarray(guide).astype(f32).reshape(h, w, -1)
    s = np.ones(radius + 1, f32) if spatial is None else np.asarray(spatial, f32)
    assert s.shape == (radius + 1,)
    scale = scale_of(tau, G.shape[2])
    invalid = np.zeros((h, w), bool) if mask is None else np.asarray(mask) != 0
    cur, first = flow, None
    for k in range(iters):
        cur, code = one_pass(cur, G, invalid, radius, s, scale)
        first = code if first is None else first
        invalid = code == 3
    final = np.where(code == 3, 3, np.where(first == 0, 0, 1)).astype(np.uint8)
    with np.errstate(all="ignore"):
        t = np.abs(cur - flow)[final == 0].astype(np.float64).ravel()
    t = t[np.isfinite(t)]
    stats = np.array([(final == 0).sum(), (final == 1).sum(), (final == 3).sum(), math.fsum(t)], np.float64)
    return (cur, final, stats, t) if terms else (cur, final, stats)


def filter_batch(flow, guide, mask=None, **kw):
    outs = [filter_one(flow[i], guide[i], None if mask is None else mask[i], **kw) for i in range(len(flow))]
    return np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs]), np.stack([o[2] for o in outs])


def same_but_nan(a, b):
    """a and b (f32) have NaNs at the same positions and the same bits everywhere else"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != f32 or b.dtype != f32:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


# ---- the quality case (tests/test_flowfilter.py on the restatement, tests/test_gpu_flowfilter.py on the GPU) -----------------------
QUALITY = dict(radius=5, sigma=3.0, tau=20.0, iters=2)
QUALITY_SEED = 11


def quality_scene():
    """96 x 128: a textured rectangle moving (6, -3) over a textured background moving (-1, 0.5).  Returns (true flow, degraded
    flow, guide (h, w) f32, mask uint8, regions dict of bool maps "all", "belt", "band").  The degraded flow is the true one blurred
    by a 7 x 7 box, plus noise of 0.1 px, plus a band of 7 pixels of occluded garbage (20, 20) right of the rectangle, marked 1 in
    the mask."""
    h, w = 96, 128
    rng = np.random.default_rng(QUALITY_SEED)
    inside = np.zeros((h, w), bool)
    inside[28:68, 40:88] = True
    true = np.where(inside[..., None], np.array([6.0, -3.0]), np.array([-1.0, 0.5]))
    ys, xs = np.mgrid[0:h, 0:w]
    guide = np.where(inside, 190.0 + 12.0 * np.sin(xs / 3.0) * np.cos(ys / 4.0), 70.0 + 12.0 * np.cos(xs / 5.0 + ys / 7.0))
    guide = np.clip(guide + rng.normal(0, 2.0, (h, w)), 0, 255)
    p = np.pad(true, ((3, 3), (3, 3), (0, 0)), mode="edge")
    blur = sum(p[dy:dy + h, dx:dx + w] for dy in range(7) for dx in range(7)) / 49.0
    bad = blur + rng.normal(0, 0.1, blur.shape)
    band = np.zeros((h, w), bool)
    band[28:68, 88:95] = True
    bad[band] = (20.0, 20.0)
    mask = band.astype(np.uint8)
    grown, shrunk = np.zeros_like(inside), np.ones_like(inside)
    for dy in range(-4, 5):
        for dx in range(-4, 5):
            sh = np.pad(inside, 4)[4 + dy:4 + dy + h, 4 + dx:4 + dx + w]
            grown |= sh
            shrunk &= sh
    belt = grown & ~shrunk & ~band                         # within 4 pixels of the boundary on either side: 8 wide
    return true.astype(f32), bad.astype(f32), guide.astype(f32), mask, dict(all=np.ones((h, w), bool), belt=belt, band=band)


def epe(flow, true, region):
    d = np.asarray(flow, np.float64) - np.asarray(true, np.float64)
    return float(np.sqrt((d ** 2).sum(-1))[region].mean())
