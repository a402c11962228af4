"""numpy float32 restatement of the frame warp (csrc/warp.hip.h, include/fotg.h fotg_warp): every operation separately rounded to
f32, in the kernel's order, so the GPU's dst and code equal these byte for byte.  In reference mode (fill_mode 0, no occ, finite
flow) dst and code == 0 are the dst and mask of the reference's image_warp (kroeger/FDF1.0.1/opticalflow_aux.c:18-60).
Codes: 0 valid, 1 occluded (from occ), 2 the vector leaves the frame, 3 unknown (non-finite vector, or from occ)."""
import math

import numpy as np

f32 = np.float32


def to_u8(v):
    """the 8-bit destination: rintf, clamped to [0, 255]; a NaN becomes 0"""
    with np.errstate(all="ignore"):
        r = np.rint(np.asarray(v, f32))
        return np.where(r > 0, np.minimum(r, f32(255)), f32(0)).astype(np.uint8)


def warp(src, flow, ref=None, occ=None, fill_mode=0, fill=0.0, terms=False):
    """src: (h, w) or (h, w, c) float32 or uint8; flow: (h, w, 2) float32; ref: like src or None; occ: (h, w) uint8 or None.
    Returns dst (src's shape and dtype), code (h, w) uint8, stats (6,) float64 [sums added with math.fsum] and, with terms=True,
    the two lists of residual terms (float64 arrays, each term an f32 widened exactly) the sums are made of."""
    src = np.asarray(src)
    u8 = src.dtype == np.uint8
    S = src.astype(f32).reshape(src.shape[0], src.shape[1], -1)
    h, w, noc = S.shape
    F = np.asarray(flow, f32)
    u, v = F[..., 0], F[..., 1]
    one, fillf = f32(1), f32(fill)
    ys, xs = np.mgrid[0:h, 0:w]
    with np.errstate(all="ignore"):
        known = np.isfinite(u) & np.isfinite(v)
        uz, vz = np.where(known, u, f32(0)), np.where(known, v, f32(0))
        xx, yy = xs.astype(f32) + uz, ys.astype(f32) + vz
        fx, fy = np.floor(xx), np.floor(yy)
        dx, dy = xx - fx, yy - fy
        inside = (xx >= f32(0)) & (xx <= f32(w - 1)) & (yy >= f32(0)) & (yy <= f32(h - 1))
        xi = np.clip(fx, f32(-2), f32(w)).astype(np.int64)
        yi = np.clip(fy, f32(-2), f32(h)).astype(np.int64)
        x1, x2 = np.clip(xi, 0, w - 1), np.clip(xi + 1, 0, w - 1)
        y1, y2 = np.clip(yi, 0, h - 1), np.clip(yi + 1, 0, h - 1)
        dx_, dy_ = dx[..., None], dy[..., None]
        value = (S[y1, x1] * (one - dx_) * (one - dy_) + S[y1, x2] * dx_ * (one - dy_) +
                 S[y2, x1] * (one - dx_) * dy_ + S[y2, x2] * dx_ * dy_)
    assert value.dtype == f32
    own = np.where(known, np.where(inside, 0, 2), 3).astype(np.uint8)
    code = own.copy()
    if occ is not None:
        code = np.where(own == 0, np.minimum(np.asarray(occ, np.uint8), 3), own).astype(np.uint8)
    keep = (own != 3) if fill_mode == 0 else (code == 0)
    out = np.where(keep[..., None], value, fillf).astype(f32)
    dst = (to_u8(out) if u8 else out).reshape(src.shape)
    stats = np.zeros(6, np.float64)
    stats[:4] = np.bincount(code.ravel(), minlength=4)[:4]
    tw = tu = np.zeros(0, np.float64)
    if ref is not None:
        R = np.asarray(ref).astype(f32).reshape(h, w, noc)
        ok = code == 0
        tw = np.abs(R[ok] - value[ok]).astype(np.float64).ravel()
        tu = np.abs(R[ok] - S[ok]).astype(np.float64).ravel()
        stats[4], stats[5] = math.fsum(tw), math.fsum(tu)
    return (dst, code, stats, tw, tu) if terms else (dst, code, stats)


def warp_batch(src, flow, ref=None, occ=None, fill_mode=0, fill=0.0):
    """a batch: src (n, h, w[, c]), flow (n, h, w, 2) -> dst, code (n, h, w), stats (n, 6)"""
    outs = [warp(src[k], flow[k], None if ref is None else ref[k], None if occ is None else occ[k], fill_mode, fill)
            for k in range(len(src))]
    return np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs]), np.stack([o[2] for o in outs])


# ---- the flows of the reference comparison (tests/test_warp.py, tests/golden/make_warp_golden.py, tests/test_gpu_warp.py) ------
SIZES = ((64, 96), (37, 53), (5, 3))          # (h, w)
KINDS = ("smooth", "random", "integer", "border", "huge")


def case_image(h, w, noc, seed):
    """an 8-bit valued f32 image (h, w) or (h, w, 3)"""
    rng = np.random.default_rng(1000 + seed)
    return rng.integers(0, 256, (h, w) if noc == 1 else (h, w, noc)).astype(f32)


def case_flow(kind, h, w, seed):
    rng = np.random.default_rng(2000 + seed)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    if kind == "smooth":
        fl = np.stack([3.0 * np.sin(ys / 7.0) + 1.5 * np.cos(xs / 5.0), 2.0 * np.cos(ys / 6.0 + xs / 9.0)], -1)
    elif kind == "random":                      # up to +- 2 w: most pixels leave the frame
        fl = rng.uniform(-2.0 * w, 2.0 * w, (h, w, 2))
    elif kind == "integer":
        fl = rng.integers(-4, 5, (h, w, 2)).astype(np.float64)
    elif kind == "border":                      # targets exactly on the last / first column and row, and -0.0
        fl = rng.uniform(-1.0, 1.0, (h, w, 2))
        fl[::3, :, 0] = (w - 1) - xs[::3]
        fl[1::3, :, 0] = -xs[1::3]
        fl[:, ::4, 1] = (h - 1) - ys[:, ::4]
        fl[:, 1::4, 1] = -ys[:, 1::4]
        fl[0, 0] = (-0.0, -0.0)
        fl[h - 1, w - 1] = (-0.0, 0.0)
    elif kind == "huge":                        # +- 1e9: the reference's int conversion is still defined
        fl = rng.choice([1e9, -1e9, 0.25, -3.5], (h, w, 2))
    else:
        raise ValueError(kind)
    return fl.astype(f32)


def cases():
    """(name, noc, h, w, kind, seed) of every reference comparison"""
    out = []
    for noc in (1, 3):
        for si, (h, w) in enumerate(SIZES):
            for ki, kind in enumerate(KINDS):
                out.append(("%s_%dx%d_%s" % ("gray" if noc == 1 else "rgb", h, w, kind), noc, h, w, kind, 100 * noc + 10 * si + ki))
    return out
