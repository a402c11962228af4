"""numpy float32 restatement of the background subtraction (csrc/subtract.hip.h, include/fotg.h fotg_subtract): every f32 operation
separately rounded, in the kernel's order, so the GPU's code, diff, evidence and stats equal these byte for byte.  The taps are
plate_ref.taps (those of warp_ref.warp) on the plate's canvas, the coefficients of the motion source come from motion_ref.coef
(through plate_ref.motion_vectors on the frame grid).  Everything after Dq is integer.  Also the numpy twin of
flowonthego_amd.subtract.frame_motions."""
import numpy as np

import motion_ref as M
import plate_ref as PR
import warp_ref as WR  # noqa: F401  (the taps' definition)

f32 = np.float32
MAX_Q = 32767


def thresholds(low, high):
    """L = lrintf(16 low), Hh = lrintf(16 high)"""
    L, Hh = int(np.rint(f32(16) * f32(low))), int(np.rint(f32(16) * f32(high)))
    assert 0 <= L <= Hh <= MAX_Q
    return L, Hh


def words(frame, plate, F, ox, oy, pcode=None, mask=None):
    """one frame (h, w, c) f32 against one plate (H, W, c) f32 along the vectors F (h, w, 2): (Dq (h, w) int64, 0 where
    inadmissible; own (h, w) uint8: 0 admissible, 2 or 3 the code of an inadmissible pixel)"""
    h, w = frame.shape[:2]
    u, v = F[..., 0], F[..., 1]
    xg = np.broadcast_to((np.arange(w, dtype=np.int64) + ox).astype(f32)[None, :], (h, w))
    yg = np.broadcast_to((np.arange(h, dtype=np.int64) + oy).astype(f32)[:, None], (h, w))
    with np.errstate(all="ignore"):
        fin = np.isfinite(u) & np.isfinite(v)
        Xc, Yc = xg + np.where(fin, u, f32(0)), yg + np.where(fin, v, f32(0))
        s, inside, (x1, x2, y1, y2) = PR.taps(plate, Xc, Yc)
        unknown = ~fin
        if mask is not None:
            unknown = unknown | (mask != 0)
        noplate = ~inside
        if pcode is not None:
            noplate = noplate | ((pcode[y1, x1] | pcode[y1, x2] | pcode[y2, x1] | pcode[y2, x2]) != 0)
        nan = np.isnan(s).any(-1) | np.isnan(frame).any(-1)
        d = np.zeros((h, w), f32)
        for ch in range(frame.shape[2]):
            e = np.abs(frame[..., ch] - s[..., ch])
            d = np.where(e > d, e, d)
        assert d.dtype == f32
        dq = (np.minimum(np.nan_to_num(d, nan=0.0) * f32(16), f32(32767)) + f32(0.5)).astype(np.int64)
    own = np.where(unknown, 3, np.where(noplate, 2, np.where(nan, 3, 0))).astype(np.uint8)
    return np.where(own == 0, dq, 0), own


def box(a, r):
    """the sum over the (2r+1)^2 window, pixels outside the array adding nothing"""
    h, w = a.shape
    p = np.zeros((h + 2 * r, w + 2 * r), np.int64)
    p[r:r + h, r:r + w] = a
    out = np.zeros((h, w), np.int64)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            out += p[dy:dy + h, dx:dx + w]
    return out


def classify(dq, own, L, Hh, r):
    """the code map of one frame from its Dq and admissibility"""
    adm = own == 0
    S, C = box(dq, r), box(adm.astype(np.int64), r)
    code = np.where(S >= Hh * C, 4, np.where(S >= L * C, 1, 0))
    return np.where(adm, code, own).astype(np.uint8)


def subtract(frames, plate, index=None, ox=0, oy=0, flows=None, params=None, plate_code=None, mask=None, low=8.0, high=24.0, window=1):
    """frames (n, h, w[, c]) f32 or uint8; plate (P, H, W[, c]) of their type; index n plate indices or None (plate 0 for P == 1,
    plate i otherwise); flows (n, h, w, 2) f32 or params (n, 6) f64; plate_code (P, H, W) uint8 or None; mask (n, h, w) uint8 or
    None.  Returns code (n, h, w) uint8, diff (n, h, w) int16, evidence (n, h, w, 2) f32, stats (n, 7) int64."""
    frames, plate = np.asarray(frames), np.asarray(plate)
    n, h, w = frames.shape[:3]
    P, H, W = plate.shape[:3]
    Fr = frames.astype(f32).reshape(n, h, w, -1)
    Pl = plate.astype(f32).reshape(P, H, W, -1)
    L, Hh = thresholds(low, high)
    if index is None:
        assert P in (1, n)
        index = [0] * n if P == 1 else list(range(n))
    code = np.zeros((n, h, w), np.uint8)
    diff = np.zeros((n, h, w), np.int16)
    evidence = np.zeros((n, h, w, 2), f32)
    stats = np.zeros((n, 7), np.int64)
    for i in range(n):
        b = int(index[i])
        F = np.asarray(flows[i], f32) if flows is not None else PR.motion_vectors(params[i], w, h, w, h, 0, 0)
        dq, own = words(Fr[i], Pl[b], F, ox, oy, None if plate_code is None else plate_code[b], None if mask is None else mask[i])
        cd = classify(dq, own, L, Hh, window)
        code[i], diff[i] = cd, dq
        evidence[i, ..., 0] = (cd == 4).astype(f32)
        evidence[i, ..., 1] = dq.astype(f32) * f32(0.0625)
        stats[i, :5] = np.bincount(cd.ravel(), minlength=5)[:5]
        stats[i, 5] = dq.sum()
        stats[i, 6] = dq[(cd == 1) | (cd == 4)].sum()
    return code, diff, evidence, stats


def frame_motions(motions):
    """(n, 6) f64, the maps reference -> frame -> the maps frame -> reference (flowonthego_amd.subtract.frame_motions)"""
    m = np.asarray(motions, np.float64)
    i = M._inverse((m[:, 0] + 1.0, m[:, 1], m[:, 2], m[:, 3], m[:, 4] + 1.0, m[:, 5]))
    return np.stack((i[0] - 1.0, i[1], i[2], i[3], i[4] - 1.0, i[5]), axis=1)
