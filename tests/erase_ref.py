"""numpy restatement of the object removal (csrc/erase.hip.h, include/fotg.h fotg_erase), written from the definition: the distance by
brute force over the (2R + 1)^2 window, the weight in integers, the sample with subtract_ref's rules (plate_ref.taps, those of
warp_ref.warp) less the test of the frame pixel, the blend in f32 with every operation rounded on its own -- so the GPU's dst, code,
alpha and stats equal these byte for byte.  Also the numpy disc dilation flowonthego_amd.erase.grow_mask is compared with."""
import math

import numpy as np

import plate_ref as PR
import warp_ref as WR  # noqa: F401  (the taps' definition)

f32 = np.float32
MAX_GROW = MAX_FEATHER = 8
FAR = 1 << 30


def distance2(remove, R):
    """(h, w) int64: the smallest dx^2 + dy^2 to a pixel of the frame with remove != 0 within |dx|, |dy| <= R; FAR without one"""
    h, w = remove.shape
    p = np.zeros((h + 2 * R, w + 2 * R), bool)
    p[R:R + h, R:R + w] = remove != 0
    d2 = np.full((h, w), FAR, np.int64)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            hit = p[R + dy:R + dy + h, R + dx:R + dx + w]
            d2 = np.where(hit, np.minimum(d2, dx * dx + dy * dy), d2)
    return d2


def alpha_table(G, F):
    """alpha for D2 = 0 .. 2 R^2 (every value the window can give), by the definition's integer formula"""
    assert 0 <= G <= MAX_GROW and 0 <= F <= MAX_FEATHER
    R = G + F
    out = np.zeros(2 * R * R + 1, np.int64)
    for D2 in range(len(out)):
        if D2 <= G * G:
            out[D2] = 256
        elif F == 0:
            out[D2] = 0
        else:
            E = 16 * (G + F) - math.isqrt(256 * D2)
            out[D2] = 0 if E <= 0 else min(256, (256 * E + 8 * F) // (16 * F))
    return out


def weights(remove, G, F):
    """(h, w) int64 alpha of one frame"""
    d2 = distance2(remove, G + F)
    tab = alpha_table(G, F)
    return np.where(d2 == FAR, 0, tab[np.minimum(d2, len(tab) - 1)])


def sample(plate, F, w, h, ox, oy, pcode=None, mask=None):
    """one plate (H, W, c) f32 along the vectors F (h, w, 2): (s (h, w, c) f32, code (h, w) uint8: 1 a good sample, 2 or 3 the
    code of a pixel without one) -- steps 1 to 4 of subtract_ref.words without the test of the frame pixel"""
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
        nan = np.isnan(s).any(-1)
    return s, np.where(unknown, 3, np.where(noplate, 2, np.where(nan, 3, 1))).astype(np.uint8)


def to_u8(v):
    """warp_to_u8: rintf, clamped to [0, 255]; a NaN becomes 0"""
    with np.errstate(all="ignore"):
        r = np.rint(v)
        return np.where(r > 0, np.minimum(r, f32(255)), f32(0)).astype(np.uint8)


def erase(frames, plate, remove, index=None, ox=0, oy=0, flows=None, params=None, plate_code=None, mask=None, grow=2, feather=3):
    """frames (n, h, w[, c]) f32 or uint8; plate (P, H, W[, c]) of their type; remove (n, h, w) uint8; index n plate indices or None
    (plate 0 for P == 1, plate i otherwise); flows (n, h, w, 2) f32 or params (n, 6) f64; plate_code (P, H, W) uint8 or None; mask
    (n, h, w) uint8 or None.  Returns dst (the frames' shape and type), code (n, h, w) uint8, alpha (n, h, w) int16, stats (n, 8)
    int64."""
    frames, plate = np.asarray(frames), np.asarray(plate)
    n, h, w = frames.shape[:3]
    P, H, W = plate.shape[:3]
    u8 = frames.dtype == np.uint8
    Fr = frames.astype(f32).reshape(n, h, w, -1)
    Pl = plate.astype(f32).reshape(P, H, W, -1)
    if index is None:
        assert P in (1, n)
        index = [0] * n if P == 1 else list(range(n))
    dst = frames.copy().reshape(n, h, w, -1)
    code = np.zeros((n, h, w), np.uint8)
    alpha = np.zeros((n, h, w), np.int16)
    stats = np.zeros((n, 8), np.int64)
    for i in range(n):
        b = int(index[i])
        al = weights(remove[i], grow, feather)
        F = np.asarray(flows[i], f32) if flows is not None else PR.motion_vectors(params[i], w, h, w, h, 0, 0)
        s, own = sample(Pl[b], F, w, h, ox, oy, None if plate_code is None else plate_code[b], None if mask is None else mask[i])
        cd = np.where(al == 0, 0, np.where(own != 1, own, np.where(al == 256, 1, 4))).astype(np.uint8)
        a = (al.astype(f32) * f32(0.00390625))[..., None]
        with np.errstate(all="ignore"):
            diff = s - Fr[i]
            assert diff.dtype == f32
            step = diff * a
            blend = Fr[i] + step
            assert blend.dtype == f32
        val = np.where((cd == 1)[..., None], s, blend)
        touched = (cd == 1) | (cd == 4)
        out = to_u8(val) if u8 else val
        dst[i] = np.where(touched[..., None], out, dst[i])
        code[i], alpha[i] = cd, al
        stats[i, :5] = np.bincount(cd.ravel(), minlength=5)[:5]
        stats[i, 5] = ((al == 256) & ((cd == 2) | (cd == 3))).sum()
        stats[i, 6] = (remove[i] != 0).sum()
        stats[i, 7] = al.sum()
    return dst.reshape(frames.shape), code, alpha, stats


def disc_dilation(remove, G):
    """(..., h, w) uint8: 1 where a set pixel of the same frame lies within the disc dx^2 + dy^2 <= G^2"""
    remove = np.asarray(remove)
    flat = remove.reshape((-1,) + remove.shape[-2:])
    out = np.zeros(flat.shape, np.uint8)
    h, w = flat.shape[1:]
    for k in range(flat.shape[0]):
        p = np.zeros((h + 2 * G, w + 2 * G), bool)
        p[G:G + h, G:G + w] = flat[k] != 0
        for dy in range(-G, G + 1):
            for dx in range(-G, G + 1):
                if dx * dx + dy * dy <= G * G:
                    out[k] |= p[G + dy:G + dy + h, G + dx:G + dx + w].astype(np.uint8)
    return out.reshape(remove.shape)
