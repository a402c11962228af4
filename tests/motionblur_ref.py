"""The motion blur along a flow restated in numpy, in the order include/fotg.h and flowonthego_amd/csrc/motionblur.hip.h define it:
one f32 multiply per component, exact integers (int64) after it, and for f32 frames the f32 sums in the defined order, so the GPU is
compared byte for byte.  Vectorised over the pixels; the only loop is the one over the taps k = -32 .. 32."""
import numpy as np

from histograms_ref import mag

f32 = np.float32
TILE, MAX_BLUR, COPY_BELOW = 32, 32, 8
C0, C1, C2, C3, TAPS, COPY_TILES, MAX_LEN = range(7)


def shutter256(shutter):
    return int(round(256 * shutter))


def half_vectors(flow, mask=None, s256=128, max_blur=32):
    """step 1: (H int64 (..., 2), unknown bool (...)) of flow (..., 2) f32"""
    flow = np.asarray(flow, f32)
    u, v = flow[..., 0], flow[..., 1]
    with np.errstate(invalid="ignore"):
        known = (np.abs(u) <= f32(4096)) & (np.abs(v) <= f32(4096))          # false for a NaN or an infinity
    if mask is not None:
        known &= np.asarray(mask) == 0
    s = f32(s256) / f32(32)
    with np.errstate(invalid="ignore", over="ignore"):
        hx = np.rint(np.where(known, u, f32(0)) * s).astype(np.int64)           # rintf: ties to even
        hy = np.rint(np.where(known, v, f32(0)) * s).astype(np.int64)
    length, cap16 = mag(hx, hy), 16 * max_blur
    over = length > cap16
    div = np.maximum(length, 1)
    hx = np.where(over, np.sign(hx) * (np.abs(hx) * cap16 // div), hx)          # C division: towards zero
    hy = np.where(over, np.sign(hy) * (np.abs(hy) * cap16 // div), hy)
    return np.stack([hx, hy], -1), ~known


def tile_max(H):
    """step 2, first half: tilemax (n, th, tw, 2) of H (n, h, w, 2)"""
    n, h, w = H.shape[:3]
    th, tw = -(-h // TILE), -(-w // TILE)
    Hp = np.zeros((n, th * TILE, tw * TILE, 2), np.int64)
    Hp[:, :h, :w] = H
    sq = np.full((n, th * TILE, tw * TILE), -1, np.int64)                        # outside the frame: never the largest
    sq[:, :h, :w] = H[..., 0] ** 2 + H[..., 1] ** 2
    tiles = lambda a: a.reshape((n, th, TILE, tw, TILE) + a.shape[3:]).swapaxes(2, 3).reshape((n, th, tw, TILE * TILE) + a.shape[3:])
    first = tiles(sq).argmax(3)                                                  # argmax: the first (lowest linear index) of the largest
    return np.take_along_axis(tiles(Hp), first[..., None, None], 3)[:, :, :, 0]


def neighbour_max(tm):
    """step 2, second half: D (n, th, tw, 2): the largest of the up to nine around, the first in raster order on a tie"""
    n, th, tw = tm.shape[:3]
    D = np.zeros_like(tm)
    best = np.full((n, th, tw), -1, np.int64)
    pad = np.zeros((n, th + 2, tw + 2, 2), np.int64)
    pad[:, 1:-1, 1:-1] = tm
    ok = np.zeros((th + 2, tw + 2), bool)
    ok[1:-1, 1:-1] = True
    for dy in range(3):
        for dx in range(3):
            c = pad[:, dy:dy + th, dx:dx + tw]
            sq = np.where(ok[dy:dy + th, dx:dx + tw][None], c[..., 0] ** 2 + c[..., 1] ** 2, -1)
            take = sq > best
            best = np.where(take, sq, best)
            D = np.where(take[..., None], c, D)
    return D


def _per_pixel(a, h, w):
    return np.repeat(np.repeat(a, TILE, 1), TILE, 2)[:, :h, :w]


def blur(frame, flow, mask=None, s256=128, max_blur=32):
    """frame (n, h, w[, c]) uint8 or f32, flow (n, h, w, 2) -> dst, code (n, h, w) uint8, vectors (n, h, w, 2) int16, stats (n, 8) int64"""
    frame = np.asarray(frame)
    n, h, w = flow.shape[:3]
    img = frame.reshape(n, h, w, -1)
    H, unknown = half_vectors(flow, mask, s256, max_blur)
    tm = tile_max(H)
    Dt = neighbour_max(tm)
    lenDt = mag(Dt[..., 0], Dt[..., 1])
    Dx, Dy, lenD = _per_pixel(Dt[..., 0], h, w), _per_pixel(Dt[..., 1], h, w), _per_pixel(lenDt, h, w)
    copy = lenD < COPY_BELOW
    L = (lenD + 15) // 16
    Ls, lenDs = np.maximum(L, 1), np.maximum(lenD, 1)
    ys, xs = np.mgrid[0:h, 0:w]
    ys, xs, ni = ys[None], xs[None], np.arange(n)[:, None, None]

    def reach(P):
        return np.abs(P[..., 0] * Dx + P[..., 1] * Dy) // lenDs

    rX = reach(H)
    is_f = img.dtype == np.float32
    acc = np.zeros(img.shape, f32 if is_f else np.int64)
    W = np.zeros((n, h, w), np.int64)
    taps = np.zeros((n, h, w), np.int64)
    any_off = np.zeros((n, h, w), bool)
    any_clamped = np.zeros((n, h, w), bool)
    for k in range(-MAX_BLUR, MAX_BLUR + 1):
        a = abs(k)
        active = ~copy & (a <= L)
        if not active.any():
            continue
        sk = 1 if k >= 0 else -1
        ox = sk * np.sign(Dx) * ((2 * np.abs(Dx) * a + Ls) // (2 * Ls))
        oy = sk * np.sign(Dy) * ((2 * np.abs(Dy) * a + Ls) // (2 * Ls))
        px, py = xs + ((ox + 8) >> 4), ys + ((oy + 8) >> 4)
        cx, cy = np.clip(px, 0, w - 1), np.clip(py, 0, h - 1)
        clamped = (cx != px) | (cy != py)
        d = lenD * a // Ls
        wk = np.clip(np.maximum(reach(H[ni, cy, cx]), rX) + 16 - d, 0, 16)
        wk = np.where(active, wk, 0)
        on = wk > 0
        c = img[ni, cy, cx]
        if is_f:
            with np.errstate(invalid="ignore", over="ignore"):
                acc = np.where(active[..., None], acc + wk.astype(f32)[..., None] * c, acc)      # f32 product, f32 sum
        else:
            acc += wk[..., None] * c.astype(np.int64)
        W += wk
        taps += on
        any_off |= on & (k != 0)
        any_clamped |= on & clamped
    Ws = np.maximum(W, 1)
    if is_f:
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            out = acc / Ws.astype(f32)[..., None]
        assert out.dtype == np.float32
    else:
        out = ((2 * acc + Ws[..., None]) // (2 * Ws[..., None])).astype(np.uint8)
    dst = np.where(copy[..., None], img, out).reshape(frame.shape)
    code = np.where(unknown, 3, np.where(copy, 0, np.where(any_clamped, 2, np.where(any_off, 1, 0)))).astype(np.uint8)
    length = mag(H[..., 0], H[..., 1])
    stats = np.zeros((n, 8), np.int64)
    for c_ in range(4):
        stats[:, c_] = (code == c_).sum((1, 2))
    stats[:, TAPS] = taps.sum((1, 2))
    stats[:, COPY_TILES] = (lenDt < COPY_BELOW).sum((1, 2))
    stats[:, MAX_LEN] = length.reshape(n, -1).max(1)
    return dst, code, H.astype(np.int16), stats


def tile_view(H):
    """(tilemax, D, lenD, L) per tile, for the tests that look at the branches"""
    tm = tile_max(H)
    D = neighbour_max(tm)
    lenD = mag(D[..., 0], D[..., 1])
    return tm, D, lenD, np.where(lenD < COPY_BELOW, 0, (lenD + 15) // 16)
