"""numpy float32 restatement of the background plate (csrc/plate.hip.h, include/fotg.h fotg_plate): every operation separately
rounded to f32, in the kernel's order, so the GPU's dst, count and code equal these byte for byte.  The taps are those of
warp_ref.warp, here at the positions of a canvas that need not be the frame grid; the coefficients of the motion source come from
motion_ref.coef.  The statistics are added in the kernel's order too (per lane, the wave's xor butterfly, warp_fold_kernel), in
float64, so their bits are the GPU's as well.  Also the numpy twins of flowonthego_amd.plate.plate_motions / mosaic_canvas."""
import math

import numpy as np

import motion_ref as M
import warp_ref as WR

f32 = np.float32


def taps(S, xx, yy):
    """warp_ref.warp's value of S (h, w, c) f32 at the positions (xx, yy) (f32 arrays of one shape) -> (value (..., c), inside,
    (x1, x2, y1, y2))"""
    h, w = S.shape[:2]
    one = f32(1)
    with np.errstate(all="ignore"):
        fx, fy = np.floor(xx), np.floor(yy)
        dx, dy = xx - fx, yy - fy
        inside = (xx >= f32(0)) & (xx <= f32(w - 1)) & (yy >= f32(0)) & (yy <= f32(h - 1))
        xi = np.clip(np.nan_to_num(fx, nan=0.0), f32(-2), f32(w)).astype(np.int64)
        yi = np.clip(np.nan_to_num(fy, nan=0.0), f32(-2), f32(h)).astype(np.int64)
        x1, x2 = np.clip(xi, 0, w - 1), np.clip(xi + 1, 0, w - 1)
        y1, y2 = np.clip(yi, 0, h - 1), np.clip(yi + 1, 0, h - 1)
        dx_, dy_ = dx[..., None], dy[..., None]
        value = (S[y1, x1] * (one - dx_) * (one - dy_) + S[y1, x2] * dx_ * (one - dy_) +
                 S[y2, x1] * (one - dx_) * dy_ + S[y2, x2] * dx_ * dy_)
    assert value.dtype == f32
    return value, inside, (x1, x2, y1, y2)


def motion_vectors(P, w, h, W, H, ox, oy):
    """(H, W, 2) f32: the motion source's vector at every canvas pixel"""
    x = np.arange(W, dtype=np.int64) - ox
    y = np.arange(H, dtype=np.int64) - oy
    Xf = np.broadcast_to((2 * x - (w - 1)).astype(f32)[None, :], (H, W))
    Yf = np.broadcast_to((2 * y - (h - 1)).astype(f32)[:, None], (H, W))
    k = M.coef(P, w, h)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.stack([(k[0] * Xf + k[1] * Yf) + k[2], (k[3] * Xf + k[4] * Yf) + k[5]], -1)


def _butterfly(a):
    """the wave's xor shuffles 32 .. 1 over the last axis (64 lanes): lane 0's sum"""
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        a = a + a[..., lane ^ o]
    return a[..., 0]


def fold(part):
    """warp_fold_kernel: the partials (blocks,) f64 of one plate -> their sum in the kernel's order"""
    blocks = len(part)
    pad = np.zeros(-(-blocks // 256) * 256 if blocks else 256)
    pad[:blocks] = part
    acc = np.zeros(256)
    for row in pad.reshape(-1, 256):                      # thread t adds t, t + 256, ...
        acc = acc + row
    waves = _butterfly(acc.reshape(4, 64))
    r = waves[0]
    for i in range(1, 4):
        r = r + waves[i]
    return r


def _sum_in_kernel_order(terms):
    """terms (H, W, c) f64, zero where a pixel adds nothing -> the plate's sum: per lane in channel order, per wave of 64 pixels of a
    row, then fold() over the waves at index Y tiles_x + bx"""
    H, W, c = terms.shape
    lane = np.zeros((H, W))
    for ch in range(c):
        lane = lane + terms[..., ch]
    tx = -(-W // 64)
    pad = np.zeros((H, tx * 64))
    pad[:, :W] = lane
    return fold(_butterfly(pad.reshape(H, tx, 64)).reshape(-1))


def plate(frames, index, W, H, ox=0, oy=0, flows=None, params=None, occ=None, exclude=None, mode=0, min_count=1, fill=0.0, ref=None):
    """frames (T, h, w[, c]) f32 or uint8; index (n, K) ints; flows (n, K, H, W, 2) f32 or params (n, K, 6) f64; occ (n, K, H, W)
    uint8 or None; exclude (T, h, w) uint8 or None; ref (n, H, W[, c]) or None.
    Returns dst (n, H, W[, c]) of frames' type, count (n, H, W) uint8, code (n, H, W) uint8, stats (n, 6) f64, coverage (n, H, W)."""
    frames = np.asarray(frames)
    u8 = frames.dtype == np.uint8
    T, h, w = frames.shape[:3]
    S = frames.astype(f32).reshape(T, h, w, -1)
    noc = S.shape[3]
    index = np.asarray(index, np.int64)
    n, K = index.shape
    xg = np.broadcast_to((np.arange(W, dtype=np.int64) - ox).astype(f32)[None, :], (H, W))
    yg = np.broadcast_to((np.arange(H, dtype=np.int64) - oy).astype(f32)[:, None], (H, W))
    dst = np.zeros((n, H, W, noc), np.uint8 if u8 else f32)
    count = np.zeros((n, H, W), np.uint8)
    code = np.zeros((n, H, W), np.uint8)
    cover_all = np.zeros((n, H, W), np.int64)
    stats = np.zeros((n, 6), np.float64)
    for i in range(n):
        vals = np.full((K, H, W, noc), np.inf, f32)
        adm = np.zeros((K, H, W), bool)
        cover = np.zeros((H, W), np.int64)
        for k in range(K):
            b = int(index[i, k])
            if b < 0:
                continue
            F = np.asarray(flows[i, k], f32) if flows is not None else motion_vectors(params[i, k], w, h, W, H, ox, oy)
            u, v = F[..., 0], F[..., 1]
            with np.errstate(all="ignore"):
                fin = np.isfinite(u) & np.isfinite(v)
                xx, yy = xg + np.where(fin, u, f32(0)), yg + np.where(fin, v, f32(0))
            val, inside, (x1, x2, y1, y2) = taps(S[b], xx, yy)
            ok = fin & inside
            cover += ok
            if occ is not None:
                ok = ok & (occ[i, k] == 0)
            if exclude is not None:
                e = exclude[b]
                ok = ok & ((e[y1, x1] | e[y1, x2] | e[y2, x1] | e[y2, x2]) == 0)
            ok = ok & ~np.isnan(val).any(-1)
            adm[k] = ok
            vals[k] = np.where(ok[..., None], val, f32(np.inf))
        m = adm.sum(0)
        first = np.take_along_axis(vals, np.argmax(adm, 0)[None, ..., None], 0)[0]
        with np.errstate(all="ignore"):
            if mode == 0:
                s = np.sort(vals, axis=0, kind="stable")            # the admitted values first, ties in k order
                lo = np.take_along_axis(s, np.maximum((m - 1) // 2, 0)[None, ..., None], 0)[0]
                hi = np.take_along_axis(s, np.minimum(m // 2, K - 1)[None, ..., None], 0)[0]
                est = np.where((m % 2 == 1)[..., None], lo, (lo + hi) * f32(0.5))
            else:
                tot = np.zeros((H, W, noc), f32)
                seen = np.zeros((H, W), bool)
                for k in range(K):
                    nxt = np.where(seen[..., None], tot + vals[k], vals[k])
                    tot = np.where(adm[k][..., None], nxt, tot)
                    seen = seen | adm[k]
                est = tot / m.astype(f32)[..., None]
        assert est.dtype == f32
        cd = np.where(m >= min_count, 0, np.where(cover < min_count, 2, 1)).astype(np.uint8)
        out = np.where((cd == 0)[..., None], est, f32(fill)).astype(f32)
        dst[i] = WR.to_u8(out) if u8 else out
        count[i], code[i], cover_all[i] = m, cd, cover
        stats[i, :3] = np.bincount(cd.ravel(), minlength=3)[:3]
        stats[i, 3] = m.sum()
        if ref is not None:
            R = np.asarray(ref[i]).astype(f32).reshape(H, W, noc)
            good = (cd == 0)[..., None]
            with np.errstate(all="ignore"):
                stats[i, 4] = _sum_in_kernel_order(np.where(good, np.abs(R - est).astype(np.float64), 0.0))
                stats[i, 5] = _sum_in_kernel_order(np.where(good, np.abs(R - first).astype(np.float64), 0.0))
    return dst.reshape((n, H, W) + frames.shape[3:]), count, code, stats, cover_all


def plate_motions(params, ref=0):
    """params (T, 6) f64, the motions frame k -> k+1 -> (T+1, 6): C_k . C_ref^-1 - I (flowonthego_amd.plate.plate_motions)"""
    params = np.asarray(params, np.float64)
    path = [tuple(np.float64(v) for v in (1, 0, 0, 0, 1, 0))]
    for p in params:
        path.append(M._compose((p[0] + 1.0, p[1], p[2], p[3], p[4] + 1.0, p[5]), path[-1]))
    Cs = np.array(path, np.float64)
    Wm = M._compose(tuple(Cs[:, i] for i in range(6)), M._inverse(tuple(Cs[ref, i] for i in range(6))))
    return np.stack((Wm[0] - 1.0, Wm[1], Wm[2], Wm[3], Wm[4] - 1.0, Wm[5]), axis=1)


def mosaic_canvas(motions, w, h):
    """(W, H, ox, oy): the integer bounding box of every frame's corners in reference coordinates"""
    xs, ys = [], []
    for a00, a01, tx, a10, a11, ty in np.asarray(motions, np.float64).tolist():
        m00, m11 = a00 + 1.0, a11 + 1.0
        det = m00 * m11 - a01 * a10
        for cx in (0.0, float(w - 1)):
            for cy in (0.0, float(h - 1)):
                dx, dy = cx - tx, cy - ty
                xs.append((m11 * dx - a01 * dy) / det)
                ys.append((m00 * dy - a10 * dx) / det)
    x0, x1, y0, y1 = math.floor(min(xs)), math.ceil(max(xs)), math.floor(min(ys)), math.ceil(max(ys))
    return x1 - x0 + 1, y1 - y0 + 1, -x0, -y0


# ---- the scene of the end-to-end tests ------------------------------------------------------------------------------------------
BIG_W, BIG_H = 640, 384          # the crops of the end-to-end quality test: at 320 x 192 the flows of this scene are too poor to align


def crops_scene(image, T=8, w=M.CROP_W, h=M.CROP_H):
    """motion_ref.jittered_crops(image, T, patch=True) with what is known about it: frames (T+1, h, w) uint8, the integer motions
    reference (frame 0) -> frame k as (T+1, 6) f64, the canvas (W, H, ox, oy), the underlying image on the canvas (H, W) uint8 and
    the patch's footprint per frame (T+1, h, w) uint8.  Another w x h: the same walk, the same patch, larger crops."""
    frames, off = M.jittered_crops(image, T=T, patch=True)
    if (w, h) != (M.CROP_W, M.CROP_H):
        big = []
        for k in range(T + 1):
            x, y = M.CROP_X + off[k, 0], M.CROP_Y + off[k, 1]
            f = image[y:y + h, x:x + w].copy()
            f[40 + 4 * k:104 + 4 * k, 60 + 5 * k:156 + 5 * k] = image[700:764, 200:296]
            big.append(f)
        frames = np.stack(big)
    K, h, w = frames.shape
    motions = np.zeros((K, 6))
    motions[:, 2] = off[0, 0] - off[:, 0]
    motions[:, 5] = off[0, 1] - off[:, 1]
    W, H, ox, oy = mosaic_canvas(motions, w, h)
    x0, y0 = M.CROP_X + off[0, 0] - ox, M.CROP_Y + off[0, 1] - oy
    truth = image[y0:y0 + H, x0:x0 + W].copy()
    foot = np.zeros((K, h, w), np.uint8)
    for k in range(K):
        foot[k, 40 + 4 * k:104 + 4 * k, 60 + 5 * k:156 + 5 * k] = 1
    return frames, motions, (W, H, ox, oy), truth, foot


def stamp(maps, motions, canvas):
    """maps (K, h, w) of 0 / 1 per frame pixel, integer translations reference -> frame, a canvas (W, H, ox, oy) -> per canvas pixel
    the number of frames whose sample there has a 1 (the frame's part outside the canvas is cut off)"""
    K, h, w = maps.shape
    W, H, ox, oy = canvas
    hit = np.zeros((H, W), np.int64)
    for k in range(K):
        X0, Y0 = ox - int(motions[k, 2]), oy - int(motions[k, 5])      # canvas position of the frame's pixel (0, 0)
        xa, xb, ya, yb = max(X0, 0), min(X0 + w, W), max(Y0, 0), min(Y0 + h, H)
        if xa < xb and ya < yb:
            hit[ya:yb, xa:xb] += maps[k, ya - Y0:yb - Y0, xa - X0:xb - X0]
    return hit
