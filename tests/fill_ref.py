"""The pull-push hole filling restated in numpy, straight from the definition in include/fotg.h (fotg_fill): a pyramid of exact
integer sums over the known pixels, one f64 division per block, and the bilinear push in f32 in the definition's order.  Vectorised
per level, nothing clever: this is what the GPU has to equal byte for byte.  naive() is the same definition as loops over the
levels and the pixels, for the small shapes of tests/test_fill.py."""
import numpy as np

F32 = np.float32
CODES = ("known", "filled", "unfilled")
STATS = ("known", "filled", "unfilled", "depth")


def hole_map(hole, fg=None):
    """(..., h, w) uint8 -> bool: the holes.  fg None: every non-zero byte; otherwise the byte values (each 0 .. 7) that are holes"""
    hole = np.asarray(hole)
    assert hole.dtype == np.uint8
    if fg is None:
        return hole != 0
    out = np.zeros(hole.shape, bool)
    for c in fg:
        assert 0 <= int(c) <= 7
        out |= hole == int(c)
    return out


def known_map(src, hole=None, fg=None):
    """src (h, w, c) f32 or uint8 -> bool (h, w): not a hole and, for f32, every channel finite with |v| <= 32768"""
    assert src.dtype in (np.float32, np.uint8) and src.ndim == 3
    known = np.ones(src.shape[:2], bool) if hole is None else ~hole_map(hole, fg)
    if src.dtype == np.float32:
        with np.errstate(invalid="ignore"):
            known = known & (np.abs(src) <= F32(32768)).all(axis=2)          # false for a NaN and an infinity
    return known


def quantise(src, known):
    """q = lrintf(256 v) as int64 at known pixels, 0 elsewhere"""
    if src.dtype == np.uint8:
        q = src.astype(np.int64) * 256
    else:
        v = np.where(known[..., None], src, F32(0))
        p = F32(256) * v
        assert p.dtype == np.float32
        q = np.rint(p).astype(np.int64)                                     # rint: half to even, as lrintf
    return np.where(known[..., None], q, 0)


def pull(S0, N0):
    """the levels [(S, N)]: S int64 (h_l, w_l, c), N int64 (h_l, w_l), up to the first level of size 1 x 1"""
    levels = [(S0, N0)]
    while levels[-1][1].shape != (1, 1):
        S, N = levels[-1]
        h, w = N.shape
        Sp = np.zeros((2 * ((h + 1) >> 1), 2 * ((w + 1) >> 1), S.shape[2]), np.int64)
        Np = np.zeros(Sp.shape[:2], np.int64)
        Sp[:h, :w] = S
        Np[:h, :w] = N
        levels.append((Sp[0::2, 0::2] + Sp[0::2, 1::2] + Sp[1::2, 0::2] + Sp[1::2, 1::2],
                       Np[0::2, 0::2] + Np[0::2, 1::2] + Np[1::2, 0::2] + Np[1::2, 1::2]))
    return levels


def mean(S, N):
    """M = (float)((double)S / (double)(256 N)) where N > 0 (0 elsewhere)"""
    assert np.abs(S).max(initial=0) < 2 ** 53
    den = np.where(N > 0, 256 * N, 1).astype(np.float64)[..., None]
    m = (S.astype(np.float64) / den).astype(F32)
    assert m.dtype == np.float32
    return m


def bilinear(Fp, h, w):
    """the bilinear values of a level of h x w pixels from its parents' level Fp f32 (hp, wp, c)"""
    assert Fp.dtype == np.float32
    hp, wp = Fp.shape[:2]
    x, y = np.arange(w), np.arange(h)
    px, py = x >> 1, y >> 1
    px2 = np.clip(px + np.where(x & 1, 1, -1), 0, wp - 1)
    py2 = np.clip(py + np.where(y & 1, 1, -1), 0, hp - 1)
    a, b = Fp[py[:, None], px[None, :]], Fp[py[:, None], px2[None, :]]
    c, d = Fp[py2[:, None], px[None, :]], Fp[py2[:, None], px2[None, :]]
    out = ((a * F32(9) + b * F32(3)) + (c * F32(3) + d)) * F32(0.0625)
    assert out.dtype == np.float32
    return out


def to_u8(f):
    assert f.dtype == np.float32
    return np.clip(np.rint(f), F32(0), F32(255)).astype(np.uint8)


def fill_one(src, hole=None, fg=None):
    """src (h, w, c) f32 or uint8, hole (h, w) uint8 or None -> (dst of src's type and shape, code uint8 (h, w), stats int64 (4,))"""
    known = known_map(src, hole, fg)
    assert src.dtype == np.float32 or hole is not None
    levels = pull(quantise(src, known), known.astype(np.int64))
    L = len(levels) - 1
    empty_levels = [l for l, (_, N) in enumerate(levels) if (N == 0).any()]
    depth = 1 + max(empty_levels) if empty_levels else 0
    nknown = int(known.sum())
    nholes = known.size - nknown
    if levels[L][1][0, 0] == 0:
        return src.copy(), np.where(known, 0, 2).astype(np.uint8), np.array([nknown, 0, nholes, depth], np.int64)
    F = mean(*levels[L])
    for l in range(L - 1, -1, -1):
        S, N = levels[l]
        B = bilinear(F, *N.shape)
        F = B if l == 0 else np.where((N > 0)[..., None], mean(S, N), B)
        assert F.dtype == np.float32
    dst = np.where(known[..., None], src, F if src.dtype == np.float32 else to_u8(F))
    assert dst.dtype == src.dtype
    return dst, np.where(known, 0, 1).astype(np.uint8), np.array([nknown, nholes, 0, depth], np.int64)


def _forms(src, hole):
    """src (n, h, w[, c]) / (h, w[, c]) and hole (n, h, w) / (h, w) / None as (n, h, w, c), (n, h, w) or None, and how to undo it"""
    src = np.asarray(src)
    if hole is not None:
        hole = np.asarray(hole)
        single = hole.ndim == 2
        chan = src.ndim == hole.ndim + 1
    else:
        single = src.ndim == 3
        chan = True
    s = src if chan else src[..., None]
    if single:
        s, hole = s[None], (None if hole is None else hole[None])
    assert s.ndim == 4 and (hole is None or hole.shape == s.shape[:3])
    return s, hole, single, chan


def fill_holes(src, hole=None, fg=None):
    """flowonthego_amd.fill.fill_holes restated: (dst, code, stats), shaped as the call shapes them"""
    s, ho, single, chan = _forms(src, hole)
    res = [fill_one(np.ascontiguousarray(s[k]), None if ho is None else ho[k], fg) for k in range(s.shape[0])]
    dst, code, stats = (np.stack([r[j] for r in res]) for j in range(3))
    if not chan:
        dst = dst[..., 0]
    return (dst[0], code[0], stats[0]) if single else (dst, code, stats)


def naive(src, hole=None, fg=None):
    """fill_one as loops over the levels and the pixels, in Python integers and numpy f32 scalars"""
    h, w, ch = src.shape
    known = known_map(src, hole, fg)
    S = [[[(int(np.rint(F32(256) * src[y, x, c])) if src.dtype == np.float32 else 256 * int(src[y, x, c])) if known[y, x] else 0
           for c in range(ch)] for x in range(w)] for y in range(h)]
    N = [[1 if known[y, x] else 0 for x in range(w)] for y in range(h)]
    levels = [(S, N, w, h)]
    while levels[-1][2:] != (1, 1):
        S, N, wl, hl = levels[-1]
        wn, hn = (wl + 1) >> 1, (hl + 1) >> 1
        Sn = [[[0] * ch for _ in range(wn)] for _ in range(hn)]
        Nn = [[0] * wn for _ in range(hn)]
        for Y in range(hn):
            for X in range(wn):
                for j in (0, 1):
                    for i in (0, 1):
                        if 2 * X + i < wl and 2 * Y + j < hl:
                            Nn[Y][X] += N[2 * Y + j][2 * X + i]
                            for c in range(ch):
                                Sn[Y][X][c] += S[2 * Y + j][2 * X + i][c]
        levels.append((Sn, Nn, wn, hn))
    L = len(levels) - 1
    depth = 0
    for l, (_, N, wl, hl) in enumerate(levels):
        if any(N[y][x] == 0 for y in range(hl) for x in range(wl)):
            depth = l + 1
    nknown = int(known.sum())
    if levels[L][1][0][0] == 0:
        return src.copy(), np.where(known, 0, 2).astype(np.uint8), np.array([nknown, 0, h * w - nknown, depth], np.int64)
    M = lambda s, n: F32(np.float64(s) / np.float64(256 * n))
    Fp = [[[M(levels[L][0][0][0][c], levels[L][1][0][0]) for c in range(ch)]]]
    for l in range(L - 1, -1, -1):
        S, N, wl, hl = levels[l]
        wp, hp = levels[l + 1][2:]
        Fl = [[None] * wl for _ in range(hl)]
        for y in range(hl):
            for x in range(wl):
                if N[y][x] > 0 and l >= 1:
                    Fl[y][x] = [M(S[y][x][c], N[y][x]) for c in range(ch)]
                else:
                    px, py = x >> 1, y >> 1
                    px2 = min(max(px + (1 if x & 1 else -1), 0), wp - 1)
                    py2 = min(max(py + (1 if y & 1 else -1), 0), hp - 1)
                    Fl[y][x] = [((Fp[py][px][c] * F32(9) + Fp[py][px2][c] * F32(3)) + (Fp[py2][px][c] * F32(3) + Fp[py2][px2][c])) * F32(0.0625)
                                for c in range(ch)]
        Fp = Fl
    dst = src.copy()
    for y in range(h):
        for x in range(w):
            if not known[y, x]:
                for c in range(ch):
                    f = Fp[y][x][c]
                    assert type(f) is np.float32
                    dst[y, x, c] = f if src.dtype == np.float32 else min(max(np.rint(f), F32(0)), F32(255))
    return dst, np.where(known, 0, 1).astype(np.uint8), np.array([nknown, h * w - nknown, 0, depth], np.int64)
