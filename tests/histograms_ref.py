"""The motion histograms (HOF, MBHx, MBHy per cell and per object) restated in numpy, in the order include/fotg.h and
flowonthego_amd/csrc/histograms.hip.h define them: the residual in f32 with the arithmetic of motion_ref.predict, everything after it
in exact integers (int64; Python integers for the square root), so the GPU is compared byte for byte.  Vectorised over the image;
M and A are also given for single vectors (mag1, angle1), which the tests use for the hand cases."""
import math

import numpy as np

import motion_ref as R

f32 = np.float32
NREC = 32
HOF, ZERO, MBHX, MBHY, N, NMBH, NBAD, SM, SU, SV = 0, 8, 9, 17, 25, 26, 27, 28, 29, 30
CELLS = (8, 16, 32)
THRESH256 = 102                                   # rint(0.4 * 256)

# T[k] = rint(256 atan(k / 256) / (pi / 4)), k = 0 .. 256
ATAN = np.array([
    0,   1,   3,   4,   5,   6,   8,   9,  10,  11,  13,  14,  15,  17,  18,  19,  20,  22,  23,  24,
   25,  27,  28,  29,  30,  32,  33,  34,  36,  37,  38,  39,  41,  42,  43,  44,  46,  47,  48,  49,
   51,  52,  53,  54,  55,  57,  58,  59,  60,  62,  63,  64,  65,  67,  68,  69,  70,  71,  73,  74,
   75,  76,  77,  79,  80,  81,  82,  83,  85,  86,  87,  88,  89,  91,  92,  93,  94,  95,  96,  98,
   99, 100, 101, 102, 103, 104, 106, 107, 108, 109, 110, 111, 112, 114, 115, 116, 117, 118, 119, 120,
  121, 122, 124, 125, 126, 127, 128, 129, 130, 131, 132, 133, 134, 135, 137, 138, 139, 140, 141, 142,
  143, 144, 145, 146, 147, 148, 149, 150, 151, 152, 153, 154, 155, 156, 157, 158, 159, 160, 161, 162,
  163, 164, 165, 166, 167, 168, 169, 170, 171, 172, 173, 174, 175, 176, 177, 177, 178, 179, 180, 181,
  182, 183, 184, 185, 186, 187, 188, 188, 189, 190, 191, 192, 193, 194, 195, 195, 196, 197, 198, 199,
  200, 201, 201, 202, 203, 204, 205, 206, 206, 207, 208, 209, 210, 211, 211, 212, 213, 214, 215, 215,
  216, 217, 218, 219, 219, 220, 221, 222, 222, 223, 224, 225, 225, 226, 227, 228, 228, 229, 230, 231,
  231, 232, 233, 234, 234, 235, 236, 236, 237, 238, 239, 239, 240, 241, 241, 242, 243, 243, 244, 245,
  245, 246, 247, 248, 248, 249, 250, 250, 251, 251, 252, 253, 253, 254, 255, 255, 256,
], np.int64)


def atan_formula():
    return [int(round(256.0 * math.atan(k / 256.0) / (math.pi / 4.0))) for k in range(257)]


def mag1(a, b):
    """M(a, b) of one vector, by Python's exact integer square root"""
    return math.isqrt(int(a) * int(a) + int(b) * int(b))


def angle1(a, b):
    """A(a, b) of one vector != (0, 0)"""
    a, b = int(a), int(b)
    ax, ay = abs(a), abs(b)
    phi = int(ATAN[(ay << 8) // ax]) if ax >= ay else 512 - int(ATAN[(ax << 8) // ay])
    if a >= 0 and b >= 0:
        return phi
    if a < 0 and b >= 0:
        return 1024 - phi
    if a < 0 and b < 0:
        return 1024 + phi
    return (2048 - phi) % 2048


def mag(a, b):
    """M over int64 arrays: the f64 root, then corrected against the exact 64-bit squares"""
    n = a * a + b * b
    s = np.floor(np.sqrt(n.astype(np.float64))).astype(np.int64)
    s = np.where(s * s > n, s - 1, s)
    s = np.where((s + 1) * (s + 1) <= n, s + 1, s)
    assert np.all(s * s <= n) and np.all((s + 1) * (s + 1) > n)
    return s


def angle(a, b):
    """A over int64 arrays; 0 where a = b = 0 (never used there)"""
    ax, ay = np.abs(a), np.abs(b)
    lo, hi = np.minimum(ax, ay), np.maximum(ax, ay)
    t = ATAN[(lo << 8) // np.maximum(hi, 1)]
    phi = np.where(ax >= ay, t, 512 - t)
    return np.where(a >= 0, np.where(b >= 0, phi, (2048 - phi) % 2048), np.where(b >= 0, 1024 - phi, 1024 + phi))


def soft(m, A):
    """(b0, w0, b1, w1) of step 5"""
    b0, f = A >> 8, A & 255
    w1 = (m * f) >> 8
    return b0, m - w1, (b0 + 1) & 7, w1


def fixed(flow, mask=None, P=None):
    """steps 1 and 2 of one image: flow (h, w, 2) f32 -> (adm bool, U, V int64; U = V = 0 where not admissible)"""
    flow = np.asarray(flow, f32)
    h, w = flow.shape[:2]
    ok = R.known(flow)
    res = flow
    if P is not None:
        with np.errstate(over="ignore", invalid="ignore"):
            res = flow - R.predict(P, w, h)
        ok = ok & R.known(res)
    if mask is not None:
        ok = ok & (np.asarray(mask) == 0)
    U, V = R.fixed_point(res, ok)
    return ok, U, V


def pixel_records(adm, U, V, thresh256=THRESH256):
    """(h, w, 32) int64: what each pixel adds to the record of its cell or object"""
    h, w = adm.shape
    rec = np.zeros((h, w, NREC), np.int64)
    yy, xx = np.nonzero(np.ones((h, w), bool))
    yy, xx = yy.reshape(h, w), xx.reshape(h, w)

    def add(sel, off, m, a, b):
        sel = sel & (m > 0)
        b0, w0, b1, w1 = soft(m, angle(a, b))
        np.add.at(rec, (yy[sel], xx[sel], off + b0[sel]), w0[sel])
        np.add.at(rec, (yy[sel], xx[sel], off + b1[sel]), w1[sel])

    m = mag(U, V)
    rec[..., N] = adm
    rec[..., NBAD] = ~adm
    rec[..., SM] = np.where(adm, m, 0)
    rec[..., SU] = np.where(adm, U, 0)
    rec[..., SV] = np.where(adm, V, 0)
    zero = adm & (m < thresh256)
    rec[..., ZERO] = zero
    add(adm & ~zero, HOF, m, U, V)
    xl, xr = np.maximum(np.arange(w) - 1, 0), np.minimum(np.arange(w) + 1, w - 1)
    yu, yd = np.maximum(np.arange(h) - 1, 0), np.minimum(np.arange(h) + 1, h - 1)
    part = adm & adm[:, xl] & adm[:, xr] & adm[yu, :] & adm[yd, :]
    rec[..., NMBH] = part
    Ux, Uy, Vx, Vy = U[:, xr] - U[:, xl], U[yd, :] - U[yu, :], V[:, xr] - V[:, xl], V[yd, :] - V[yu, :]
    add(part, MBHX, mag(Ux, Uy), Ux, Uy)
    add(part, MBHY, mag(Vx, Vy), Vx, Vy)
    return rec


def group_cells(rec, cell):
    h, w = rec.shape[:2]
    gh, gw = (h + cell - 1) // cell, (w + cell - 1) // cell
    out = np.zeros((gh, gw, NREC), np.int64)
    cy, cx = np.arange(h) // cell, np.arange(w) // cell
    np.add.at(out, (np.broadcast_to(cy[:, None], (h, w)), np.broadcast_to(cx[None, :], (h, w))), rec)
    return out


def group_objects(rec, ids, rows):
    out = np.zeros((rows, NREC), np.int64)
    ids = np.asarray(ids).astype(np.int64)
    sel = (ids >= 0) & (ids < rows)
    np.add.at(out, ids[sel], rec[sel])
    return out


def histograms(flow, mask=None, params=None, cell=16, thresh256=THRESH256, ids=None, rows=256, cells=True):
    """a batch: flow (n, h, w, 2), mask (n, h, w) or None, params (n, 6) or None, ids (n, h, w) or None ->
    (cells (n, gh, gw, 32) or None, objects (n, rows, 32) or None)"""
    assert cell in CELLS and thresh256 >= 0 and 1 <= rows <= 1024
    n = flow.shape[0]
    oc, oo = [], []
    for i in range(n):
        adm, U, V = fixed(flow[i], None if mask is None else mask[i], None if params is None else params[i])
        rec = pixel_records(adm, U, V, thresh256)
        if cells:
            oc.append(group_cells(rec, cell))
        if ids is not None:
            oo.append(group_objects(rec, ids[i], rows))
    return (np.stack(oc) if cells else None), (np.stack(oo) if ids is not None else None)


def from_fixed(U, V, adm=None, cell=8, thresh256=THRESH256):
    """the cells of one image given directly in fixed point (the CPU tests)"""
    U, V = np.asarray(U, np.int64), np.asarray(V, np.int64)
    adm = np.ones(U.shape, bool) if adm is None else np.asarray(adm, bool)
    return group_cells(pixel_records(adm, np.where(adm, U, 0), np.where(adm, V, 0), thresh256), cell)


def float_hof(U, V, thresh256=THRESH256):
    """the textbook form per pixel: f64 hypot and atan2 on the same U, V, soft-binned over eight bins -> (h, w, 8) f64"""
    U, V = np.asarray(U, np.float64), np.asarray(V, np.float64)
    m = np.hypot(U, V)
    pos = (np.arctan2(V, U) / (math.pi / 4.0)) % 8.0
    b0 = np.floor(pos).astype(np.int64) % 8
    fr = pos - np.floor(pos)
    out = np.zeros(U.shape + (8,), np.float64)
    keep = m >= thresh256
    yy, xx = np.nonzero(keep)
    np.add.at(out, (yy, xx, b0[keep]), (m * (1.0 - fr))[keep])
    np.add.at(out, (yy, xx, (b0[keep] + 1) % 8), (m * fr)[keep])
    return out


def descriptors(hist):
    """motion_descriptors in numpy: (..., 32) int64 -> (..., 25) f32"""
    h = np.asarray(hist, np.float64)
    parts = (np.concatenate((h[..., 0:8], h[..., 8:9] * 256.0), -1), h[..., 9:17], h[..., 17:25])
    out = []
    for p in parts:
        s = p.sum(-1, keepdims=True)
        out.append(np.sqrt(p / np.where(s > 0, s, 1.0)))
    return np.concatenate(out, -1).astype(f32)
