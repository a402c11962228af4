"""The global-motion fit and the stabilisation path restated in numpy, operation for operation as include/fotg.h and
flowonthego_amd/csrc/motion.hip.h define them: exact int64 sums, the f64 solve in its written order (Python floats: IEEE doubles,
one rounding per operation), the f32 classification, and the path algebra of flowonthego_amd.motion.smoothing_motions."""
import numpy as np

f32 = np.float32
MODELS = ("translation", "similarity", "affine")
MIN_PIXELS = (1, 2, 3)


def coords(w, h):
    """X = 2x - (w-1), Y = 2y - (h-1) as (h, w) int64"""
    X = 2 * np.arange(w, dtype=np.int64) - (w - 1)
    Y = 2 * np.arange(h, dtype=np.int64) - (h - 1)
    return np.broadcast_to(X[None, :], (h, w)), np.broadcast_to(Y[:, None], (h, w))


def known(flow):
    with np.errstate(invalid="ignore"):
        return (np.abs(flow[..., 0]) <= f32(4096)) & (np.abs(flow[..., 1]) <= f32(4096))


def fixed_point(flow, k):
    """U, V = rintf(256 u), rintf(256 v) as int64 where known (0 elsewhere: never summed)"""
    safe = np.where(k[..., None], flow, f32(0))
    q = np.rint(safe * f32(256)).astype(np.int64)
    return q[..., 0], q[..., 1]


def sums(X, Y, U, V, sel):
    """the twelve sums over the selected pixels, as Python integers"""
    x, y, u, v = X[sel], Y[sel], U[sel], V[sel]
    return [int(sel.sum()), int(x.sum()), int(y.sum()), int((x * x).sum()), int((x * y).sum()), int((y * y).sum()),
            int(u.sum()), int((x * u).sum()), int((y * u).sum()), int(v.sum()), int((x * v).sum()), int((y * v).sum())]


def solve(S, model):
    """c0 .. c5 (Python floats) or None where the system is unusable"""
    if S[0] < MIN_PIXELS[model]:
        return None
    n, sx, sy, sxx, sxy, syy, su, sxu, syu, sv, sxv, syv = (float(s) for s in S)
    if model == 0:
        return [0.0, 0.0, su / n, 0.0, 0.0, sv / n]
    if model == 1:
        D = n * (sxx + syy) - (sx * sx + sy * sy)
        if not D > 0.0:
            return None
        a = (n * (sxu + syv) - (sx * su + sy * sv)) / D
        b = (n * (sxv - syu) - (sx * sv - sy * su)) / D
        return [a, -b, ((su - a * sx) + b * sy) / n, b, a, ((sv - b * sx) - a * sy) / n]
    A00, A01, A02 = syy * n - sy * sy, sx * sy - sxy * n, sxy * sy - syy * sx
    A11, A12, A22 = sxx * n - sx * sx, sx * sxy - sxx * sy, sxx * syy - sxy * sxy
    det = (sxx * A00 + sxy * A01) + sx * A02
    if not det > 0.0:
        return None
    return [((A00 * sxu + A01 * syu) + A02 * su) / det, ((A01 * sxu + A11 * syu) + A12 * su) / det,
            ((A02 * sxu + A12 * syu) + A22 * su) / det,
            ((A00 * sxv + A01 * syv) + A02 * sv) / det, ((A01 * sxv + A11 * syv) + A12 * sv) / det,
            ((A02 * sxv + A12 * syv) + A22 * sv) / det]


def to_pixel_frame(c, w, h):
    wx, hy = float(w - 1), float(h - 1)
    P = []
    for r in range(2):
        q0, q1, q2 = c[3 * r] * 0.00390625, c[3 * r + 1] * 0.00390625, c[3 * r + 2] * 0.00390625
        P += [q0 * 2.0, q1 * 2.0, (q2 - q0 * wx) - q1 * hy]
    return P


def coef(P, w, h):
    """the six f32 coefficients of the prediction from the pixel-frame parameters"""
    wx, hy = float(w - 1), float(h - 1)
    k = []
    for r in range(2):
        h0, h1 = float(P[3 * r]) * 0.5, float(P[3 * r + 1]) * 0.5
        k += [f32(h0), f32(h1), f32((float(P[3 * r + 2]) + h0 * wx) + h1 * hy)]
    return k


def predict(P, w, h):
    """(h, w, 2) f32: (pu, pv) at every pixel"""
    X, Y = coords(w, h)
    Xf, Yf = X.astype(f32), Y.astype(f32)
    k = coef(P, w, h)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.stack([(k[0] * Xf + k[1] * Yf) + k[2], (k[3] * Xf + k[4] * Yf) + k[5]], -1)


def motion_flow(P, w, h):
    return predict(P, w, h)


def follows(flow, P, thresh):
    """(du, dv) and the test du du + dv dv <= thresh thresh, all f32"""
    h, w = flow.shape[:2]
    with np.errstate(over="ignore", invalid="ignore"):
        res = flow - predict(P, w, h)
        ok = res[..., 0] * res[..., 0] + res[..., 1] * res[..., 1] <= f32(thresh) * f32(thresh)
    return res, ok


def fit(flow, mask=None, model=2, iters=3, thresh=1.0):
    """one image: flow (h, w, 2) f32, mask (h, w) uint8 or None -> dict(params (6,) f64, code (h, w) uint8, residual (h, w, 2) f32,
    stats (6,) int64, sums (12,) int64)"""
    if isinstance(model, str):
        model = MODELS.index(model)
    flow = np.asarray(flow, f32)
    h, w = flow.shape[:2]
    X, Y = coords(w, h)
    k = known(flow)
    U, V = fixed_point(flow, k)
    adm = k if mask is None else k & (np.asarray(mask) == 0)
    P, fitted, S = [0.0] * 6, 1, None
    for r in range(iters + 1):
        sel = adm if r == 0 else adm & follows(flow, P, thresh)[1]
        S = sums(X, Y, U, V, sel)
        c = solve(S, model)
        if c is None:
            fitted = 0
        else:
            P = to_pixel_frame(c, w, h)
    res, ok = follows(flow, P, thresh)
    code = np.where(~k, 3, np.where(~adm, 2, np.where(ok, 0, 1))).astype(np.uint8)
    stats = np.array([(code == i).sum() for i in range(4)] + [S[0], fitted], np.int64)
    return dict(params=np.array(P, np.float64), code=code, residual=res.astype(f32), stats=stats, sums=np.array(S, np.int64))


def corner_error(P, Q, w, h):
    """the largest displacement difference between two motions over the four corners of the image, in pixels"""
    P, Q = np.asarray(P, np.float64), np.asarray(Q, np.float64)
    worst = 0.0
    for x in (0.0, w - 1.0):
        for y in (0.0, h - 1.0):
            d = (P - Q) * np.array([x, y, 1.0, x, y, 1.0])
            worst = max(worst, float(np.hypot(d[:3].sum(), d[3:].sum())))
    return worst


# ---- the camera path of stabilize --------------------------------------------------------------------------------------------
def _compose(A, B):
    a00, a01, a02, a10, a11, a12 = A
    b00, b01, b02, b10, b11, b12 = B
    return (a00 * b00 + a01 * b10, a00 * b01 + a01 * b11, (a00 * b02 + a01 * b12) + a02,
            a10 * b00 + a11 * b10, a10 * b01 + a11 * b11, (a10 * b02 + a11 * b12) + a12)


def _inverse(S):
    s00, s01, s02, s10, s11, s12 = S
    det = s00 * s11 - s01 * s10
    i00, i01, i10, i11 = s11 / det, -s01 / det, -s10 / det, s00 / det
    return (i00, i01, -(i00 * s02 + i01 * s12), i10, i11, -(i10 * s02 + i11 * s12))


def smoothing_motions(params, radius):
    """params (T, 6) f64 -> (T+1, 6) f64: the parameters of C_k . S_k^-1 - I per frame (flowonthego_amd.motion.smoothing_motions)"""
    params = np.asarray(params, np.float64)
    T = params.shape[0]
    path = [tuple(np.float64(v) for v in (1, 0, 0, 0, 1, 0))]
    for k in range(T):
        p = params[k]
        path.append(_compose((p[0] + 1.0, p[1], p[2], p[3], p[4] + 1.0, p[5]), path[-1]))
    Cs = np.array(path, np.float64)
    r = min(radius, T)
    pad = np.zeros((T + 1 + 2 * r, 6))
    pad[r:r + T + 1] = Cs
    acc = pad[0:T + 1]
    for d in range(1, 2 * r + 1):
        acc = acc + pad[d:d + T + 1]
    cnt = np.array([min(k + r, T) - max(k - r, 0) + 1 for k in range(T + 1)], np.float64)
    S = acc / cnt[:, None]
    W = _compose(tuple(Cs[:, i] for i in range(6)), _inverse(tuple(S[:, i] for i in range(6))))
    return np.stack((W[0] - 1.0, W[1], W[2], W[3], W[4] - 1.0, W[5]), axis=1)


# ---- seeded inputs shared by the CPU and the GPU tests -----------------------------------------------------------------------
CROP_W, CROP_H, CROP_X, CROP_Y = 320, 192, 800, 400


def jittered_crops(image, T=8, seed=7, step=6, patch=False):
    """T+1 crops (CROP_H x CROP_W) of image around (CROP_X, CROP_Y), the crop window jittered by a random walk with steps from
    {-step, 0, step} px: (frames uint8 (T+1, h, w), offsets int (T+1, 2) as (x, y)).  The camera flow frame k -> k+1 is
    offsets[k] - offsets[k+1].  patch: a 96 x 64 piece of another part of the image pasted at (60 + 5k, 40 + 4k) of frame k."""
    rng = np.random.default_rng(seed)
    off = np.cumsum(np.vstack([np.zeros((1, 2), np.int64), rng.integers(-1, 2, (T, 2)) * step]), 0)
    frames = []
    for k in range(T + 1):
        x, y = CROP_X + off[k, 0], CROP_Y + off[k, 1]
        f = image[y:y + CROP_H, x:x + CROP_W].copy()
        if patch:
            f[40 + 4 * k:104 + 4 * k, 60 + 5 * k:156 + 5 * k] = image[700:764, 200:296]
        frames.append(f)
    return np.stack(frames), off



def make_scene(w, h, seed, outlier_share=0.25, noise=0.2, specials=True):
    """an affine background with noise, a block moving by (6.5, -4) on its own, and (specials) the values the definition singles
    out: NaN, infinities, components just inside and beyond 4096 px, a mask with every code.  Returns (flow, mask, P_true)."""
    rng = np.random.default_rng(seed)
    P = np.array([0.004, -0.011, 1.75, 0.009, 0.006, -2.5])
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    flow = np.stack([P[0] * xs + P[1] * ys + P[2], P[3] * xs + P[4] * ys + P[5]], -1) + noise * rng.standard_normal((h, w, 2))
    bh = max(1, int(round(h * np.sqrt(outlier_share))))
    bw = max(1, int(round(w * outlier_share * h / bh))) if outlier_share > 0 else 0
    if bw:
        bw = min(bw, w)
        y0, x0 = (h - bh) // 2, (w - bw) // 2 + w // 8               # an object in mid-frame, a little off the centre
        x0 = min(x0, w - bw)
        flow[y0:y0 + bh, x0:x0 + bw] = (6.5, -4.0) + noise * rng.standard_normal((bh, bw, 2))
    flow = flow.astype(f32)
    mask = np.zeros((h, w), np.uint8)
    if specials and w * h >= 64:
        idx = rng.choice(w * h, 12, replace=False)
        fl = flow.reshape(-1, 2)
        fl[idx[0]] = (np.nan, 1.0)
        fl[idx[1]] = (2.0, np.inf)
        fl[idx[2]] = (-np.inf, np.nan)
        fl[idx[3]] = (4096.0, -4096.0)                 # the largest known magnitude
        fl[idx[4]] = (np.nextafter(f32(4096), f32(5000)), 0.0)
        fl[idx[5]] = (0.0, -1e30)
        fl[idx[6]] = (3.0e38, 3.0e38)
        m = mask.reshape(-1)
        m[rng.choice(w * h, w * h // 9, replace=False)] = 1
        m[rng.choice(w * h, w * h // 31, replace=False)] = 2
        m[rng.choice(w * h, w * h // 47, replace=False)] = 3
        m[idx[7]] = 255
        m[idx[0]] = 1                                   # unknown wins over masked
    return flow, mask, P
