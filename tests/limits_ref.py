"""Closed forms for the add-ons at the limits their headers promise (csrc/motion.hip.h, layers.hip.h, components.hip.h,
objtracks.hip.h, morph.hip.h): w, h = 16384, 2^28 pixels, |sum XU| = 2^61, sum U = 2^48.

No restatement can walk 2^28 pixels in a test's time, so the inputs here are separable -- u depends on x alone, v on y alone, a map
is uniform, striped, or uniform but for one byte -- and every expected integer is a product of a few one-dimensional sums, in Python
integers (which cannot overflow).  Every function takes any w, h: tests/test_limits.py proves each against the module's own
restatement on the materialised input at small sizes; tests/test_gpu_limits.py then uses the same functions at 16384 x 16384.  The
f64 solve and the f32 classification are not restated again: they are motion_ref's own functions, fed the closed-form integers.

The second half builds the inputs of the thin-frame tests (16384 x 1, 1 x 16384, 16384 x 3, 3 x 16384): flows with non-finite and
out-of-range vectors in the first and the last quad of a row, images, masks, and code maps whose runs cross every tile edge."""
import numpy as np

import motion_ref as M

f32 = np.float32
LIMIT = 16384
UNASSIGNED = 253


# ---- the separable flow -----------------------------------------------------------------------------------------------------------
def sgn_profiles(w, h):
    """ux (w,) = 4096 sgn(X), vy (h,) = -4096 sgn(Y) as f32, X = 2x - (w-1), Y = 2y - (h-1): every vector known, |U| = |V| = 2^20
    (0 on the centre column / row of an odd size)"""
    X = 2 * np.arange(w, dtype=np.int64) - (w - 1)
    Y = 2 * np.arange(h, dtype=np.int64) - (h - 1)
    return (f32(4096) * np.sign(X)).astype(f32), (f32(-4096) * np.sign(Y)).astype(f32)


def materialise(ux, vy):
    """(h, w, 2) f32: u = ux[x], v = vy[y]"""
    h, w = len(vy), len(ux)
    return np.stack([np.broadcast_to(ux[None, :], (h, w)), np.broadcast_to(vy[:, None], (h, w))], -1).astype(f32)


def _ints(a):
    return [int(v) for v in a]


def separable_sums(ux, vy, selx=None, sely=None):
    """the twelve sums (motion.SUMS) over the pixels {x in selx} x {y in sely} (None: all) of the flow u = ux[x], v = vy[y], every
    selected vector known: products of one-dimensional sums, as Python integers"""
    w, h = len(ux), len(vy)
    sx = np.ones(w, bool) if selx is None else np.asarray(selx, bool)
    sy = np.ones(h, bool) if sely is None else np.asarray(sely, bool)
    assert (np.abs(ux[sx]) <= 4096).all() and (np.abs(vy[sy]) <= 4096).all()
    X = _ints((2 * np.arange(w, dtype=np.int64) - (w - 1))[sx])
    Y = _ints((2 * np.arange(h, dtype=np.int64) - (h - 1))[sy])
    U = _ints(np.rint(ux[sx] * f32(256)).astype(np.int64))
    V = _ints(np.rint(vy[sy] * f32(256)).astype(np.int64))
    nx, ny = len(X), len(Y)
    SX, SY, SU, SV = sum(X), sum(Y), sum(U), sum(V)
    SXX, SYY = sum(a * a for a in X), sum(a * a for a in Y)
    SXU, SYV = sum(a * b for a, b in zip(X, U)), sum(a * b for a, b in zip(Y, V))
    return [nx * ny, SX * ny, nx * SY, SXX * ny, SX * SY, nx * SYY,
            SU * ny, SXU * ny, SU * SY, nx * SV, SX * SV, nx * SYV]


def _fit_from_sums(S, model, w, h, P, fitted):
    """one round of motion_ref.fit after its sums: (P, fitted)"""
    c = M.solve(S, model)
    return (P, 0) if c is None else (M.to_pixel_frame(c, w, h), fitted)


def _residual_profiles(ux, vy, P):
    """(du (w,), dv (h,)) f32 of the separable flow against parameters whose prediction is separable too (pu of x alone, pv of y
    alone: the cross coefficients are exactly zero, so motion_predict's (k0 X + k1 Y) + k2 adds an exact zero)"""
    w, h = len(ux), len(vy)
    k = M.coef(P, w, h)
    assert k[1] == 0 and k[3] == 0, "the prediction is not separable"
    Xf = (2 * np.arange(w, dtype=np.int64) - (w - 1)).astype(f32)
    Yf = (2 * np.arange(h, dtype=np.int64) - (h - 1)).astype(f32)
    pu = (k[0] * Xf + k[1] * f32(0)) + k[2]
    pv = (k[3] * f32(0) + k[4] * Yf) + k[5]
    return ux - pu, vy - pv


def within_set(ux, vy, P, thresh):
    """the pixels with du du + dv dv <= thresh thresh (f32, one rounding per operation): None for all of them, else their (xs, ys).
    f32 addition of non-negative terms is monotone, so only columns with du du <= t2 and rows with dv dv <= t2 can hold one."""
    du, dv = _residual_profiles(ux, vy, P)
    a, b = du * du, dv * dv
    t2 = f32(thresh) * f32(thresh)
    if f32(a.max() + b.max()) <= t2:
        return None
    cx, cy = np.flatnonzero(a <= t2), np.flatnonzero(b <= t2)
    assert len(cx) * len(cy) <= 1 << 24, "too many candidates for an explicit list"
    ok = (a[cx][None, :] + b[cy][:, None]) <= t2
    iy, ix = np.nonzero(ok)
    return cx[ix], cy[iy]


def _listed_sums(ux, vy, sel):
    """the twelve sums over an explicit pixel list (motion_ref.sums on the listed pixels)"""
    w, h = len(ux), len(vy)
    xs, ys = sel
    X, Y = 2 * xs.astype(np.int64) - (w - 1), 2 * ys.astype(np.int64) - (h - 1)
    U, V = np.rint(ux[xs] * f32(256)).astype(np.int64), np.rint(vy[ys] * f32(256)).astype(np.int64)
    return M.sums(X, Y, U, V, np.ones(len(xs), bool))


def _count(sel, w, h):
    return w * h if sel is None else len(sel[0])


def motion_expected(ux, vy, model, thresh=1.0):
    """fit_motion(flow, None, model, iters=0, thresh) of the separable flow: dict(sums (12 ints), params (6 floats), stats (6 ints))"""
    w, h = len(ux), len(vy)
    S = separable_sums(ux, vy)
    P, fitted = _fit_from_sums(S, model, w, h, [0.0] * 6, 1)
    follows = _count(within_set(ux, vy, P, thresh), w, h)
    return dict(sums=S, params=P, stats=[follows, w * h - follows, 0, 0, S[0], fitted])


def corners(w, h):
    """the distinct corners of a w x h image as (xs, ys) in raster order"""
    pts = sorted({(y, x) for y in (0, h - 1) for x in (0, w - 1)})
    return np.array([p[1] for p in pts]), np.array([p[0] for p in pts])


def corner_mask(w, h):
    """(h, w) uint8: 1 everywhere but 0 on the corners"""
    m = np.ones((h, w), np.uint8)
    xs, ys = corners(w, h)
    m[ys, xs] = 0
    return m


def motion_corners_expected(ux, vy, model, iters=3, thresh=1.0):
    """fit_motion(flow, corner_mask, model, iters, thresh): motion_ref.fit restated on the list of the only admissible pixels"""
    w, h = len(ux), len(vy)
    xs, ys = corners(w, h)
    Xf, Yf = (2 * xs - (w - 1)).astype(f32), (2 * ys - (h - 1)).astype(f32)
    t2 = f32(thresh) * f32(thresh)

    def follows(P):
        k = M.coef(P, w, h)
        du, dv = ux[xs] - ((k[0] * Xf + k[1] * Yf) + k[2]), vy[ys] - ((k[3] * Xf + k[4] * Yf) + k[5])
        return du * du + dv * dv <= t2

    P, fitted, S = [0.0] * 6, 1, None
    for r in range(iters + 1):
        keep = np.ones(len(xs), bool) if r == 0 else follows(P)
        S = _listed_sums(ux, vy, (xs[keep], ys[keep]))
        P, fitted = _fit_from_sums(S, model, w, h, P, fitted)
    ok = int(follows(P).sum())
    return dict(sums=S, params=P, stats=[ok, len(xs) - ok, w * h - len(xs), 0, S[0], fitted])


def layers_expected(ux, vy, model, rounds, thresh):
    """motion_layers(flow, None, layers=1, model, iters=0, rounds, thresh) of the separable flow: dict(sums (1, 12), params (1, 6),
    records (1, 8), stats (4,)) -- layers_ref.layers with K = 1 and no mask, its pixel sets kept as `all` or as a list"""
    w, h = len(ux), len(vy)
    S = separable_sums(ux, vy)
    P, fitted = _fit_from_sums(S, model, w, h, [0.0] * 6, 1)
    live, in_fit = fitted, S[0]
    empty = (np.zeros(0, np.int64), np.zeros(0, np.int64))
    for _ in range(rounds):
        if not live:
            break
        sel = within_set(ux, vy, P, thresh)
        S = separable_sums(ux, vy) if sel is None else _listed_sums(ux, vy, sel)
        in_fit = S[0]
        P, fitted = _fit_from_sums(S, model, w, h, P, fitted)
    sel = within_set(ux, vy, P, thresh) if live else empty
    L = separable_sums(ux, vy) if sel is None else _listed_sums(ux, vy, sel)
    records = [L[0], in_fit, live, fitted, -1, L[1], L[2], L[6]]
    return dict(sums=[S], params=[P], records=[records], stats=[w * h - L[0], 0, 0, live])


# ---- components -------------------------------------------------------------------------------------------------------------------
VALUE_U, VALUE_V = 4096.0, -4096.0                    # the values of every pixel of the component maps: U = 2^20, V = -2^20
PATTERNS = ("all", "rows", "columns")


def component_map(pattern, w, h):
    """(h, w) uint8 code map, foreground code 1: everything, the even rows, or the even columns"""
    m = np.zeros((h, w), np.uint8)
    if pattern == "all":
        m[:] = 1
    elif pattern == "rows":
        m[0::2] = 1
    else:
        m[:, 0::2] = 1
    return m


def components_expected(pattern, w, h, max_objects):
    """label_components of component_map with values (VALUE_U, VALUE_V) everywhere, min_area 1, either connectivity (a background
    line between two stripes separates them for both): dict(objects (max_objects, 11) int64, stats (4 ints), label_of_row /
    label_of_column: labels and ids follow from them).  Every field is a closed form of the stripe's index k."""
    U, V = int(VALUE_U * 256), int(VALUE_V * 256)
    if pattern == "all":
        rows = [[0, w * h, 0, 0, w - 1, h - 1, h * (w * (w - 1) // 2), w * (h * (h - 1) // 2), w * h, U * w * h, V * w * h]]
    elif pattern == "rows":
        rows = [[2 * k * w, w, 0, 2 * k, w - 1, 2 * k, w * (w - 1) // 2, 2 * k * w, w, U * w, V * w] for k in range((h + 1) // 2)]
    else:
        rows = [[2 * k, h, 2 * k, 0, 2 * k, h - 1, 2 * k * h, h * (h - 1) // 2, h, U * h, V * h] for k in range((w + 1) // 2)]
    objects = np.zeros((max_objects, 11), np.int64)
    written = min(len(rows), max_objects)
    if written:
        objects[:written] = np.array(rows[:written], np.int64)
    return dict(objects=objects, stats=[sum(r[1] for r in rows), len(rows), len(rows), written])


def component_labels(pattern, w, h, max_objects):
    """(labels, ids) as int64 profiles that broadcast to (h, w): (h, 1) for rows, (1, w) for columns, (1, 1) for all"""
    if pattern == "all":
        return np.zeros((1, 1), np.int64), np.zeros((1, 1), np.int64)
    if pattern == "rows":
        y = np.arange(h, dtype=np.int64)[:, None]
        return np.where(y % 2 == 0, y * w, -1), np.where((y % 2 == 0) & (y // 2 < max_objects), y // 2, -1)
    x = np.arange(w, dtype=np.int64)[None, :]
    return np.where(x % 2 == 0, x, -1), np.where((x % 2 == 0) & (x // 2 < max_objects), x // 2, -1)


# ---- object votes -----------------------------------------------------------------------------------------------------------------
def votes_expected(w, h, u, v, masked, ka, kb):
    """object_overlap of ids that are 0 everywhere in both frames, one vector (u, v) at every pixel, a mask that is 0 or 1
    everywhere: (votes (ka, kb) int32, sent (ka, 4) int64).  A vector beyond +-4096 is inadmissible whatever it points at."""
    votes, sent = np.zeros((ka, kb), np.int32), np.zeros((ka, 4), np.int64)
    n = w * h
    if masked or not (np.isfinite(u) and np.isfinite(v)) or abs(u) > 4096 or abs(v) > 4096:
        sent[0, 3] = n
        return votes, sent
    ru, rv = int(np.rint(f32(u))), int(np.rint(f32(v)))
    inside = max(0, w - abs(ru)) * max(0, h - abs(rv))
    votes[0, 0] = inside
    sent[0, 0], sent[0, 2] = inside, n - inside
    return votes, sent


# ---- morphology -------------------------------------------------------------------------------------------------------------------
MORPH_OPS = ("erode", "dilate", "open", "close")


def pinhole_map(w, h):
    """(h, w) uint8: set everywhere but one clear byte in the last corner"""
    m = np.ones((h, w), np.uint8)
    m[h - 1, w - 1] = 0
    return m


def quarter_disc(r, w, h):
    """the pixels of the frame within the disc of radius r around the last corner"""
    return sum(1 for dy in range(0, min(r, h - 1) + 1) for dx in range(0, min(r, w - 1) + 1) if dx * dx + dy * dy <= r * r)


def pinhole_expected(w, h, op, r):
    """the stats (before, after, added, removed) of morphology(pinhole_map, op, r), r >= 1, for a frame of more than 2r rows and
    columns (or of one pixel).  The erosion clears the quarter disc around the hole; the dilation fills the hole; the opening
    restores all of the quarter disc but the hole itself (every other pixel lies in a disc that misses the hole and fits the
    frame, whose border does not erode); the closing fills the hole and then erodes a full map."""
    n = w * h
    assert r >= 1 and (n == 1 or min(w, h) > 2 * r)
    if n == 1:
        return [0, 0, 0, 0]
    clear = {"erode": quarter_disc(r, w, h), "dilate": 0, "open": 1, "close": 0}[op]
    after = n - clear
    return [n - 1, after, max(0, after - (n - 1)), max(0, (n - 1) - after)]


# ---- thin frames: the largest dimension on one axis ---------------------------------------------------------------------------------
THIN = ((16384, 1), (1, 16384), (16384, 3), (3, 16384))                  # (w, h)
SPECIALS = np.array([[np.nan, 0], [np.inf, 1], [1, -np.inf], [5000, 0], [0, -5000], [4096.5, 0], [3e38, 3e38], [-1e30, 2]], f32)


def edge_quads(w, h):
    """the flat pixel indices of the first and the last quad of the first row and of the last row, and of the first and the last
    quad of the image (on a frame narrower than four pixels a thread's quad spans rows)"""
    q = min(4, w)
    idx = []
    for y in sorted({0, h - 1}):
        idx += [y * w + x for x in range(q)] + [y * w + x for x in range(w - q, w)]
    idx += list(range(min(4, w * h))) + list(range(max(0, w * h - 4), w * h))
    return sorted(set(idx))


def edge_specials(flow, shift=0):
    """a copy of flow (n, h, w, 2) with non-finite and out-of-range vectors (SPECIALS, in another order per image) in the pixels of
    edge_quads"""
    f = np.array(flow, f32, copy=True)
    n, h, w = f.shape[:3]
    idx = np.array(edge_quads(w, h))
    for i in range(n):
        f[i].reshape(h * w, 2)[idx] = SPECIALS[(np.arange(len(idx)) + 3 * i + shift) % len(SPECIALS)]
    return f


def thin_flow(w, h, n, seed, scale=3.0, specials=True):
    """n different flows (n, h, w, 2) of a few pixels, quarter-pixel values on the even columns and rows, with edge_specials"""
    rng = np.random.default_rng(seed)
    f = (rng.standard_normal((n, h, w, 2)) * scale).astype(f32)
    f[:, ::2, ::2] = np.round(f[:, ::2, ::2] * 4) / 4
    if min(w, h) == 1:                                       # one line: a vector with a component across it leaves the frame,
        across = f[..., 1 if h == 1 else 0].reshape(n, -1)   # so four of five have none
        across[:, np.arange(w * h) % 5 != 2] = 0
    return edge_specials(f, seed) if specials else f


def thin_images(w, h, n, noc, u8, seed):
    """n different images (n, h, w) or (n, h, w, 3): a smooth texture along the long axis plus noise, uint8 or f32 with fractions"""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    t = (xs + ys) / 7.0
    base = np.stack([128 + 70 * np.sin(t + i) + 30 * np.cos(t / 3.7 - i) for i in range(n)])
    if noc == 3:
        base = np.stack([base, 255 - base, base[:, ::-1, ::-1]], -1)
    a = np.clip(base + rng.normal(0, 4.0, base.shape), 0, 255)
    return np.rint(a).astype(np.uint8) if u8 else a.astype(f32)


def thin_mask(w, h, n, seed):
    """masks in fb_check's alphabet with a byte above it, a non-zero byte in the very last pixel of image 0 and a zero one in image 1"""
    m = np.random.default_rng(seed).choice(np.array([0] * 10 + [1, 2, 3, 200], np.uint8), (n, h, w))
    m[0, h - 1, w - 1], m[(n - 1), h - 1, w - 1] = 3, 0
    return m


def thin_runs(w, h, n=2):
    """code maps (n, h, w) uint8 (foreground 1) whose lines along the long axis hold three kinds of run: one that crosses every edge
    of the 64-pixel tiles, one of length 1, one that ends in the last column (row); on a frame of three lines the middle line holds
    single pixels that join the outer lines, and the third line is one run from pixel 3 to the end.  Image k starts its long run at k."""
    long_axis = max(w, h)
    m = np.zeros((n, min(w, h), long_axis), np.uint8)
    for k in range(n):
        m[k, 0, k:long_axis - 58 + k] = 1                    # crosses the edges at 64, 128, .., long_axis - 64
        m[k, 0, long_axis - 55 + k] = 1                      # a single pixel
        m[k, 0, long_axis - 50 + 2 * k:] = 1                 # ends in the last column
        if m.shape[1] == 3:
            m[k, 1, 7 + k::997] = 1
            m[k, 2, 3:] = 1
            m[k, 2, 100 + k] = 0
    return m if w >= h else np.ascontiguousarray(m.transpose(0, 2, 1))
