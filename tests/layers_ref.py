"""Motion layers restated in numpy, operation for operation as include/fotg.h and flowonthego_amd/csrc/layers.hip.h define them,
on the pieces of tests/motion_ref.py (the fixed-point flow, the twelve exact int64 sums, the f64 solve in its written order, the
f32 prediction): the seeding layer by layer, the refinement rounds and the final pass."""
import numpy as np

import motion_ref as M

f32 = np.float32
TILE = 32
UNASSIGNED, MASKED, UNKNOWN = 253, 254, 255


def _residual(flow, P):
    """(du, dv, r) against parameters P, all f32: r = du du + dv dv"""
    h, w = flow.shape[:2]
    with np.errstate(over="ignore", invalid="ignore"):
        res = flow - M.predict(P, w, h)
        return res[..., 0], res[..., 1], res[..., 0] * res[..., 0] + res[..., 1] * res[..., 1]


def _within(r, t2):
    with np.errstate(invalid="ignore"):
        return r <= t2


def assign(flow, adm, P, live, t2):
    """the layer of every pixel: (best (h, w) int, -1 with no live layer; du, dv against it -- the flow itself with no live layer;
    within).  The first live layer is taken as it comes, a later one only where its r is strictly smaller than the smallest so far
    (which starts at +infinity): a NaN never displaces a value."""
    h, w = flow.shape[:2]
    best = np.full((h, w), -1, np.int64)
    rb = np.full((h, w), np.inf, f32)
    dub, dvb = flow[..., 0].copy(), flow[..., 1].copy()
    for j in range(len(P)):
        if not live[j]:
            continue
        du, dv, r = _residual(flow, P[j])
        with np.errstate(invalid="ignore"):
            less = r < rb
        take = (best < 0) | less
        best = np.where(take, j, best)
        dub, dvb = np.where(take, du, dub), np.where(take, dv, dvb)
        rb = np.where(less, r, rb)
    with np.errstate(over="ignore", invalid="ignore"):
        within = adm & (best >= 0) & _within(dub * dub + dvb * dvb, t2)
    return best, dub, dvb, within


def layers(flow, mask=None, layers=3, model=2, iters=3, rounds=3, thresh=1.0, init=None):
    """one image: flow (h, w, 2) f32, mask (h, w) uint8 or None, init (K, 6) f64 or None -> dict(params (K, 6) f64, labels (h, w)
    uint8, residual (h, w, 2) f32, records (K, 8) int64, stats (4,) int64, sums (K, 12) int64)"""
    if isinstance(model, str):
        model = M.MODELS.index(model)
    K = layers
    flow = np.asarray(flow, f32)
    h, w = flow.shape[:2]
    X, Y = M.coords(w, h)
    kn = M.known(flow)
    U, V = M.fixed_point(flow, kn)
    adm = kn if mask is None else kn & (np.asarray(mask) == 0)
    t2 = f32(thresh) * f32(thresh)
    P = [[0.0] * 6 for _ in range(K)]
    live, fitted, seed, in_fit = [0] * K, [0] * K, [-1] * K, [0] * K
    S = [[0] * 12 for _ in range(K)]
    if init is not None:
        P = [[float(v) for v in row] for row in np.asarray(init, np.float64)]
        live, fitted, seed = [1] * K, [1] * K, [-2] * K
    else:
        tx, ty = (w + TILE - 1) // TILE, (h + TILE - 1) // TILE
        for k in range(K):
            cand = adm.copy()
            for j in range(k):
                if live[j]:
                    cand &= ~_within(_residual(flow, P[j])[2], t2)
            if k > 0:
                pad = np.zeros((ty * TILE, tx * TILE), bool)
                pad[:h, :w] = cand
                cnt = pad.reshape(ty, TILE, tx, TILE).sum((1, 3)).reshape(-1)
                t = int(np.argmax(cnt))                      # the first of the largest: the lowest tile index
                if cnt[t] == 0:
                    continue                                 # dead: zeros, seed -1
                seed[k] = t
                sel = np.zeros((h, w), bool)
                y0, x0 = (t // tx) * TILE, (t % tx) * TILE
                sel[y0:y0 + TILE, x0:x0 + TILE] = cand[y0:y0 + TILE, x0:x0 + TILE]
                P[k] = M.to_pixel_frame(M.solve(M.sums(X, Y, U, V, sel), 0), w, h)
            fitted[k] = 1
            for r in range(iters + 1):
                sel = cand if k == 0 and r == 0 else cand & _within(_residual(flow, P[k])[2], t2)
                S[k] = M.sums(X, Y, U, V, sel)
                in_fit[k] = S[k][0]
                c = M.solve(S[k], model)
                if c is None:
                    fitted[k] = 0
                else:
                    P[k] = M.to_pixel_frame(c, w, h)
            live[k] = fitted[k]
    for _ in range(rounds):
        best, _, _, within = assign(flow, adm, P, live, t2)
        for k in range(K):
            if not live[k]:
                continue
            S[k] = M.sums(X, Y, U, V, within & (best == k))
            in_fit[k] = S[k][0]
            c = M.solve(S[k], model)
            if c is None:
                fitted[k] = 0
            else:
                P[k] = M.to_pixel_frame(c, w, h)
    best, dub, dvb, within = assign(flow, adm, P, live, t2)
    labels = np.where(~kn, UNKNOWN, np.where(~adm, MASKED, np.where(within, best, UNASSIGNED))).astype(np.uint8)
    records = np.zeros((K, 8), np.int64)
    for k in range(K):
        m = labels == k
        records[k] = [int(m.sum()), in_fit[k], live[k], fitted[k], seed[k], int(X[m].sum()), int(Y[m].sum()), int(U[m].sum())]
    stats = np.array([(labels == UNASSIGNED).sum(), (labels == MASKED).sum(), (labels == UNKNOWN).sum(), sum(live)], np.int64)
    return dict(params=np.array(P, np.float64).reshape(K, 6), labels=labels, residual=np.stack([dub, dvb], -1).astype(f32),
                records=records, stats=stats, sums=np.array(S, np.int64).reshape(K, 12))


def layers_batch(flow, mask=None, init=None, **kw):
    """flow (n, h, w, 2): the dict of layers() with every entry stacked"""
    outs = [layers(flow[i], None if mask is None else mask[i], init=None if init is None else init[i], **kw) for i in range(len(flow))]
    return {k: np.stack([o[k] for o in outs]) for k in outs[0]}


# ---- the scene of the tests -------------------------------------------------------------------------------------------------------
P_BACKGROUND = (0.004, -0.011, 1.75, 0.009, 0.006, -2.5)
P_A = (0.0, 0.0, 6.5, 0.0, 0.0, -4.0)
P_B = (0.03, -0.02, -7.0, 0.02, 0.03, 3.0)


def three_motions(w, h, seed, noise=0.2):
    """the background of motion_ref.make_scene, object A (rows h/8 .. h/8 + h/3, columns w/10 .. w/10 + w/4) moving by (6.5, -4),
    object B (rows h/2 .. h/2 + h/3, columns w/2 .. w/2 + w/3) moving by an affine motion of its own; Gaussian noise on both
    components, then f32.  Returns (flow (h, w, 2) f32, truth (h, w) int: 0 background, 1 A, 2 B, the three motions (3, 6))."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    truth = np.zeros((h, w), np.int64)
    truth[h // 8:h // 8 + h // 3, w // 10:w // 10 + w // 4] = 1
    truth[h // 2:h // 2 + h // 3, w // 2:w // 2 + w // 3] = 2
    Ps = np.array([P_BACKGROUND, P_A, P_B])
    flow = np.zeros((h, w, 2))
    for k, P in enumerate(Ps):
        f = np.stack([P[0] * xs + P[1] * ys + P[2], P[3] * xs + P[4] * ys + P[5]], -1)
        flow[truth == k] = f[truth == k]
    flow = flow + noise * rng.standard_normal((h, w, 2))
    return flow.astype(f32), truth, Ps
