"""The numpy restatement of block motion vectors from a dense flow (include/fotg.h fotg_block_motion), written from the definition
and not from the kernel.  Everything is integer arithmetic, so the GPU has to return these bytes.

Per pixel: known = |u| <= 4096 and |v| <= 4096 (false for a NaN), Q = rint(4 flow) in quarter pixels (to nearest even), admissible =
known and (no mask or mask == 0).  Per B x B block of the grid ceil(w / B) x ceil(h / B), clipped to the frame: the candidates 0 the
zero vector, 1 the rounded mean of Q over the block's admissible pixels, 2 Q of the block's centre pixel, 3 .. 6 the means of the four
quadrants; the winner is the lowest SAD of the quarter-pel bilinear prediction from ref, the lowest index among equals; then `refine`
steps of (4, 2, 1) quarter pixels over the eight neighbours."""
import numpy as np

NEIGHBOURS = ((-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1))
QMAX = 16384
NSTAT = 11


def quantise(flow, mask=None):
    """flow (h, w, 2) f32 -> (Q int64 (h, w, 2), admissible bool (h, w))"""
    with np.errstate(invalid="ignore"):
        known = (np.abs(flow[..., 0]) <= np.float32(4096)) & (np.abs(flow[..., 1]) <= np.float32(4096))
    safe = np.where(known[..., None], flow, np.float32(0)).astype(np.float32)
    Q = np.rint(safe * np.float32(4)).astype(np.int64)                  # np.rint rounds to nearest even
    adm = known if mask is None else known & (mask == 0)
    return Q, adm


def predict(ref, x0, x1, y0, y1, mx, my):
    """the prediction of the pixels [y0, y1) x [x0, x1) by (mx, my): int64 (y1 - y0, x1 - x0, c).  ref: int64 (h, w, c)"""
    h, w = ref.shape[:2]
    ix = 4 * np.arange(x0, x1, dtype=np.int64) + mx
    iy = 4 * np.arange(y0, y1, dtype=np.int64) + my
    X0, fx = ix >> 2, (ix & 3)[None, :, None]
    Y0, fy = iy >> 2, (iy & 3)[:, None, None]
    xa, xb = np.clip(X0, 0, w - 1), np.clip(X0 + 1, 0, w - 1)
    ya, yb = np.clip(Y0, 0, h - 1), np.clip(Y0 + 1, 0, h - 1)
    a, b = ref[ya][:, xa], ref[ya][:, xb]
    c, d = ref[yb][:, xa], ref[yb][:, xb]
    return ((4 - fx) * (4 - fy) * a + fx * (4 - fy) * b + (4 - fx) * fy * c + fx * fy * d + 8) >> 4


def mean_vector(Q, adm):
    """floor((2 S + m) / (2 m)) per component over the admissible pixels, or None when there is none"""
    m = int(adm.sum())
    if m == 0:
        return None
    return tuple(int((2 * int(Q[..., k][adm].sum()) + m) // (2 * m)) for k in range(2))     # Python's // is the floor division


def block_motion_one(cur, ref, flow, mask=None, block=16, refine=2):
    """cur, ref uint8 (h, w[, c]); flow f32 (h, w, 2); mask None or uint8 (h, w) -> mv int16 (bh, bw, 2), cost uint32 (bh, bw, 2),
    kind uint8 (bh, bw), pred uint8 like cur, stats int64 (11,)"""
    assert block in (8, 16, 32) and refine in (0, 1, 2, 3) and cur.dtype == np.uint8 and ref.dtype == np.uint8
    shape = cur.shape
    h, w = shape[:2]
    c3 = cur.reshape(h, w, -1).astype(np.int64)
    r3 = ref.reshape(h, w, -1).astype(np.int64)
    Q, adm = quantise(flow, mask)
    B, H = block, block // 2
    bw, bh = -(-w // B), -(-h // B)
    mv = np.zeros((bh, bw, 2), np.int16)
    cost = np.zeros((bh, bw, 2), np.uint32)
    kind = np.zeros((bh, bw), np.uint8)
    pred = np.zeros((h, w, c3.shape[2]), np.uint8)
    stats = np.zeros(NSTAT, np.int64)
    for by in range(bh):
        for bx in range(bw):
            x0, x1, y0, y1 = bx * B, min(bx * B + B, w), by * B, min(by * B + B, h)
            cb = c3[y0:y1, x0:x1]
            sad = lambda m: int(np.abs(cb - predict(r3, x0, x1, y0, y1, m[0], m[1])).sum())
            cands = [(0, 0), mean_vector(Q[y0:y1, x0:x1], adm[y0:y1, x0:x1])]
            cx, cy = min(x0 + H, w - 1), min(y0 + H, h - 1)
            cands.append((int(Q[cy, cx, 0]), int(Q[cy, cx, 1])) if adm[cy, cx] else None)
            for qy in (0, 1):
                for qx in (0, 1):
                    xs = slice(min(x0 + qx * H, w), min(x0 + qx * H + H, w))
                    ys = slice(min(y0 + qy * H, h), min(y0 + qy * H + H, h))
                    cands.append(mean_vector(Q[ys, xs], adm[ys, xs]))
            best, bs, bk = None, None, 0
            for k, m in enumerate(cands):
                if m is None:
                    continue
                s = sad(m)
                if best is None or s < bs:
                    best, bs, bk = m, s, k
            zero = sad((0, 0))
            moved = False
            for step in (4, 2, 1)[3 - refine:]:
                nb, ns = None, bs
                for dx, dy in NEIGHBOURS:
                    m = (best[0] + step * dx, best[1] + step * dy)
                    if abs(m[0]) > QMAX or abs(m[1]) > QMAX:
                        continue
                    s = sad(m)
                    if s < ns:
                        nb, ns = m, s
                if nb is not None:
                    best, bs, moved = nb, ns, True
            p = predict(r3, x0, x1, y0, y1, best[0], best[1])
            pred[y0:y1, x0:x1] = p
            mv[by, bx] = best
            cost[by, bx] = (bs, zero)
            kind[by, bx] = bk | (8 if moved else 0)
            stats[0] += bs
            stats[1] += zero
            stats[2] += int(((cb - p) ** 2).sum())
            stats[3] += moved
            stats[4 + bk] += 1
    return mv, cost, kind, pred.reshape(shape), stats


def block_motion(cur, ref, flow, mask=None, block=16, refine=2):
    """the batch: every output stacked over the images"""
    res = [block_motion_one(cur[i], ref[i], flow[i], None if mask is None else mask[i], block, refine) for i in range(len(cur))]
    return tuple(np.stack([r[j] for r in res]) for j in range(5))


def psnr(sse, count):
    return float("inf") if sse == 0 else 10.0 * np.log10(255.0 ** 2 * count / float(sse))


ODD = np.array([np.nan, np.inf, -np.inf, 2e9, -5000.0, 4096.0, -4096.0, 4096.5], np.float32)


def scene(h, w, noc, seed, n=3):
    """n frame pairs of different content for the GPU comparison: a smooth texture plus noise, moved piecewise by two sub-pixel
    motions with a still patch; the flow is the true motion plus noise of sigma 0.35 px with 2 % of its entries replaced by the
    entries of ODD; a mask from {0 x 10, 1, 2, 3, 200}.  -> cur, ref uint8 (n, h, w[, 3]), flow f32 (n, h, w, 2), mask uint8"""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)

    def tex(x, y, i):
        t = 120 + 50 * np.sin(x / 2.3 + i) * np.cos(y / 3.1) + 40 * np.sin((x + 2 * y) / 5.7 + 0.5 * i) + 25 * np.cos(x * y / 37.0)
        return t

    cur, ref, flow = [], [], []
    for i in range(n):
        mo = np.zeros((h, w, 2))
        mo[:] = (1.75 + i, -0.5)
        mo[:, w // 2:] = (-2.25, 1.25 + 0.5 * i)
        mo[h // 3:h // 3 + max(1, h // 4), w // 4:w // 4 + max(1, w // 5)] = 0.0          # the still patch
        r = tex(xs, ys, i)
        c = tex(xs + mo[..., 0], ys + mo[..., 1], i)                                      # cur(x) = ref(x + flow(x))
        if noc == 3:
            r = np.stack([r, 255 - r, r[::-1]], -1)
            c = np.stack([c, 255 - c, tex(xs + mo[..., 0], (h - 1 - ys) - mo[..., 1], i)], -1)
        r = r + rng.normal(0, 2.0, r.shape)
        c = c + rng.normal(0, 2.0, c.shape)
        f = (mo + rng.normal(0, 0.35, mo.shape)).astype(np.float32)
        flat = f.reshape(-1)
        idx = np.flatnonzero(rng.random(flat.size) < 0.02)
        flat[idx] = ODD[rng.integers(0, ODD.size, idx.size)]
        cur.append(np.rint(np.clip(c, 0, 255)).astype(np.uint8))
        ref.append(np.rint(np.clip(r, 0, 255)).astype(np.uint8))
        flow.append(f)
    mask = rng.choice(np.array([0] * 10 + [1, 2, 3, 200], np.uint8), (n, h, w))
    return np.stack(cur), np.stack(ref), np.stack(flow), mask
