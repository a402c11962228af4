"""numpy float32 restatement of flow chaining (csrc/chain.hip.h, include/fotg.h fotg_flow_chain / fotg_track_points): every
operation separately rounded to f32, in the kernel's order, so the GPU's displacements, codes, step counts and trajectories
equal these byte for byte.  Codes: 0 valid to the end, 1 occluded / inconsistent, 2 leaves the frame, 3 unknown (non-finite)."""
import numpy as np

f32 = np.float32


def inside(X, Y, w, h):
    """warp_inside (a NaN is outside)"""
    with np.errstate(invalid="ignore"):
        return (X >= f32(0)) & (X <= f32(w - 1)) & (Y >= f32(0)) & (Y <= f32(h - 1))


def bilerp(F, X, Y):
    """fb_sample: F (h, w, 2), X, Y in-frame f32 arrays -> (u, v), fb_code's taps and lerp order"""
    h, w = F.shape[:2]
    one = f32(1)
    x0 = np.minimum(np.floor(X).astype(np.int64), w - 1)
    y0 = np.minimum(np.floor(Y).astype(np.int64), h - 1)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    ax, ay = X - x0.astype(f32), Y - y0.astype(f32)
    out = []
    with np.errstate(all="ignore"):
        for c in range(2):
            r0 = F[y0, x0, c] * (one - ax) + F[y0, x1, c] * ax
            r1 = F[y1, x0, c] * (one - ax) + F[y1, x1, c] * ax
            out.append(r0 * (one - ay) + r1 * ay)
    return out


def track(pts, flows, flows_bw=None, alpha1=0.01, alpha2=0.5):
    """pts (P, 2) f32 (x, y); flows, flows_bw (T, h, w, 2) f32 of one sequence ->
    traj (T+1, P, 2) f32, code (P,) uint8, steps (P,) int32, disp (P, 2) f32"""
    pts, F = np.asarray(pts, f32), np.asarray(flows, f32)
    B = None if flows_bw is None else np.asarray(flows_bw, f32)
    T, h, w = F.shape[:3]
    a1, a2 = f32(alpha1), f32(alpha2)
    X0, Y0 = pts[:, 0].copy(), pts[:, 1].copy()
    P = X0.size
    Dx, Dy = np.zeros(P, f32), np.zeros(P, f32)
    steps = np.zeros(P, np.int32)
    code = np.zeros(P, np.uint8)
    known = np.isfinite(X0) & np.isfinite(Y0)
    code[known & ~inside(X0, Y0, w, h)] = 2
    code[~known] = 3
    traj = np.empty((T + 1, P, 2), f32)
    traj[0] = pts
    with np.errstate(all="ignore"):
        for k in range(T):
            live = np.flatnonzero(code == 0)
            if live.size:
                x0, y0, dx, dy = X0[live], Y0[live], Dx[live], Dy[live]
                X, Y = x0 + dx, y0 + dy
                u, v = bilerp(F[k], X, Y)
                fin = np.isfinite(u) & np.isfinite(v)
                Ex, Ey = dx + u, dy + v
                Xn, Yn = x0 + Ex, y0 + Ey
                ins = fin & inside(Xn, Yn, w, h)
                c = np.where(fin, np.where(ins, 0, 2), 3).astype(np.uint8)
                if B is not None:
                    bu, bv = bilerp(B[k], np.where(ins, Xn, f32(0)), np.where(ins, Yn, f32(0)))
                    du, dv = u + bu, v + bv
                    lhs = du * du + dv * dv
                    rhs = a1 * ((u * u + v * v) + (bu * bu + bv * bv)) + a2
                    c[ins & ~(lhs < rhs)] = 1
                ok = c == 0
                code[live] = c
                Dx[live[ok]], Dy[live[ok]] = Ex[ok], Ey[ok]
                steps[live[ok]] = k + 1
            traj[k + 1, :, 0], traj[k + 1, :, 1] = X0 + Dx, Y0 + Dy
    return traj, code, steps, np.stack([Dx, Dy], -1)


def chain(flows, flows_bw=None, alpha1=0.01, alpha2=0.5):
    """the dense form: one chain per pixel of frame 0.  flows (T, h, w, 2) -> total (h, w, 2) f32, code (h, w) uint8,
    steps (h, w) int32"""
    F = np.asarray(flows, f32)
    T, h, w = F.shape[:3]
    ys, xs = np.mgrid[0:h, 0:w]
    pts = np.stack([xs.ravel().astype(f32), ys.ravel().astype(f32)], -1)
    _, code, steps, disp = track(pts, F, flows_bw, alpha1, alpha2)
    return disp.reshape(h, w, 2), code.reshape(h, w), steps.reshape(h, w)


def stats(code, steps):
    """the five counters of one sequence: chains ending with code 0, 1, 2, 3 and the sum of steps"""
    c = np.bincount(np.asarray(code).ravel(), minlength=4)[:4]
    return np.array(list(c) + [int(np.asarray(steps, np.int64).sum())], np.uint64)


# ---- the seeded inputs the GPU tests use (tests/test_chain.py asserts that they exercise every code and every step count) --------
SIZES = ((37, 23), (64, 48), (5, 3))          # w x h: w h % 4 != 0 with a ragged tail; whole; smaller than one thread's span
CASES = [(w, h, n_seq, T, bw) for (w, h) in SIZES for n_seq in (1, 2) for T in (1, 2, 5) for bw in (False, True)]


def make_flows(w, h, n_seq, T, seed=0):
    """(F, B), each (n_seq, T, h, w, 2): smooth flows of a few pixels plus a little noise, rows of NaN and inf, a band of 1e30,
    vectors that land exactly on w-1 and h-1; B the negated F (consistent for a smooth flow) on the left two thirds of the frame
    and random on the rest, with a NaN row of its own"""
    rng = np.random.default_rng(1000 * w + 10 * T + n_seq + seed)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    F = np.empty((n_seq, T, h, w, 2), f32)
    B = np.empty_like(F)
    for s in range(n_seq):
        if min(w, h) < 8:
            # a frame of a few pixels: a slow contraction towards the centre, under which every chain survives all T steps, and
            # one bad vector per step k, each at a pixel of its own, that ends the chains near it after exactly k steps
            g = 1.0 + 0.1 * s
            for k in range(T):
                F[s, k] = np.stack([0.12 * g * ((w - 1) / 2 - xs) + 0.01 * rng.standard_normal((h, w)),
                                    0.10 * g * ((h - 1) / 2 - ys) + 0.01 * rng.standard_normal((h, w))], -1)
                B[s, k] = -F[s, k]
            B[s, T - 1, 1, 1] = (1.5, 1.5)                   # inconsistent at the last step
            events = (((0, 0), (np.nan, 0.0)), ((w - 1, 0), (1e30, 0.0)),        # step 0: unknown in one corner, outside in another
                      ((w // 2, h - 1), (0.0, -6.0)),        # step 1: leaves over the top
                      ((0, h - 1), (np.inf, 0.0)),           # step 2
                      ((w - 1, h - 1), (-1e30, 0.0)),        # step 3
                      ((w // 2, 0), (0.0, 30.0)))            # step 4
            for k, ((x, y), vec) in zip((0, 0, 1, 2, 3, 4), events):
                if k < T:
                    F[s, k, y, x] = vec
            # targets exactly on the last column / row; against the small backward vector there they are inconsistent
            F[s, 0, 1, 0] = (f32(w - 1), 0.0)
            F[s, 0, 0, w - 2] = (0.0, f32(h - 1))
            continue
        for k in range(T):
            ang = rng.uniform(0, 2 * np.pi)
            sp = min(w, h) * 0.11 + 0.4                      # a border strip of every depth 1 .. T steps leaves the frame
            u = sp * np.cos(ang) + 0.4 * np.sin(ys / 9.0 + k) + 0.02 * rng.standard_normal((h, w))
            v = sp * np.sin(ang) + 0.4 * np.cos(xs / 11.0 + s) + 0.02 * rng.standard_normal((h, w))
            F[s, k] = np.stack([u, v], -1)
            B[s, k] = -F[s, k]
            cut = (2 * w) // 3
            B[s, k, :, cut:] = rng.standard_normal((h, w - cut, 2)) * 3
            B[s, k, (h // 2 + k) % h, : w // 2] = np.nan
            # non-finite rows and a huge band, at another place in every step so that chains meet them after 0 .. T-1 steps
            F[s, k, (3 * k + 1) % h, w // 3: w // 3 + max(2, w // 4)] = (np.nan, 0.0)
            F[s, k, (5 * k + 2) % h, : max(1, w // 5)] = (1.0, np.inf if k % 2 else -np.inf)
            F[s, k, :, (7 * k + w // 2) % w] = (1e30 if k % 2 else -1e30, 0.5)
        # targets exactly on the last column / row (from integer starts), first step
        F[s, 0, h - 1, ::2, 0] = (f32(w - 1) - xs[h - 1, ::2]).astype(f32)
        F[s, 0, h - 1, ::2, 1] = 0.0
        F[s, 0, ::2, 0, 1] = (f32(h - 1) - ys[::2, 0]).astype(f32)
        F[s, 0, ::2, 0, 0] = 0.0
    return F, B


def make_points(w, h, n_seq, P, seed=0):
    """(n_seq, P, 2): points off the grid, on the last column / row, outside the frame and non-finite"""
    rng = np.random.default_rng(77 + 13 * w + P + seed)
    pts = np.stack([rng.uniform(-2, w + 1, (n_seq, P)), rng.uniform(-2, h + 1, (n_seq, P))], -1).astype(f32)
    special = np.array([[0, 0], [w - 1, h - 1], [w - 1, 0.5], [0.25, h - 1], [np.nan, 1], [1, np.inf], [-np.inf, np.nan],
                        [-0.0, -0.0], [w - 1 + 1e-3, 1], [1e30, 1], [-1e-7, 2]], f32)
    m = min(len(special), P)
    pts[:, :m] = special[:m]
    return pts
