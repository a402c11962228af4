"""numpy float32 restatement of the forward-backward consistency check (csrc/fbcheck.hip.h, include/fotg.h fotg_fb_check): every
operation separately rounded to f32, in the kernel's order, so the GPU's masks equal these byte for byte.
Codes: 0 consistent, 1 occluded / inconsistent, 2 the vector leaves the frame, 3 unknown (non-finite vector)."""
import numpy as np

f32 = np.float32


def fb_code(F, B, alpha1=0.01, alpha2=0.5):
    """F, B: (h, w, 2) float32 -> (h, w) uint8 codes of F checked against B"""
    F, B = np.asarray(F, f32), np.asarray(B, f32)
    h, w = F.shape[:2]
    a1, a2, one = f32(alpha1), f32(alpha2), f32(1)
    u, v = F[..., 0], F[..., 1]
    ys, xs = np.mgrid[0:h, 0:w]
    with np.errstate(all="ignore"):
        known = np.isfinite(u) & np.isfinite(v)
        X, Y = xs.astype(f32) + u, ys.astype(f32) + v
        inside = known & (X >= f32(0)) & (X <= f32(w - 1)) & (Y >= f32(0)) & (Y <= f32(h - 1))
        Xs, Ys = np.where(inside, X, f32(0)), np.where(inside, Y, f32(0))
        x0 = np.minimum(np.floor(Xs).astype(np.int64), w - 1)
        y0 = np.minimum(np.floor(Ys).astype(np.int64), h - 1)
        x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
        ax, ay = Xs - x0.astype(f32), Ys - y0.astype(f32)
        b = []
        for c in range(2):
            r0 = B[y0, x0, c] * (one - ax) + B[y0, x1, c] * ax
            r1 = B[y1, x0, c] * (one - ax) + B[y1, x1, c] * ax
            b.append(r0 * (one - ay) + r1 * ay)
        bu, bv = b
        du, dv = u + bu, v + bv
        lhs = du * du + dv * dv
        rhs = a1 * ((u * u + v * v) + (bu * bu + bv * bv)) + a2
    code = np.where(lhs < rhs, 0, 1).astype(np.uint8)
    code[~inside] = 2
    code[~known] = 3
    return code


def fb_check(F, B, alpha1=0.01, alpha2=0.5):
    """both directions of a pair or a batch: (mask, mask_bw) -- F against B over frame 0, B against F over frame 1"""
    F, B = np.asarray(F, f32), np.asarray(B, f32)
    if F.ndim == 3:
        return fb_code(F, B, alpha1, alpha2), fb_code(B, F, alpha1, alpha2)
    return (np.stack([fb_code(f, b, alpha1, alpha2) for f, b in zip(F, B)]),
            np.stack([fb_code(b, f, alpha1, alpha2) for f, b in zip(F, B)]))


def counts(mask, mask_bw):
    """n x 2 x 4: per image and direction the number of pixels of each code (fotg_fb_check's counts)"""
    m, mb = np.asarray(mask), np.asarray(mask_bw)
    if m.ndim == 2:
        m, mb = m[None], mb[None]
    return np.stack([np.stack([np.bincount(a.ravel(), minlength=4)[:4], np.bincount(b.ravel(), minlength=4)[:4]])
                     for a, b in zip(m, mb)]).astype(np.int64)
