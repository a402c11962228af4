"""numpy float32 restatement of the frame interpolation (csrc/interp.hip.h, include/fotg.h fotg_interp): every operation separately
rounded to f32, in the kernels' order, so the GPU's dst, code and counts equal these byte for byte.  The tap arithmetic and the
in-frame test are tests/warp_ref.py's (the restatement of fotg_warp), called, not copied.

Code byte: origin (0 forward vector, 1 backward vector, 2 hole) + 4 (only frame 0 used) + 8 (only frame 1 used).
Statistics: pixels of origin 0, 1, 2; one-sided pixels; sum |ref - value|; sum |ref - plain blend|."""
import math

import numpy as np

import fbcheck_ref as FB
import warp_ref as W

f32 = np.float32
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
QMAX = 2 ** 24 - 1


def _taps(S, flow):
    """fotg_warp's unrounded value and in-frame test of the f32 image S (h, w, c) along flow (finite)"""
    dst, code, _ = W.warp(S, flow)
    return dst.reshape(S.shape), code == 0


def keys(Isrc, Idst, V, m, s):
    """the key plane (h, w) uint64 of one direction: Isrc, Idst (h, w, c) f32; V (h, w, 2); m (h, w) uint8; s f32"""
    h, w, noc = Isrc.shape
    s = f32(s)
    u, v = V[..., 0], V[..., 1]
    ys, xs = np.mgrid[0:h, 0:w]
    with np.errstate(all="ignore"):
        ok = np.isfinite(u) & np.isfinite(v) & (m <= 1)
        Vz = np.where(ok[..., None], V, f32(0))
        val, _ = _taps(Idst, Vz)
        e = np.abs(Isrc[..., 0] - val[..., 0])
        for c in range(1, noc):
            e = e + np.abs(Isrc[..., c] - val[..., c])
        assert e.dtype == f32
        e256 = e * f32(256)
        q = np.where(e256 < f32(QMAX), np.floor(np.where(e256 < f32(QMAX), e256, f32(0))), f32(QMAX)).astype(np.uint64)
        tx = np.floor((xs.astype(f32) + s * Vz[..., 0]) + f32(0.5))
        ty = np.floor((ys.astype(f32) + s * Vz[..., 1]) + f32(0.5))
        assert tx.dtype == f32
        ok &= (tx >= f32(0)) & (tx <= f32(w - 1)) & (ty >= f32(0)) & (ty <= f32(h - 1))
    key = (m.astype(np.uint64) << np.uint64(56)) | (q << np.uint64(32)) | (ys * w + xs).astype(np.uint64)
    K = np.full(h * w, EMPTY, np.uint64)
    tgt = (ty[ok].astype(np.int64) * w + tx[ok].astype(np.int64))
    np.minimum.at(K, tgt, key[ok])
    return K.reshape(h, w)


def _near(m, xx, yy):
    """m at the nearest in-frame pixel of (xx, yy)"""
    h, w = m.shape
    with np.errstate(all="ignore"):
        nx = np.clip(np.clip(np.floor(xx + f32(0.5)), f32(-2), f32(w)).astype(np.int64), 0, w - 1)
        ny = np.clip(np.clip(np.floor(yy + f32(0.5)), f32(-2), f32(h)).astype(np.int64), 0, h - 1)
    return m[ny, nx]


def interp(I0, I1, F, B, t, mF=None, mB=None, ref=None, alpha1=0.01, alpha2=0.5, terms=False, planes=False):
    """I0, I1: (h, w) or (h, w, c) float32 or uint8; F, B: (h, w, 2) float32; mF, mB: (h, w) uint8 or None (then fb_check's);
    0 < t < 1; ref: like I0 or None.  Returns dst (I0's shape and dtype), code (h, w) uint8, stats (6,) float64 [sums added with
    math.fsum]; with terms=True also the two arrays of residual terms; with planes=True also the two key planes."""
    I0 = np.asarray(I0)
    u8 = I0.dtype == np.uint8
    S0 = I0.astype(f32).reshape(I0.shape[0], I0.shape[1], -1)
    S1 = np.asarray(I1).astype(f32).reshape(S0.shape)
    h, w, noc = S0.shape
    F, B = np.asarray(F, f32), np.asarray(B, f32)
    if mF is None:
        mF, mB = FB.fb_code(F, B, alpha1, alpha2), FB.fb_code(B, F, alpha1, alpha2)
    mF, mB = np.asarray(mF, np.uint8), np.asarray(mB, np.uint8)
    t = f32(t)
    assert f32(0) < t < f32(1)
    t1 = f32(1) - t
    KF, KB = keys(S0, S1, F, mF, t), keys(S1, S0, B, mB, t1)
    hasF, hasB = KF != EMPTY, (KF == EMPTY) & (KB != EMPTY)
    origin = np.where(hasF, 0, np.where(hasB, 1, 2)).astype(np.uint8)
    V = np.zeros((h, w, 2), f32)
    lo = np.uint64(0xFFFFFFFF)
    V[hasF] = F.reshape(-1, 2)[(KF[hasF] & lo).astype(np.int64)]
    V[hasB] = -B.reshape(-1, 2)[(KB[hasB] & lo).astype(np.int64)]
    ys, xs = np.mgrid[0:h, 0:w]
    xf, yf = xs.astype(f32), ys.astype(f32)
    d0, d1 = -(t * V), t1 * V                      # x + (-(t Vu)) == x - t Vu, bit for bit
    assert d0.dtype == f32 and d1.dtype == f32
    v0, use0 = _taps(S0, d0)
    v1, use1 = _taps(S1, d1)
    o0 = _near(mF, xf + d0[..., 0], yf + d0[..., 1]) != 0
    o1 = _near(mB, xf + d1[..., 0], yf + d1[..., 1]) != 0
    known = origin != 2
    use0 = use0 & ~(known & o1 & ~o0)
    use1 = use1 & ~(known & o0 & ~o1)
    only0, only1 = use0 & ~use1, use1 & ~use0
    value = np.where(only0[..., None], v0, np.where(only1[..., None], v1, t1 * v0 + t * v1))
    assert value.dtype == f32
    code = (origin + 4 * only0 + 8 * only1).astype(np.uint8)
    dst = (W.to_u8(value) if u8 else value).reshape(I0.shape)
    stats = np.zeros(6, np.float64)
    stats[:3] = np.bincount(origin.ravel(), minlength=3)[:3]
    stats[3] = (only0 | only1).sum()
    tv = tb = np.zeros(0, np.float64)
    if ref is not None:
        R = np.asarray(ref).astype(f32).reshape(S0.shape)
        tv = np.abs(R - value).astype(np.float64).ravel()
        tb = np.abs(R - (t1 * S0 + t * S1)).astype(np.float64).ravel()
        stats[4], stats[5] = math.fsum(tv), math.fsum(tb)
    out = (dst, code, stats)
    if terms:
        out += (tv, tb)
    if planes:
        out += (KF, KB)
    return out


def interp_batch(I0, I1, F, B, t, mF=None, mB=None, ref=None):
    """a batch: leading dimension n on every argument -> dst, code (n, h, w), stats (n, 6)"""
    outs = [interp(I0[k], I1[k], F[k], B[k], t, None if mF is None else mF[k], None if mB is None else mB[k],
                   None if ref is None else ref[k]) for k in range(len(I0))]
    return np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs]), np.stack([o[2] for o in outs])


def psnr(a, b):
    """PSNR in dB of two 8-bit-range images"""
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    return 10.0 * math.log10(255.0 ** 2 / float(np.mean(d * d)))
