"""CPU tests of the frame interpolation's restatement (tests/interp_ref.py), pinned by facts that do not depend on the code under
test: zero flows, integer translations, sub-half-pixel motion against warp_ref, hand-made 4 x 4 cases (one per rule of the key and
per one-sided rule), and the quality on two triplets of the reference's alley_1 frames with the oracle's flows."""
import math
import os

import numpy as np
import pytest

import fbcheck_ref as FB
import interp_ref as I
import warp_ref as W
from conftest import GOLDEN

f32 = np.float32

# (frames 0, middle, 1) -> (PSNR of the plain blend, PSNR of the restatement's frame at t = 0.5) in dB against the real middle frame,
# with the oracle's op-pt 2 flows and fbcheck_ref's masks, recorded from this restatement on the CPU.  The
# tests ask for half of that gain: the GPU's frame is the restatement's byte for byte, so the threshold only has to catch a broken
# definition.
QUALITY = {(1, 2, 3): (28.2428, 36.8512), (20, 21, 22): (26.1318, 30.7904)}
HOLE_SHARE_MAX = 0.03


def rand_img(rng, h, w, noc=1):
    return rng.integers(0, 256, (h, w) if noc == 1 else (h, w, noc)).astype(f32)


@pytest.mark.parametrize("t", [0.5, 0.25, 0.3, 0.9375])
def test_zero_flows_give_the_plain_blend(t):
    rng = np.random.default_rng(1)
    for noc in (1, 3):
        I0, I1 = rand_img(rng, 13, 17, noc), rand_img(rng, 13, 17, noc)
        Z = np.zeros((13, 17, 2), f32)
        dst, code, st = I.interp(I0, I1, Z, Z, t)
        assert np.array_equal(dst, (f32(1) - f32(t)) * I0 + f32(t) * I1)
        assert (code == 0).all() and np.array_equal(st[:4], [13 * 17, 0, 0, 0])
    d8, _, _ = I.interp(I0.astype(np.uint8), I1.astype(np.uint8), Z, Z, t)
    assert d8.dtype == np.uint8 and np.array_equal(d8, W.to_u8(dst))


@pytest.mark.parametrize("d,t", [((4, 0), 0.5), ((4, -8), 0.25), ((-6, 2), 0.5), ((0, 8), 0.875)])
def test_integer_translation_gives_the_shifted_frame(d, t):
    """I1(x) = I0(x - d), t d integer: the frame at t is I0(x - t d), exactly, wherever all three positions are inside"""
    rng = np.random.default_rng(2)
    h, w = 40, 56
    big = rand_img(rng, h + 32, w + 32)
    crop = lambda ox, oy: big[16 - oy:16 - oy + h, 16 - ox:16 - ox + w].copy()
    I0, I1 = crop(0, 0), crop(d[0], d[1])
    want = crop(int(t * d[0]), int(t * d[1]))
    F = np.broadcast_to(np.array(d, f32), (h, w, 2)).copy()
    dst, code, st = I.interp(I0, I1, F, -F, t)
    m = 9
    assert np.array_equal(dst[m:-m, m:-m], want[m:-m, m:-m])
    assert (code[m:-m, m:-m] == 0).all()
    assert st[:3].sum() == h * w


def test_sub_half_pixel_motion_every_pixel_is_its_own_candidate():
    rng = np.random.default_rng(3)
    h, w, t = 21, 30, 0.5
    I0, I1 = rand_img(rng, h, w, 3), rand_img(rng, h, w, 3)
    F = rng.uniform(-0.9, 0.9, (h, w, 2)).astype(f32)                      # t |V| < 1/2
    B = rng.uniform(-0.9, 0.9, (h, w, 2)).astype(f32)
    Z = np.zeros((h, w), np.uint8)
    dst, code, st, KF, KB = I.interp(I0, I1, F, B, t, Z, Z, planes=True)
    idx = np.arange(h * w, dtype=np.uint64).reshape(h, w)
    assert np.array_equal(KF & np.uint64(0xFFFFFFFF), idx) and np.array_equal(KB & np.uint64(0xFFFFFFFF), idx)
    assert (code & 3 == 0).all() and st[0] == h * w
    v0, own0, _ = W.warp(I0, -(f32(t) * F))
    v1, own1, _ = W.warp(I1, (f32(1) - f32(t)) * F)
    both = (own0 == 0) & (own1 == 0)
    assert np.array_equal(dst[both], (f32(0.5) * v0 + f32(0.5) * v1)[both])
    assert np.array_equal(dst[(own0 == 0) & (own1 != 0)], v0[(own0 == 0) & (own1 != 0)])
    assert np.array_equal(code[(own0 == 0) & (own1 != 0)], np.full(((own0 == 0) & (own1 != 0)).sum(), 4))
    # the cost in the key is fotg_warp's residual term, quantised
    wv, _, _ = W.warp(I1, F)
    e = np.abs(I0[..., 0] - wv[..., 0]) + np.abs(I0[..., 1] - wv[..., 1]) + np.abs(I0[..., 2] - wv[..., 2])
    assert np.array_equal((KF >> np.uint64(32)) & np.uint64(0xFFFFFF), np.floor(e * f32(256)).astype(np.uint64))


# ---- hand-made 4 x 4 cases ---------------------------------------------------------------------------------------------------------
def base4():
    """I0 = I1 = a ramp; no motion anywhere; all consistent: the tests below move single pixels"""
    S = (np.arange(16, dtype=f32).reshape(4, 4) * 10)
    Z = np.zeros((4, 4, 2), f32)
    return S.copy(), S.copy(), Z.copy(), Z.copy(), np.zeros((4, 4), np.uint8), np.zeros((4, 4), np.uint8)


def winner(K, y, x):
    return int(K[y, x] & np.uint64(0xFFFFFFFF))


def test_key_consistent_beats_inconsistent_at_higher_cost():
    I0, I1, F, B, mF, mB = base4()
    # (0,0) and (0,2) [x = 0 and x = 2 of row 0] both land on (0,1) at t = 0.5; the pixel (0,1) itself is sent away (code 2)
    F[0, 0], F[0, 2], mF[0, 1] = (2, 0), (-2, 0), 2
    I1[0, 2] = 0                       # source x = 0 (value 0) matches I1 at x = 2: cost 0; source x = 2 (20) finds I1[0,0] = 0: cost 20
    mF[0, 0] = 1                       # ... but the cheap one is inconsistent
    _, _, _, KF, _ = I.interp(I0, I1, F, B, 0.5, mF, mB, planes=True)
    assert winner(KF, 0, 1) == 2 and KF[0, 1] >> np.uint64(56) == 0
    mF[0, 0] = 0                       # both consistent: the lower cost wins
    _, _, _, KF, _ = I.interp(I0, I1, F, B, 0.5, mF, mB, planes=True)
    assert winner(KF, 0, 1) == 0 and (KF[0, 1] >> np.uint64(32)) == 0
    mF[0, 2] = 1                       # both ways round
    _, _, _, KF, _ = I.interp(I0, I1, F, B, 0.5, mF, mB, planes=True)
    assert winner(KF, 0, 1) == 0


def test_key_lower_cost_wins_and_equal_cost_goes_to_the_lower_index():
    I0, I1, F, B, mF, mB = base4()
    F[1, 0], F[1, 2], mF[1, 1] = (2, 0), (-2, 0), 3
    I1[1, 2], I1[1, 0] = 47, 53        # source x = 0 (40): |40 - 47| = 7; source x = 2 (60): |60 - 53| = 7
    _, _, _, KF, _ = I.interp(I0, I1, F, B, 0.5, mF, mB, planes=True)
    assert winner(KF, 1, 1) == 4 and (KF[1, 1] >> np.uint64(32)) == 7 * 256
    I1[1, 0] = 54                      # 60 - 54 = 6 < 7: the higher index now wins by cost
    _, _, _, KF, _ = I.interp(I0, I1, F, B, 0.5, mF, mB, planes=True)
    assert winner(KF, 1, 1) == 6 and (KF[1, 1] >> np.uint64(32)) == 6 * 256
    I1[1, 0] = 53.99                   # the cost is quantised to 1/256: 6.01 -> 1538 < 7 * 256
    _, _, _, KF, _ = I.interp(I0, I1, F, B, 0.5, mF, mB, planes=True)
    assert winner(KF, 1, 1) == 6 and (KF[1, 1] >> np.uint64(32)) == int(np.floor((f32(60) - f32(53.99)) * f32(256)))


def test_codes_2_and_3_and_non_finite_vectors_never_project_and_the_backward_flow_fills():
    I0, I1, F, B, mF, mB = base4()
    mF[2, 1], mF[2, 2], mF[3, 3] = 2, 3, 200
    F[2, 3] = (np.nan, 0)
    B[2, 0] = (np.inf, 0)
    mB[3, 0] = 3
    dst, code, st, KF, KB = I.interp(I0, I1, F, B, 0.5, mF, mB, planes=True)
    empty_f = np.zeros((4, 4), bool)
    empty_f[2, 1] = empty_f[2, 2] = empty_f[3, 3] = empty_f[2, 3] = True
    assert np.array_equal(KF == I.EMPTY, empty_f)
    assert (KB == I.EMPTY).sum() == 2 and KB[2, 0] == I.EMPTY and KB[3, 0] == I.EMPTY
    # the backward flow fills only where the forward flow left nothing
    assert np.array_equal(code & 3, np.where(empty_f, 1, 0))
    assert np.array_equal(st[:3], [12, 4, 0])
    # a backward vector is used negated: B = (-2, 0) at (3, 3) alone lands on (3, 2) at t = 0.5, V = (2, 0)
    I0, I1, F, B, mF, mB = base4()
    mF[:], mB[:] = 2, 2
    mB[3, 3] = 1
    B[3, 3] = (-2, 0)
    dst, code, st, KF, KB = I.interp(I0, I1, F, B, 0.5, mF, mB, planes=True)
    assert (KF == I.EMPTY).all() and (KB != I.EMPTY).sum() == 1 and winner(KB, 3, 2) == 15 and KB[3, 2] >> np.uint64(56) == 1
    assert code[3, 2] & 3 == 1 and ((code & 3) == 2).sum() == 15 and np.array_equal(st[:3], [0, 1, 15])
    # x0 = 2 - 0.5 * 2 = 1, x1 = 2 + 0.5 * 2 = 3: frame 0 at (3, 1) = 130, frame 1 at (3, 3) = 150; mF there is 2 (set), mB is 1 (set)
    assert dst[3, 2] == 0.5 * 130 + 0.5 * 150 and code[3, 2] == 1
    # holes are the plain blend whatever the masks say
    assert dst[0, 0] == 0 and code[0, 0] == 2


def test_one_sided_rules():
    I0, I1, F, B, mF, mB = base4()
    I1 += 1
    F[:], B[:] = (1, 0), (-1, 0)                   # t = 0.5: x0 = x - 0.5 -> nearest pixel floor(x0 + 0.5) = x; x1 = x + 0.5 -> x + 1
    # row 0: o0 set at x = 1 only; row 1: o1 set at the pixel x1 = 2 + 1 only; row 2: both set; row 3: neither
    mF[0, 1] = 1
    mB[1, 3] = 1
    mF[2, 1], mB[2, 2] = 1, 1
    dst, code, st = I.interp(I0, I1, F, B, 0.5, mF, mB)
    v0 = lambda y, x: 0.5 * (I0[y, x - 1] + I0[y, x])
    v1 = lambda y, x: 0.5 * (I1[y, x] + I1[y, x + 1])
    # targets: source x lands on floor(x + 0.5 + 0.5) = x + 1, so column 0 has no forward key; its backward key comes from x = 1
    assert (code[:, 1:] & 3 == 0).all() and (code[:, 0] & 3 == 1).all()
    # o0 && !o1 -> w1 = 0: only frame 0 (code + 4)
    assert code[0, 1] == 4 and dst[0, 1] == v0(0, 1)
    # o1 && !o0 -> w0 = 0: only frame 1 (code + 8)
    assert code[1, 2] == 8 and dst[1, 2] == v1(1, 2)
    # both set, or neither: both frames
    assert code[2, 1] == 0 and dst[2, 1] == f32(0.5) * f32(v0(2, 1)) + f32(0.5) * f32(v1(2, 1))
    assert code[3, 1] == 0 and code[3, 2] == 0
    # the last column: x1 = 3.5 leaves the frame -> in1 false -> only frame 0; column 0: x0 = -0.5 leaves -> only frame 1
    assert (code[[0, 2, 3], 3] == 4).all() and dst[3, 3] == v0(3, 3)
    assert (code[:, 0] == 1 + 8).all() and dst[3, 0] == v1(3, 0)
    # (1, 3): x1 leaves the frame AND its nearest in-frame pixel (1, 3) has o1 set with o0 clear: neither frame is left, the blend
    assert code[1, 3] == 0 and dst[1, 3] == f32(0.5) * f32(v0(1, 3)) + f32(0.5) * I1[1, 3]
    assert st[3] == (code >= 4).sum() == 3 + 4 + 2
    # a hole ignores the masks
    mF[:], mB[:] = 2, 2
    mF[0, 0], mB[0, 0] = 1, 0
    F[:], B[:] = 0, 0
    dst, code, st = I.interp(I0, I1, F, B, 0.5, mF, mB)
    assert code[0, 1] == 2 and dst[0, 1] == f32(0.5) * I0[0, 1] + f32(0.5) * I1[0, 1] and code[0, 0] == 4


def test_codes_sum_to_the_pixels_and_the_statistics_are_the_terms():
    rng = np.random.default_rng(6)
    for (h, w), noc in (((37, 53), 1), ((5, 3), 3), ((64, 96), 3)):
        I0, I1, R = rand_img(rng, h, w, noc), rand_img(rng, h, w, noc), rand_img(rng, h, w, noc)
        F, B = W.case_flow("integer", h, w, 1), W.case_flow("smooth", h, w, 2)
        dst, code, st, tv, tb = I.interp(I0, I1, F, B, 0.3, ref=R, terms=True)
        assert st[:3].sum() == h * w and np.array_equal(st[:3], np.bincount((code & 3).ravel(), minlength=3)[:3])
        assert st[3] == (code >= 4).sum() and not ((code & 4 != 0) & (code & 8 != 0)).any()
        assert len(tv) == len(tb) == h * w * noc
        assert np.array_equal(tv, np.abs(R - dst).astype(np.float64).ravel()) and st[4] == math.fsum(tv)     # f32 terms, widened
        assert np.array_equal(tb, np.abs(R - (f32(0.7) * I0 + f32(0.3) * I1)).astype(np.float64).ravel()) and st[5] == math.fsum(tb)
        # the masks the restatement computes itself are fb_check's
        mF, mB = FB.fb_check(F, B)
        d2, c2, s2 = I.interp(I0, I1, F, B, 0.3, mF, mB, ref=R)
        assert np.array_equal(d2, dst) and np.array_equal(c2, code) and np.array_equal(s2, st)


# ---- quality on the reference's frames ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("triplet", sorted(QUALITY))
def test_quality_on_alley_triplets(triplet, alley):
    from oracle import oracle as O
    more = np.load(os.path.join(GOLDEN, "alley_1_more.npz"))
    assert os.path.getsize(os.path.join(GOLDEN, "alley_1_more.npz")) < 1024 * 1024
    fr = {1: alley["frame_0001"], 2: alley["frame_0002"], 3: more["frame_0003"], 20: more["frame_0020"], 21: more["frame_0021"],
          22: more["frame_0022"]}
    f0, fm, f1 = (fr[k].astype(f32) for k in triplet)
    F, B = O.full_flow(f0, f1), O.full_flow(f1, f0)
    dst, code, st = I.interp(f0, f1, F, B, 0.5, ref=fm)
    blend_db, interp_db = QUALITY[triplet]
    blend, got = I.psnr(f32(0.5) * f0 + f32(0.5) * f1, fm), I.psnr(dst, fm)
    print("%s: blend %.4f dB, interpolated %.4f dB, gain %.4f dB, holes %.5f" % (triplet, blend, got, got - blend, st[2] / code.size))
    assert abs(blend - blend_db) < 1e-3
    assert got >= blend + 0.5 * (interp_db - blend_db)
    assert st[2] <= HOLE_SHARE_MAX * code.size
