"""CPU tests of the forward-backward consistency restatement (tests/fbcheck_ref.py) on hand-built cases whose codes are known."""
import numpy as np

import fbcheck_ref as R

f32 = np.float32


def field(h, w, u=0.0, v=0.0):
    f = np.zeros((h, w, 2), f32)
    f[..., 0], f[..., 1] = u, v
    return f


def test_zero_flows_are_consistent_everywhere():
    m, mb = R.fb_check(field(9, 13), field(9, 13))
    assert not m.any() and not mb.any()
    assert R.counts(m, mb).tolist() == [[[117, 0, 0, 0], [117, 0, 0, 0]]]


def test_translation_with_its_exact_inverse():
    h, w = 11, 17
    m, mb = R.fb_check(field(h, w, 3, -2), field(h, w, -3, 2))
    want = np.zeros((h, w), np.uint8)
    want[:, w - 3:] = 2                    # x + 3 > w - 1
    want[:2, :] = 2                        # y - 2 < 0
    assert np.array_equal(m, want)
    want_bw = np.zeros((h, w), np.uint8)
    want_bw[:, :3] = 2
    want_bw[h - 2:, :] = 2
    assert np.array_equal(mb, want_bw)


def test_moving_square_marks_the_occluded_and_disoccluded_strips():
    h, w, s, k, d = 24, 32, 8, 8, 4        # an 8 x 8 square at (8, 8) moves right by 4 over a static background
    F, B = field(h, w), field(h, w)
    F[s:s + k, s:s + k, 0] = d
    B[s:s + k, s + d:s + d + k, 0] = -d
    m, mb = R.fb_check(F, B)
    want = np.zeros((h, w), np.uint8)
    want[s:s + k, s + k:s + k + d] = 1     # background of frame 0 the square covers in frame 1
    want_bw = np.zeros((h, w), np.uint8)
    want_bw[s:s + k, s:s + d] = 1          # background of frame 1 the square uncovered
    assert np.array_equal(m, want) and np.array_equal(mb, want_bw)


def test_target_exactly_on_the_last_column_and_row_is_inside():
    h, w = 6, 8
    xs = np.arange(w, dtype=f32)
    F = field(h, w)
    F[..., 0] = f32(w - 1) - xs            # every target on x = w - 1 exactly
    F[..., 1] = f32(h - 1) - np.arange(h, dtype=f32)[:, None]
    code = R.fb_code(F, field(h, w))
    assert (code != 2).all()
    # |F|^2 = lhs against 0.01 |F|^2 + 0.5: consistent only where F = 0 (the bottom-right pixel)
    want = np.ones((h, w), np.uint8)
    want[h - 1, w - 1] = 0
    assert np.array_equal(code, want)
    F[0, 0, 0] = np.nextafter(F[0, 0, 0], f32(np.inf))    # a hair past the last column
    assert R.fb_code(F, field(h, w))[0, 0] == 2


def test_non_finite_and_huge_values():
    h, w = 5, 7
    F, B = field(h, w, 1, 0), field(h, w, -1, 0)
    F[0, 0] = (np.nan, 0)
    F[0, 1] = (0, np.inf)
    F[0, 2] = (-np.inf, 0)
    F[0, 3] = (1e30, 0)                    # finite: leaves the frame
    code = R.fb_code(F, B)
    assert code[0, :4].tolist() == [3, 3, 3, 2]
    assert code[1, 0] == 0
    # non-finite or huge backward vectors where the forward ones land: inconsistent
    for bad in (np.nan, np.inf, -np.inf, f32(1e30)):
        B2 = B.copy()
        B2[2, 3] = (bad, 0)
        c2 = R.fb_code(F, B2)
        assert c2[2, 2] == 1, bad           # (2, 2) + (1, 0) lands exactly on (3, 2)
        assert c2[3, 2] == 0
    m, mb = R.fb_check(F, B)
    assert R.counts(m, mb)[0, 0].sum() == h * w and R.counts(m, mb)[0, 0, 3] == 3


def test_exactly_on_the_threshold():
    h, w = 3, 4
    F, B = field(h, w, 1, 0), field(h, w)
    # lhs = 1 * 1 = 1, rhs = 0 * (1 + 0) + alpha2: equal -> 1 (the test is lhs < rhs), a hair above -> 0
    assert R.fb_code(F, B, alpha1=0.0, alpha2=1.0)[0, 0] == 1
    assert R.fb_code(F, B, alpha1=0.0, alpha2=float(np.nextafter(f32(1), f32(2))))[0, 0] == 0
    # with alpha1: lhs = 4, rhs = 0.5 * (4 + 0) + 2 = 4 exactly
    F2 = field(h, w, 2, 0)
    assert R.fb_code(F2, B, alpha1=0.5, alpha2=2.0)[0, 0] == 1
    # 2 + nextafter(2) is 4 + 2^-22, half an ulp of 4: the f32 sum rounds back to 4 (to even), still not below
    assert R.fb_code(F2, B, alpha1=0.5, alpha2=float(np.nextafter(f32(2), f32(3))))[0, 0] == 1
    assert R.fb_code(F2, B, alpha1=0.5, alpha2=float(np.nextafter(np.nextafter(f32(2), f32(3)), f32(3))))[0, 0] == 0


def test_restatement_rounds_in_float32():
    # a sub-pixel target: the bilinear sample and the sums are float32 values, not float64 ones
    F, B = field(4, 4, 0.3, 0.7), field(4, 4, -0.3, -0.7)
    B[1, 1] = (-0.31, -0.69)
    code = R.fb_code(F, B)
    assert code.dtype == np.uint8 and set(np.unique(code)) <= {0, 2}
