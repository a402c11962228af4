"""The pull-push hole filling restated (tests/fill_ref.py), without a GPU: the vectorised restatement equals a per-pixel, per-level
loop written straight from the definition on shapes up to 13 x 9; constants with at most 8 fractional bits are reproduced exactly
through any hole pattern; filled values stay within the range of the known ones; known pixels and empty images are kept bit for
bit; depth has its closed form for a k x k hole; 1 x 1 images; the fg selection equals a boolean map."""
import numpy as np
import pytest

import fill_ref as R

SHAPES = [(1, 1), (1, 2), (2, 1), (1, 7), (5, 1), (2, 2), (3, 5), (4, 4), (8, 8), (7, 9), (9, 13), (13, 9)]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8 if a.dtype == np.uint8 else np.uint32)


def frame(h, w, ch, dtype, seed):
    rng = np.random.default_rng(seed)
    if dtype == np.uint8:
        return rng.integers(0, 256, (h, w, ch)).astype(np.uint8)
    return ((rng.random((h, w, ch)) - 0.3) * 700).astype(np.float32)              # more than 8 fractional bits: q rounds


def patterns(h, w, seed):
    rng = np.random.default_rng(seed)
    pats = [np.zeros((h, w), bool), np.ones((h, w), bool), rng.random((h, w)) < 0.5, rng.random((h, w)) < 0.9]
    for y, x in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)):
        m = np.ones((h, w), bool)
        m[y, x] = False                                                           # one known pixel, in each corner
        pats.append(m)
    m = np.zeros((h, w), bool)
    m[h // 3:h // 3 + max(1, h // 2), w // 4:w // 4 + max(1, w // 2)] = True      # a rectangle
    pats.append(m)
    return pats


@pytest.mark.parametrize("dtype", [np.float32, np.uint8])
@pytest.mark.parametrize("shape", SHAPES)
def test_the_restatement_equals_the_loops_of_the_definition(shape, dtype):
    h, w = shape
    for ch in ((1, 2, 3) if dtype == np.float32 else (1, 3)):
        src = frame(h, w, ch, dtype, 7 * h + w + ch)
        for k, hole in enumerate(patterns(h, w, h * 31 + w)):
            hb = (hole * (1 + k)).astype(np.uint8)
            got, want = R.fill_one(src, hb), R.naive(src, hb)
            assert np.array_equal(bits(got[0]), bits(want[0])), (shape, ch, k)
            assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), (shape, ch, k, got[2], want[2])


def test_values_are_holes_without_a_map():
    src = frame(9, 13, 2, np.float32, 3)
    bad = [(0, 0, np.nan), (3, 4, np.inf), (7, 11, -np.inf), (5, 5, 1e9), (2, 9, 32768.5), (6, 1, -40000.0)]
    for k, (y, x, v) in enumerate(bad):
        src[y, x, k % 2] = v
    src[1, 1] = (32768.0, -32768.0)                                               # the largest known values
    for hole in (None, np.zeros((9, 13), np.uint8)):
        dst, code, stats = R.fill_one(src, hole)
        want = R.naive(src, hole)
        assert np.array_equal(bits(dst), bits(want[0])) and np.array_equal(code, want[1]) and np.array_equal(stats, want[2])
        assert code.sum() == len(bad) and all(code[y, x] == 1 for y, x, _ in bad) and code[1, 1] == 0
        assert np.isfinite(dst).all() and np.abs(dst).max() <= 32768 and stats.tolist() == [9 * 13 - len(bad), len(bad), 0, 1]


@pytest.mark.parametrize("shape", [(13, 9), (40, 70), (64, 65)])
def test_constants_with_eight_fractional_bits_are_reproduced_exactly(shape):
    h, w = shape
    for v in (0.0, 1.0, -3.5, 255.0, 17.00390625, -32768.0, 32767.99609375):
        for hole in patterns(h, w, 5)[2:]:
            src = np.full((h, w, 2), v, np.float32)
            junk = np.where(hole[..., None], np.float32(123.25), src)             # what lies in the holes does not matter
            dst, code, _ = R.fill_one(junk, hole.astype(np.uint8))
            assert np.array_equal(bits(dst), bits(src)) and np.array_equal(code, hole.astype(np.uint8))
    for v in (0, 1, 128, 255):
        for hole in patterns(h, w, 6)[2:]:
            src = np.full((h, w, 3), v, np.uint8)
            dst, _, _ = R.fill_one(np.where(hole[..., None], np.uint8(77), src), hole.astype(np.uint8))
            assert np.array_equal(dst, src)


@pytest.mark.parametrize("shape", [(13, 9), (37, 70), (65, 64)])
def test_filled_values_stay_within_the_known_range_and_known_pixels_are_kept(shape):
    h, w = shape
    for ch in (1, 3):
        src = frame(h, w, ch, np.float32, h + ch)
        for hole in patterns(h, w, 9):
            dst, code, stats = R.fill_one(src, hole.astype(np.uint8))
            known = ~hole
            assert np.array_equal(bits(dst)[known], bits(src)[known])
            if not known.any():                                                   # the empty image: kept bit for bit, code 2
                assert np.array_equal(bits(dst), bits(src)) and (code == 2).all() and stats.tolist()[:3] == [0, 0, h * w]
                continue
            assert np.array_equal(code, hole.astype(np.uint8)) and stats.tolist()[:3] == [known.sum(), hole.sum(), 0]
            for c in range(ch):
                lo, hi = src[..., c][known].min(), src[..., c][known].max()
                # a mean of 8-bit fractions is within 2^-9 of the range, the bilinear steps add f32 roundings of values <= 700
                tol = 2.0 ** -9 + 16 * 700 * 2.0 ** -24
                assert dst[..., c].min() >= lo - tol and dst[..., c].max() <= hi + tol
        u8 = frame(h, w, ch, np.uint8, h)
        hole = patterns(h, w, 2)[2]
        dst, _, _ = R.fill_one(u8, hole.astype(np.uint8))
        assert np.array_equal(dst[~hole], u8[~hole])
        for c in range(ch):
            assert u8[..., c][~hole].min() <= dst[..., c].min() and dst[..., c].max() <= u8[..., c][~hole].max()


def hole_depth(k, x0, y0):
    """1 + the largest l at which a block of side 2^l lies inside the k x k hole at (x0, y0); 0 without a hole"""
    depth = 0
    for l in range(0, 16):
        s = 1 << l
        fits = lambda a: (-(-a // s) + 1) * s <= a + k                            # an aligned block [m s, (m + 1) s) inside [a, a + k)
        if fits(x0) and fits(y0):
            depth = l + 1
    return depth


def test_depth_has_its_closed_form_for_a_square_hole():
    h, w = 70, 90
    src = frame(h, w, 1, np.float32, 1)
    assert R.fill_one(src, np.zeros((h, w), np.uint8))[2][3] == 0
    for k, x0, y0 in ((1, 5, 5), (2, 4, 6), (2, 5, 6), (3, 5, 5), (4, 8, 12), (4, 9, 12), (16, 16, 32), (16, 17, 32), (31, 1, 1), (32, 32, 0),
                      (33, 31, 0), (64, 0, 0), (64, 1, 1)):
        hole = np.zeros((h, w), np.uint8)
        hole[y0:y0 + k, x0:x0 + k] = 1
        assert R.fill_one(src, hole)[2][3] == hole_depth(k, x0, y0), (k, x0, y0)
    # the frames of the GPU tests reach above the 64 x 64 tile: a half-frame hole, and one known corner pixel
    for (h, w), half, corner in (((200, 300), 7, 9), ((139, 150), 6, 8)):
        src = frame(h, w, 1, np.float32, 2)
        hole = np.zeros((h, w), np.uint8)
        hole[:, :w // 2 + 22] = 1
        assert R.fill_one(src, hole)[2][3] >= half
        hole[:] = 1
        hole[0, 0] = 0
        assert R.fill_one(src, hole)[2][3] == corner
        hole[0, 0] = 1
        assert R.fill_one(src, hole)[2].tolist() == [0, 0, h * w, corner + 1]


def test_one_pixel_images():
    for dtype in (np.float32, np.uint8):
        src = np.array([[[7, 9, 250]]], dtype)
        for hole, code, stats in ((0, 0, [1, 0, 0, 0]), (3, 2, [0, 0, 1, 1])):
            dst, c, s = R.fill_one(src, np.array([[hole]], np.uint8))
            assert np.array_equal(dst, src) and c.tolist() == [[code]] and s.tolist() == stats
            assert R.naive(src, np.array([[hole]], np.uint8))[2].tolist() == stats
    dst, c, s = R.fill_one(np.array([[[np.nan]]], np.float32))
    assert np.isnan(dst[0, 0, 0]) and c.tolist() == [[2]] and s.tolist() == [0, 0, 1, 1]


def test_fg_selection_equals_a_boolean_map():
    rng = np.random.default_rng(4)
    h, w = 21, 34
    src = frame(h, w, 3, np.uint8, 8)
    codes = rng.choice(np.array([0, 1, 2, 3, 4, 7, 8, 9, 255], np.uint8), (h, w))
    for fg in ((2, 3), (0,), (7, 1), (0, 1, 2, 3, 4, 5, 6, 7)):
        boolean = np.isin(codes, fg).astype(np.uint8)
        got, want = R.fill_one(src, codes, fg), R.fill_one(src, boolean)
        assert all(np.array_equal(a, b) for a, b in zip(got, want)), fg
    assert np.array_equal(R.hole_map(codes), codes != 0)
    # the batched and the single forms are the per-image results
    srcs = np.stack([frame(h, w, 3, np.uint8, k) for k in range(3)])
    holes = np.stack([codes, np.zeros_like(codes), np.ones_like(codes)])
    d, c, s = R.fill_holes(srcs, holes, (2, 3))
    for k in range(3):
        one = R.fill_holes(srcs[k], holes[k], (2, 3))
        assert np.array_equal(d[k], one[0]) and np.array_equal(c[k], one[1]) and np.array_equal(s[k], one[2])
    g = R.fill_holes(srcs[..., 0], holes)
    assert g[0].shape == (3, h, w) and np.array_equal(g[0], R.fill_holes(srcs[..., :1], holes)[0][..., 0])
