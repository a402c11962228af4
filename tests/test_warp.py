"""CPU tests of the frame warp's restatement (tests/warp_ref.py): it IS the reference's image_warp -- equal to the oracle's
dis_image_warp, to the live image_warp of oracle/_ref where that is built, and to the recorded outputs of the live reference
(tests/golden/image_warp_ref.npz) everywhere -- and its codes, occ merging, fill modes, 8-bit rounding and statistics on
hand-made 4 x 4 cases."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import warp_ref as W
from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import make_warp_golden as G  # noqa: E402

f32 = np.float32
CASES = W.cases()


def oracle_image_warp(img, flow):
    """oracle/dis_oracle.c dis_image_warp (planar, rows padded to a multiple of 4) on an interleaved image"""
    from oracle import oracle as O
    L = O.lib()
    noc = 1 if img.ndim == 2 else 3
    h, w = flow.shape[:2]
    st = (w + 3) // 4 * 4
    src = np.zeros((noc, h, st), f32)
    src[:, :, :w] = img[None] if noc == 1 else img.transpose(2, 0, 1)
    wx, wy = np.zeros((h, st), f32), np.zeros((h, st), f32)
    wx[:, :w], wy[:, :w] = flow[..., 0], flow[..., 1]
    dst, mask = np.zeros((noc, h, st), f32), np.zeros((h, st), f32)
    L.dis_image_warp.argtypes = [O.f32p] * 5 + [C.c_int] * 3
    L.dis_image_warp.restype = None
    L.dis_image_warp(O.P(dst), O.P(mask), O.P(src), O.P(wx), O.P(wy), w, h, noc)
    d = dst[:, :, :w]
    return (d[0].copy() if noc == 1 else np.ascontiguousarray(d.transpose(1, 2, 0))), mask[:, :w].copy()


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(GOLDEN, "image_warp_ref.npz"))
    return {k: z[k] for k in z.files}


def test_fixture_holds_every_case_and_is_small(golden):
    assert os.path.getsize(os.path.join(GOLDEN, "image_warp_ref.npz")) < 228 * 1024
    assert sorted(golden) == sorted("%s/%s" % (c[0], k) for c in CASES for k in ("dst", "mask", "sha"))
    assert len(CASES) == 2 * 3 * 5


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_restatement_is_the_reference(case, golden):
    name, noc, h, w, kind, seed = case
    img, flow = W.case_image(h, w, noc, seed), W.case_flow(kind, h, w, seed)
    dst, code, stats = W.warp(img, flow)
    assert dst.dtype == f32 and not (code == 3).any() and not (code == 1).any()
    # the oracle's restatement of image_warp
    odst, omask = oracle_image_warp(img, flow)
    assert same_bits(dst, odst), np.argwhere(dst != odst)[:5]
    assert np.array_equal(code == 0, omask == 1)
    # the recorded outputs of the reference's own code
    assert np.array_equal(code == 0, golden[name + "/mask"] == 1)
    assert same_bits(np.ascontiguousarray(dst[::G.row_step(h)]), golden[name + "/dst"])
    assert np.array_equal(G.digest(dst), golden[name + "/sha"])
    assert stats[0] == (code == 0).sum() and stats[2] == (code == 2).sum() and stats[0] + stats[2] == h * w
    if kind == "random":
        assert (code == 2).mean() > 0.5
    if kind == "border":
        assert (code == 0).mean() > 0.3


def test_restatement_is_the_live_reference():
    """where oracle/_ref is built: the reference's image_warp itself, every case (elsewhere the fixture above stands in)"""
    refs = G.live_refs()
    if refs is None:
        return
    for name, noc, h, w, kind, seed in CASES:
        img, flow = W.case_image(h, w, noc, seed), W.case_flow(kind, h, w, seed)
        dst, code, _ = W.warp(img, flow)
        ldst, lmask = G.live_image_warp(refs, img, flow)
        assert same_bits(dst, ldst), name
        assert np.array_equal(code == 0, lmask == 1), name


# ---- hand-made 4 x 4 cases -------------------------------------------------------------------------------------------------------
S4 = np.arange(16, dtype=f32).reshape(4, 4) * 10          # S[y][x] = 10 (4 y + x)


def flow4():
    """row 0: identity, +0.5 in x, +0.25 in y, (0.5, 0.5); row 1: NaN, inf, leaves to the left, leaves below;
    row 2: exactly onto the last column, onto column 0, one past the last column, 1e30; row 3: identity"""
    F = np.zeros((4, 4, 2), f32)
    F[0, 1] = (0.5, 0)
    F[0, 2] = (0, 0.25)
    F[0, 3] = (-0.5, 0.5)
    F[1, 0] = (np.nan, 0)
    F[1, 1] = (0, np.inf)
    F[1, 2] = (-2.5, 0)
    F[1, 3] = (0, 2.5)
    F[2, 0] = (3, 0)
    F[2, 1] = (-1, 0)
    F[2, 2] = (1.5, 0)
    F[2, 3] = (1e30, 0)
    return F


def test_codes_values_and_reference_fill_mode():
    dst, code, stats = W.warp(S4, flow4(), fill=-1.0)
    assert np.array_equal(code, [[0, 0, 0, 0], [3, 3, 2, 2], [0, 0, 2, 2], [0, 0, 0, 0]])
    # row 0: S[0][0]; (10 + 20) / 2; 20 * 0.75 + 60 * 0.25; the mean of S[0][2], S[0][3], S[1][2], S[1][3]
    assert np.array_equal(dst[0], [0, 15, 30, 45])
    # row 1: unknown -> fill; outside keeps the reference's clamped taps: column 0 of row 1, row 3 of column 3
    assert np.array_equal(dst[1], [-1, -1, 40, 150])
    # row 2: S[2][3]; S[2][0]; clamped to S[2][3]; 1e30 saturates to S[2][3]
    assert np.array_equal(dst[2], [110, 80, 110, 110])
    assert np.array_equal(dst[3], S4[3])
    assert np.array_equal(stats, [10, 0, 4, 2, 0, 0])


def test_occ_merging_and_fill_mode_1():
    occ = np.zeros((4, 4), np.uint8)
    occ[0, 0], occ[0, 1], occ[1, 0], occ[1, 2], occ[3, 3], occ[3, 2] = 1, 3, 0, 1, 1, 200
    dst, code, stats = W.warp(S4, flow4(), occ=occ, fill_mode=1, fill=7.0)
    # the warp's own 2 / 3 win over occ; occ's 1 and 3 show where the warp's own code is 0; a byte above 3 counts as 3
    assert np.array_equal(code, [[1, 3, 0, 0], [3, 3, 2, 2], [0, 0, 2, 2], [0, 0, 3, 1]])
    assert np.array_equal(dst, [[7, 7, 30, 45], [7, 7, 7, 7], [110, 80, 7, 7], [120, 130, 7, 7]])
    assert np.array_equal(stats, [6, 2, 4, 4, 0, 0])
    # reference fill mode keeps every value the warp itself knows, whatever occ says
    dst0, code0, _ = W.warp(S4, flow4(), occ=occ, fill_mode=0, fill=7.0)
    assert np.array_equal(code0, code)
    assert np.array_equal(dst0, [[0, 15, 30, 45], [7, 7, 40, 150], [110, 80, 110, 110], [120, 130, 140, 150]])


def test_8_bit_rounding_and_clamping():
    S = np.array([[0, 1, 2, 3], [250, 251, 253, 255], [4, 7, 4, 7], [0, 0, 0, 0]], np.uint8)
    F = np.zeros((4, 4, 2), f32)
    F[0, 0] = (0.5, 0)          # 0.5 -> rint to even 0
    F[0, 1] = (0.5, 0)          # 1.5 -> 2
    F[0, 2] = (0.5, 0)          # 2.5 -> 2
    F[1, 0] = (0.25, 0)         # 250.25 -> 250
    F[1, 2] = (0.75, 0)         # 254.5 -> 254
    F[2, 0] = (0.5, 0)          # 5.5 -> 6
    F[3, 0] = (np.nan, 0)
    for fill, want_fill in ((300.0, 255), (-4.0, 0), (6.5, 6), (np.nan, 0)):
        dst, code, _ = W.warp(S, F, fill=fill)
        assert dst.dtype == np.uint8
        assert np.array_equal(dst, [[0, 2, 2, 3], [250, 251, 254, 255], [6, 7, 4, 7], [want_fill, 0, 0, 0]]), fill
    # the residuals use the unrounded value: |0 - 0.5| + ... over the code-0 pixels
    R = np.zeros((4, 4), np.uint8)
    _, code, stats, tw, tu = W.warp(S, F, ref=R, terms=True)
    assert stats[0] == 15 and len(tw) == len(tu) == 15
    assert stats[4] == 0.5 + 1.5 + 2.5 + 3 + 250.25 + 251 + 254.5 + 255 + 5.5 + 7 + 4 + 7
    assert stats[5] == float(S.astype(np.int64).sum())


def test_stats_of_three_channels_and_masked_pixels():
    S = np.stack([S4, S4 + 1, S4 + 2], -1)
    R = np.full((4, 4, 3), 100, f32)
    occ = np.zeros((4, 4), np.uint8)
    occ[3] = 1
    dst, code, stats, tw, tu = W.warp(S, flow4(), ref=R, occ=occ, fill_mode=1, fill=0.0, terms=True)
    ok = code == 0
    assert np.array_equal(code, [[0, 0, 0, 0], [3, 3, 2, 2], [0, 0, 2, 2], [1, 1, 1, 1]]) and len(tw) == len(tu) == 18
    want = np.array([[0, 15, 30, 45], [0, 0, 0, 0], [110, 80, 0, 0], [0, 0, 0, 0]], f32)
    assert np.array_equal(dst[..., 0], want) and np.array_equal(dst[..., 2][ok], want[ok] + 2)
    # over the six code-0 pixels and the three channels: |100 - (value + c)| and |100 - (S[y][x] + c)|
    assert stats[4] == sum(abs(100 - (v + c)) for v in (0, 15, 30, 45, 110, 80) for c in range(3))
    assert stats[5] == sum(abs(100 - (v + c)) for v in (0, 10, 20, 30, 80, 90) for c in range(3))
    assert np.array_equal(stats[:4], [6, 4, 4, 2])
