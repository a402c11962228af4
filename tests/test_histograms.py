"""Properties of the motion histograms' definition, checked on its numpy restatement (tests/histograms_ref.py).  No GPU:
tests/test_gpu_histograms.py compares the kernel with the same restatement byte for byte."""
import math
import os
import re

import numpy as np
import pytest

import histograms_ref as R

from conftest import ROOT
from host_checks import run_cli


def one(U, V, thresh256=R.THRESH256):
    """the record of a 1 x 1 image"""
    return R.from_fixed([[U]], [[V]], None, 8, thresh256)[0, 0]


def test_table_in_the_header_is_the_modules_and_the_formulas():
    src = open(os.path.join(ROOT, "flowonthego_amd", "csrc", "histograms.hip.h")).read()
    body = re.search(r"MH_ATAN\[257\]\s*=\s*\{(.*?)\};", src, re.S).group(1)
    table = [int(v) for v in re.findall(r"\d+", body)]
    assert len(table) == 257
    assert table == R.ATAN.tolist() == R.atan_formula()
    assert table[0] == 0 and table[128] == 151 and table[256] == 256
    assert all(a <= b for a, b in zip(table, table[1:]))
    # no entry is near a rounding tie, so every libm agrees
    assert min(abs((256.0 * math.atan(k / 256.0) / (math.pi / 4.0)) % 1.0 - 0.5) for k in range(257)) > 0.007


def test_hand_cases():
    r = one(3 * 256, 0)
    assert r[:8].tolist() == [768, 0, 0, 0, 0, 0, 0, 0] and r[R.ZERO] == 0 and r[R.N] == 1 and r[R.SM] == 768
    r = one(-256, -256)
    assert r[:8].tolist() == [0, 0, 0, 0, 0, 362, 0, 0] and r[R.SU] == -256 and r[R.SV] == -256
    r = one(0, -512)
    assert r[:8].tolist() == [0, 0, 0, 0, 0, 0, 512, 0]
    # a 1 x 1 image: the pixel is its own four neighbours, the gradient is zero, counted and nothing added
    assert r[R.NMBH] == 1 and not r[9:25].any() and r[31] == 0
    t = R.THRESH256
    assert t == 102
    r = one(t - 1, 0)
    assert r[R.ZERO] == 1 and not r[:8].any() and r[R.SM] == t - 1
    r = one(t, 0)
    assert r[R.ZERO] == 0 and r[0] == t
    r = one(0, 0, thresh256=0)
    assert r[R.ZERO] == 0 and not r[:25].any() and r[R.N] == 1
    r = one(0, 0)
    assert r[R.ZERO] == 1


def test_magnitude_is_the_exact_integer_root():
    rng = np.random.default_rng(3)
    a = rng.integers(-(1 << 21), (1 << 21) + 1, 4000)
    b = rng.integers(-(1 << 21), (1 << 21) + 1, 4000)
    a[:4], b[:4] = [1 << 21, -(1 << 21), 0, 3], [1 << 21, 1 << 21, 0, 4]
    m = R.mag(a, b)
    assert m.tolist() == [R.mag1(x, y) for x, y in zip(a, b)]
    assert m[0] == math.isqrt(2 << 42) and m[2] == 0 and m[3] == 5
    assert 1024 * R.mag1(1 << 20, 1 << 20) < 1 << 32 and 1024 * R.mag1(1 << 21, 1 << 21) < 1 << 32      # a 32 x 32 cell fits 32 bits
    assert 2048 * R.mag1(1 << 21, 1 << 21) >= 1 << 32                                                     # a 64 x 32 tile does not
    ang = R.angle(a[3:], b[3:])
    assert ang.tolist() == [R.angle1(x, y) for x, y in zip(a[3:], b[3:])] and ang.min() >= 0 and ang.max() < 2048
    assert [R.angle1(*v) for v in ((5, 0), (5, 5), (0, 5), (-5, 5), (-5, 0), (-5, -5), (0, -5), (5, -5))] == [256 * k for k in range(8)]
    assert R.angle1(1000, -1) == 0 and R.angle1(1000, -4) == 2047


def test_rotation_by_a_quarter_turn_rolls_the_bins_by_two():
    rng = np.random.default_rng(5)
    U = rng.integers(-3000, 3001, (24, 40))
    V = rng.integers(-3000, 3001, (24, 40))
    U[0, :8], V[0, :8] = [7, 7, 0, -7, -7, -7, 0, 7], [0, 7, 7, 7, 0, -7, -7, -7]
    U[1, :4], V[1, :4] = [1 << 20, 0, -(1 << 20), 200000], [0, 1 << 20, 1 << 20, -3]
    a = R.from_fixed(U, V, None, 8, 0)
    b = R.from_fixed(-V, U, None, 8, 0)
    assert np.array_equal(np.roll(a[..., :8], 2, -1), b[..., :8])
    assert np.array_equal(a[..., R.SM], b[..., R.SM])


def test_against_the_float_form():
    rng = np.random.default_rng(11)
    h, w, cell = 32, 48, 8
    mag = np.exp(rng.uniform(math.log(0.01), math.log(2000.0), (h, w)))
    th = rng.uniform(0, 2 * math.pi, (h, w))
    U = np.rint(256 * mag * np.cos(th)).astype(np.int64)
    V = np.rint(256 * mag * np.sin(th)).astype(np.int64)
    got = R.from_fixed(U, V, None, cell)
    m = R.mag(U, V)
    fl = R.float_hof(U, V)
    # a pixel whose magnitude lies within one unit of the threshold may fall on either side of it in the two forms: keep them apart
    assert not ((np.hypot(U, V) >= R.THRESH256) != (m >= R.THRESH256)).any()
    worst = 0.0
    for cy in range(h // cell):
        for cx in range(w // cell):
            sl = (slice(cy * cell, (cy + 1) * cell), slice(cx * cell, (cx + 1) * cell))
            d = np.abs(got[cy, cx, :8] - fl[sl].sum((0, 1))).sum()
            bound = (m[sl] / 32.0 + 4.0).sum()
            worst = max(worst, d / bound)
            assert d <= bound, (cy, cx, d, bound)
    assert worst > 0.0                             # (the two forms are not the same computation)


def test_mbh_borders_and_a_single_inadmissible_pixel():
    h, w = 9, 11
    ys, xs = np.mgrid[0:h, 0:w]
    U, V = 300 * xs + 7 * ys * ys, 50 * ys - 11 * xs * xs
    rec = R.pixel_records(np.ones((h, w), bool), U, V)
    # in the interior the difference is central, at the border one-sided: the corner pixel sees U[0][1] - U[0][0] and U[1][0] - U[0][0]
    ux, uy = int(U[0, 1] - U[0, 0]), int(U[1, 0] - U[0, 0])
    want = np.zeros(8, np.int64)
    b0, w0, b1, w1 = R.soft(R.mag1(ux, uy), R.angle1(ux, uy))
    want[b0] += w0
    want[b1] += w1
    assert rec[0, 0, 9:17].tolist() == want.tolist()
    ux, uy = int(U[4, 6] - U[4, 4]), int(U[5, 5] - U[3, 5])
    want[:] = 0
    b0, w0, b1, w1 = R.soft(R.mag1(ux, uy), R.angle1(ux, uy))
    want[b0] += w0
    want[b1] += w1
    assert rec[4, 5, 9:17].tolist() == want.tolist()
    assert rec[..., R.NMBH].sum() == h * w
    # one inadmissible pixel: out of HOF itself, out of MBH with its four neighbours, and nobody else changes
    for (y, x) in ((4, 5), (0, 0), (8, 3)):
        adm = np.ones((h, w), bool)
        adm[y, x] = False
        r2 = R.pixel_records(adm, np.where(adm, U, 0), np.where(adm, V, 0))
        gone = np.zeros((h, w), bool)
        for dy, dx in ((0, 0), (0, 1), (0, -1), (1, 0), (-1, 0)):
            if 0 <= y + dy < h and 0 <= x + dx < w:
                gone[y + dy, x + dx] = True
        assert np.array_equal(r2[..., R.NMBH] == 0, gone)
        assert not r2[gone][:, 9:25].any()
        assert np.array_equal(r2[~gone], rec[~gone])
        assert r2[y, x].tolist() == [0] * 27 + [1, 0, 0, 0, 0]
        hof_changed = (r2[..., :9] != rec[..., :9]).any(-1)
        assert hof_changed.sum() == 1 and hof_changed[y, x]


def test_groupings_and_partial_cells():
    rng = np.random.default_rng(2)
    h, w = 19, 37
    flow = (rng.standard_normal((2, h, w, 2)) * 3).astype(np.float32)
    flow[0, 3, 4] = np.nan
    flow[1, 5, 6, 0] = 4096.5
    ids = rng.integers(-2, 6, (2, h, w)).astype(np.int32)
    P = np.array([[0.01, 0.0, 0.5, 0.0, -0.01, 0.25], [0, 0, 0, 0, 0, 0]], np.float64)
    for cell in R.CELLS:
        cells, objs = R.histograms(flow, None, P, cell, ids=ids, rows=4)
        assert cells.shape == (2, -(-h // cell), -(-w // cell), 32) and objs.shape == (2, 4, 32)
        assert (cells[..., R.N] + cells[..., R.NBAD]).sum() == 2 * h * w and cells[..., R.NBAD].sum() == 2
        for i in range(2):
            assert (objs[i, :, R.N] + objs[i, :, R.NBAD]).tolist() == [int((ids[i] == k).sum()) for k in range(4)]
        assert np.array_equal(cells.sum((1, 2)), R.histograms(flow, None, P, 32)[0].sum((1, 2)))
    # a NaN parameter row leaves nothing admissible
    P[1, 2] = np.nan
    cells, _ = R.histograms(flow, None, P, 16)
    assert cells[1, ..., R.N].sum() == 0 and cells[1, ..., R.NBAD].sum() == h * w and cells[0, ..., R.N].sum() == h * w - 1


def test_descriptors_against_numpy():
    torch = pytest.importorskip("torch")
    from flowonthego_amd.histograms import HIST, motion_descriptors
    rng = np.random.default_rng(4)
    flow = (rng.standard_normal((1, 24, 40, 2)) * 2).astype(np.float32)
    cells, _ = R.histograms(flow, None, None, 8)
    cells[0, 0, 0] = 0                                  # an empty cell stays zero
    cells[0, 1, 1, 9:17] = 0                            # one empty part
    got = motion_descriptors(torch.from_numpy(cells)).numpy()
    want = R.descriptors(cells)
    assert len(HIST) == 32 and got.shape == cells.shape[:-1] + (25,) and got.dtype == np.float32
    assert np.allclose(got, want, rtol=1e-6, atol=0)
    assert not got[0, 0, 0].any() and not got[0, 1, 1, 9:17].any() and got[0, 1, 1, :9].any()
    for part in (slice(0, 9), slice(9, 17), slice(17, 25)):
        s = (got[0, 2, 2, part].astype(np.float64) ** 2).sum()
        assert abs(s - 1.0) < 1e-5


def test_cli_argument_errors():
    base = ["f.flo", "o.npz"]
    for args in ([], base[:1], base + ["extra"], base + ["--cell", "12"], base + ["--thresh", "-1"], base + ["--model", "rigid"],
                 base + ["--rows", "0"], base + ["--rows", "1025"], base + ["--mask"], base + ["--nosuch"]):
        r = run_cli("motion_histograms", args)
        assert r.returncode != 0 and "usage" in r.stderr, args
