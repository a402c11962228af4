"""The motion-compensated temporal filter's definition on the CPU (no GPU needed): the numpy restatement tests/temporal_ref.py, which
the GPU tests compare the kernel with byte for byte, has the properties the definition promises, and filtering along the flows of
the CPU oracle does what the filter is for.

The quality bound is derived, not tuned: the mean of three aligned frames with independent noise of equal variance has a third of
the variance, 10 log10(3) = 4.77 dB; the weights fall short of 1 and the flows of noisy frames are not exact, so the test asks for
3 dB.  Measured on the restatement (alley_1 frames 1-3, crop [100:356, 300:812], sigma 10, tau 30): noisy 28.41 dB, filtered along
the flows 33.71 dB (+5.30 dB), the same filter with zero flows 31.27 dB, the plain three-frame mean 26.75 dB."""
import numpy as np

import temporal_ref as R

f32 = np.float32


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_identical_neighbour_with_a_zero_flow_returns_the_centre():
    rng = np.random.default_rng(1)
    for shape in ((2, 9, 13), (2, 9, 13, 3)):
        img = (rng.integers(0, 256, shape[1:]) + rng.random(shape[1:])).astype(f32)
        frames = np.stack([img, img])
        dst, used, st = R.filter_one(frames, 0, [1], np.zeros((1, 9, 13, 2), f32), tau=30.0, ref=img)
        assert bits_equal(dst, img)                      # (C + 1 * C) / 2
        assert (used == 1).all() and st[0] == 9 * 13 and st[1] == 0 and st[2] == 0 and st[3] == 0
        u8 = frames.astype(np.uint8)
        dst, used, _ = R.filter_one(u8, 1, [0], np.zeros((1, 9, 13, 2), f32))
        assert bits_equal(dst, u8[1]) and (used == 1).all()


def test_absent_zero_gain_and_fully_masked_neighbours_are_left_out():
    rng = np.random.default_rng(2)
    T, h, w = 4, 17, 23
    for noc in (1, 3):
        ys, xs = np.mgrid[0:h, 0:w]
        base = (128 + 60 * np.sin(ys / 5.0) + 50 * np.cos(xs / 4.0)).astype(f32)         # smooth: a small flow changes it little
        frames = np.stack([base if noc == 1 else np.stack([base, base[::-1], base[:, ::-1]], -1)] * T)
        frames = (frames + rng.normal(0, 6, frames.shape)).astype(f32)
        flows = (rng.standard_normal((3, h, w, 2)) * 0.7).astype(f32)
        want = R.filter_one(frames, 0, [1, 3], flows[[0, 2]], tau=20.0, gains=[0.5, 2.0])
        assert want[1].min() == 0 and want[1].max() == 2
        absent = R.filter_one(frames, 0, [1, -1, 3], flows, tau=20.0, gains=[0.5, 1.0, 2.0])
        nogain = R.filter_one(frames, 0, [1, 2, 3], flows, tau=20.0, gains=[0.5, 0.0, 2.0])
        masks = np.zeros((3, h, w), np.uint8)
        masks[1] = 1
        masked = R.filter_one(frames, 0, [1, 2, 3], flows, masks=masks, tau=20.0, gains=[0.5, 1.0, 2.0])
        for got in (absent, nogain, masked):
            assert bits_equal(got[0], want[0]) and bits_equal(got[1], want[1]) and bits_equal(got[2], want[2])
        # the neighbour does count when nothing excludes it
        full = R.filter_one(frames, 0, [1, 2, 3], flows, tau=20.0, gains=[0.5, 1.0, 2.0])
        assert full[1].max() == 3 and not bits_equal(full[0], want[0])


def test_window_is_a_3x3_box_with_replicated_edges():
    rng = np.random.default_rng(3)
    d = rng.integers(0, 64, (6, 7)).astype(f32)          # small integers: every order of adding is exact
    p = np.pad(d, 1, mode="edge")
    want = sum(p[1 + dy:7 + dy, 1 + dx:8 + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1))
    assert np.array_equal(R.box3(d), want)
    assert R.box3(np.full((1, 1), 2, f32))[0, 0] == 18


def test_filtering_along_the_oracle_flows_denoises_alley():
    from oracle import oracle as O
    clean, noisy = R.quality_frames()
    h, w = clean.shape[1:]
    flows = np.stack([O.full_flow(noisy[1], noisy[0], op=2), O.full_flow(noisy[1], noisy[2], op=2)])
    along, used, st = R.filter_one(noisy, 1, [0, 2], flows, tau=R.QUALITY_TAU, ref=clean[1])
    still, _, _ = R.filter_one(noisy, 1, [0, 2], np.zeros_like(flows), tau=R.QUALITY_TAU)
    p_noisy, p_along, p_still = R.psnr(noisy[1], clean[1]), R.psnr(along, clean[1]), R.psnr(still, clean[1])
    p_mean = R.psnr(noisy.mean(axis=0), clean[1])
    print("PSNR of frame 2: noisy %.2f dB, filtered along the flows %.2f dB, with zero flows %.2f dB, plain mean %.2f dB; "
          "mean used %.3f" % (p_noisy, p_along, p_still, p_mean, used.mean()))
    assert p_along >= p_noisy + 3.0
    assert p_along > p_still
    # the statistics are the same residuals
    assert abs(st[2] / (h * w) - np.abs(clean[1] - along).mean()) < 1e-3 and st[3] > st[2]
