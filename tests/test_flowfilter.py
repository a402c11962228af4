"""The flow filter's definition on the CPU (no GPU needed): the numpy restatement tests/flowfilter_ref.py, which the GPU tests compare
the kernel with byte for byte, has the properties the definition promises, and does what the filter is for on a synthetic scene.

The 4 ulp of the constant-flow cases is the bound the definition's issue set, not a measurement.  It is also what the arithmetic
gives: with F = c everywhere, nu = sum fl(wt c) and den = sum wt run over the same weights in the same order, so the rounding
errors of the two sums are almost the same relative perturbation and cancel in nu / den; what is left is one rounding per product,
one per division and the uncorrelated part of the partial-sum roundings."""
import numpy as np

import flowfilter_ref as R

f32 = np.float32


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def ulps(a, b):
    """|a - b| in units of the last place of b (f32, same sign, finite)"""
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def noisy_guide(rng, h, w, noc):
    g = rng.integers(0, 256, (h, w, noc)).astype(f32) + rng.random((h, w, noc)).astype(f32)
    return g[..., 0] if noc == 1 else g


def test_a_constant_flow_comes_back():
    rng = np.random.default_rng(1)
    h, w = 17, 23
    vec = np.array([1.7, -3.3], f32)
    flow = np.broadcast_to(vec, (h, w, 2)).copy()
    for noc in (1, 3):
        guide = noisy_guide(rng, h, w, noc)
        mask = rng.choice(np.array([0, 0, 0, 1, 2, 3, 9], np.uint8), (h, w))
        for m, iters in ((None, 1), (mask, 1), (mask, 2)):
            out, code, st, terms = R.filter_one(flow, guide, m, 2, R.spatial_table(2, 1.0), 30.0, iters, terms=True)
            sup = code != 3
            assert sup.any() and ulps(out[sup], flow[sup]).max() <= 4
            assert bits_equal(out[~sup], flow[~sup])
            if m is None:
                assert (code == 0).all() and st[0] == h * w
                assert st[3] < w * h * 8 * 2.0 ** -23 * float(np.abs(vec).sum())
            else:
                assert np.array_equal(code == 0, mask == 0)          # a valid centre always supports itself


def test_a_constant_guide_gives_the_window_mean_clipped_to_the_image():
    rng = np.random.default_rng(2)
    h, w, radius = 9, 11, 2
    flow = rng.integers(-8, 9, (h, w, 2)).astype(f32)              # small integers: every order of adding is exact
    for guide in (np.full((h, w), 77, np.uint8), np.full((h, w, 3), 5.5, f32)):
        out, code, st = R.filter_one(flow, guide, None, radius, None, 20.0)
        want = np.zeros_like(flow)
        for y in range(h):
            for x in range(w):
                win = flow[max(0, y - radius):y + radius + 1, max(0, x - radius):x + radius + 1].reshape(-1, 2)
                want[y, x] = win.sum(0, dtype=f32) / f32(len(win))
        assert bits_equal(out, want) and (code == 0).all()
    assert bits_equal(R.filter_one(flow[:1, :1], np.zeros((1, 1), f32), None, 7, None, 1.0)[0], flow[:1, :1])


def test_no_vector_crosses_a_guide_step_larger_than_tau_times_channels():
    h, w, tau = 12, 20, 10.0
    left, right = np.array([2.5, -1.25], f32), np.array([-4.0, 7.5], f32)
    flow = np.where((np.arange(w) < 9)[None, :, None], left, right).astype(f32)
    flow = np.broadcast_to(flow, (h, w, 2)).copy()
    for noc in (1, 3):
        step = np.where(np.arange(w) < 9, 40.0, 40.0 + tau * noc + 1.0).astype(f32)         # larger than tau * channels in the sum
        guide = np.broadcast_to(step[None, :, None] if noc == 3 else step[None, :], (h, w, 3) if noc == 3 else (h, w)).copy()
        if noc == 3:
            guide[..., 1:] = 40.0                                  # the whole step sits in one channel
        out, code, _ = R.filter_one(flow, guide, None, 3, R.spatial_table(3, 1.5), tau)
        assert (code == 0).all() and ulps(out, flow).max() <= 4
        # the same flow against a guide without the step is mixed across the discontinuity
        flat, _, _ = R.filter_one(flow, np.full_like(guide, 40.0), None, 3, R.spatial_table(3, 1.5), tau)
        assert np.abs(flat[:, 6:12] - flow[:, 6:12]).min() > 0.05
        assert ulps(flat[:, :5], flow[:, :5]).max() <= 4


def test_masked_pixels_are_filled_and_an_island_shrinks_by_the_radius_per_pass():
    rng = np.random.default_rng(4)
    h, w, radius = 30, 40, 2
    flow = rng.integers(-8, 9, (h, w, 2)).astype(f32)
    guide = np.full((h, w), 100.0, f32)
    mask = np.zeros((h, w), np.uint8)
    mask[5:25, 10:31] = 1                                          # 20 x 21, wider than 2 radius + 1
    mask[2, 3] = 3
    garbage = flow.copy()
    garbage[mask != 0] = 1e6
    out, code, _ = R.filter_one(garbage, guide, mask, radius, None, 20.0)
    # a masked pixel with support: code 1 and the mean of the unmasked vectors of its window
    assert code[2, 3] == 1 and code[5, 10] == 1
    win, mw = flow[3:8, 8:13].reshape(-1, 2), (mask[3:8, 8:13] == 0).ravel()
    assert bits_equal(out[5, 10], win[mw].sum(0, dtype=f32) / f32(mw.sum()))
    for k in range(1, 5):
        out, code, st = R.filter_one(garbage, guide, mask, radius, None, 20.0, iters=k)
        want3 = np.zeros((h, w), bool)
        want3[5 + radius * k:25 - radius * k, 10 + radius * k:31 - radius * k] = True
        assert np.array_equal(code == 3, want3), k
        assert bits_equal(out[want3], garbage[want3])              # passed through bit for bit
        assert np.array_equal(code == 0, mask == 0) and st[2] == want3.sum()
        assert np.abs(out[~want3]).max() <= 8                      # no garbage leaked


def test_iters_equals_single_passes_composed_by_hand():
    rng = np.random.default_rng(5)
    h, w = 21, 33
    flow = (rng.standard_normal((h, w, 2)) * 3).astype(f32)
    flow[3, 4] = (np.nan, 1.0)
    flow[10, 20] = (3e38, -3e38)
    guide = noisy_guide(rng, h, w, 3) / f32(4)
    mask = rng.choice(np.array([0, 0, 1], np.uint8), (h, w))
    mask[6:16, 8:22] = 1
    s = R.spatial_table(2, 1.0)
    cur, m, first = flow, mask, None
    for k in range(1, 5):
        cur, cd, _ = R.filter_one(cur, guide, m, 2, s, 30.0)
        first = cd if first is None else first
        m = (cd == 3).astype(np.uint8)
        final = np.where(cd == 3, 3, np.where(first == 0, 0, 1)).astype(np.uint8)
        out, code, _ = R.filter_one(flow, guide, mask, 2, s, 30.0, iters=k)
        assert R.same_but_nan(out, cur) and np.array_equal(code, final), k


def test_non_finite_vectors_and_mask_bytes_above_3_are_invalid():
    h, w = 9, 9
    flow = np.ones((h, w, 2), f32)
    guide = np.zeros((h, w), f32)
    for bad in ((np.nan, 1.0), (1.0, np.inf), (-np.inf, np.nan)):
        f = flow.copy()
        f[4, 4] = bad
        out, code, _ = R.filter_one(f, guide, None, 1, None, 20.0)
        assert code[4, 4] == 1 and (np.delete(code.ravel(), 40) == 0).all() and bits_equal(out, flow)
        f[3:6, 3:6] = bad                                          # no valid vector within the radius of the centre
        out, code, _ = R.filter_one(f, guide, None, 1, None, 20.0)
        assert code[4, 4] == 3 and R.same_but_nan(out[4, 4], np.array(bad, f32)) and (out[code != 3] == 1).all()
    mask = np.zeros((h, w), np.uint8)
    mask[4, 4], mask[0, 0], mask[8, 8] = 4, 200, 255
    f = flow.copy()
    f[mask != 0] = 50.0
    out, code, st = R.filter_one(f, guide, mask, 1, None, 20.0)
    assert np.array_equal(code == 1, mask != 0) and bits_equal(out, flow) and st.tolist() == [78.0, 3.0, 0.0, 0.0]


def test_the_filter_repairs_the_synthetic_scene():
    """Measured on the restatement (96 x 128, seed 11, radius 5, sigma 3, tau 20, two passes), mean EPE before -> after:
    whole frame 0.9332 -> 0.1491 px, the 8-pixel belt round the boundary 1.6830 -> 0.9872 px, the occluded band 28.6575 -> 0.1169 px;
    after one pass 60 of the 280 masked pixels are without support, after two none.  Each "after" is asserted against the measured
    value plus a quarter of the measured improvement."""
    true, bad, guide, mask, regions = R.quality_scene()
    q = R.QUALITY
    s = R.spatial_table(q["radius"], q["sigma"])
    one = R.filter_one(bad, guide, mask, q["radius"], s, q["tau"], 1)
    out, code, st = R.filter_one(bad, guide, mask, q["radius"], s, q["tau"], q["iters"])
    measured = dict(all=(0.9332, 0.1491), belt=(1.6830, 0.9872), band=(28.6575, 0.1169))
    for k, m in regions.items():
        before, after = R.epe(bad, true, m), R.epe(out, true, m)
        print("EPE %s: before %.4f after %.4f" % (k, before, after))
        b0, a0 = measured[k]
        assert abs(before - b0) < 0.01 * b0
        assert after <= a0 + 0.25 * (b0 - a0), k
    assert one[2][2] == 60 and st[2] == 0 and st[1] == mask.sum() == 280
