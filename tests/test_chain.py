"""CPU tests of the restatement of flow chaining (tests/chain_ref.py, the definition of csrc/chain.hip.h in numpy float32): what
a chain is on flows whose answer is known in closed form, that no input value raises, and that the seeded inputs of the GPU
comparison (tests/test_gpu_chain.py) exercise every final code and every step count, so that comparison is not vacuous."""
import warnings

import numpy as np
import pytest

import chain_ref as R

f32 = np.float32


def test_constant_flow_adds_up_exactly_and_leaves_with_the_right_step_count():
    w, h, T = 40, 30, 6
    F = np.empty((T, h, w, 2), f32)
    F[...] = (1.5, -0.5)                                     # multiples of 0.5: every sum is exact in f32
    total, code, steps = R.chain(F)
    ys, xs = np.mgrid[0:h, 0:w]
    # the chain from (x, y) makes step k iff x + 1.5 (k+1) <= w-1 and y - 0.5 (k+1) >= 0
    n = np.minimum(np.floor((w - 1 - xs) / 1.5), np.floor(ys / 0.5)).astype(np.int64)
    want_steps = np.minimum(n, T)
    assert np.array_equal(steps, want_steps)
    assert np.array_equal(code, np.where(n >= T, 0, 2))
    assert (code == 0).any() and (code == 2).any() and set(np.unique(steps)) == set(range(T + 1))
    assert np.array_equal(total[..., 0], (1.5 * want_steps).astype(f32)) and np.array_equal(total[..., 1], (-0.5 * want_steps).astype(f32))
    assert np.array_equal(total[code == 0], np.broadcast_to(f32([1.5 * T, -0.5 * T]), ((code == 0).sum(), 2)))


def test_zero_flow_is_the_identity():
    F = np.zeros((4, 9, 11, 2), f32)
    total, code, steps = R.chain(F, F)
    assert not total.any() and not code.any() and (steps == 4).all()
    pts = np.array([[0.25, 3.5], [10, 8], [0, 0]], f32)
    traj, code, steps, disp = R.track(pts, F)
    assert np.array_equal(traj, np.broadcast_to(pts, (5, 3, 2))) and not code.any() and (steps == 4).all()


def test_a_flow_followed_by_its_negative_returns():
    w, h = 24, 16
    rng = np.random.default_rng(1)
    F0 = np.empty((h, w, 2), f32)
    F0[...] = rng.integers(-3, 4, 2).astype(f32) * f32(0.25) + f32((2.25, 1.5))       # one vector, a multiple of 0.25
    F = np.stack([F0, -F0])
    total, code, steps = R.chain(F)
    back = code == 0
    assert back.any() and (steps[back] == 2).all()
    assert not total[back].any()                             # exactly (0, 0)
    assert (code[~back] == 2).all() and (steps[~back] == 0).all()
    # with the exact backward flows every step is consistent: the same chains
    t2, c2, s2 = R.chain(F, np.stack([-F0, F0]))
    assert np.array_equal(c2, code) and np.array_equal(t2, total) and np.array_equal(s2, steps)


def test_bad_values_never_raise_and_end_as_unknown_or_outside():
    w, h, T = 13, 7, 3
    for bad, want in ((np.nan, 3), (np.inf, 3), (-np.inf, 3), (1e30, 2), (-1e30, 2), (3e38, None)):
        F = np.full((T, h, w, 2), f32(bad))
        with warnings.catch_warnings():
            warnings.simplefilter("error")                   # not even a RuntimeWarning
            total, code, steps = R.chain(F, F)
            traj, pc, ps, _ = R.track(np.array([[bad, 1], [1, bad], [2, 2]], f32), F, F)
        assert set(np.unique(code)) <= {2, 3} and not steps.any() and not total.any()
        if want is not None:
            assert (code == want).all()
        assert pc[2] in (2, 3) and (pc[:2] == (3 if not np.isfinite(f32(bad)) else 2)).all()
    # one bad vector poisons the chains whose taps touch it, nothing else
    F = np.zeros((2, h, w, 2), f32)
    F[1, 3, 5] = (np.nan, 0)
    total, code, steps = R.chain(F)
    bad = np.zeros((h, w), bool)
    bad[2:4, 4:6] = True                                     # the pixels with (5, 3) among their four taps (weight 0 included)
    assert np.array_equal(code == 3, bad) and (steps[bad] == 1).all() and (steps[~bad] == 2).all()


def test_one_step_from_integer_starts_is_the_flow_and_the_consistency_mask():
    import fbcheck_ref as FB
    rng = np.random.default_rng(5)
    h, w = 19, 27
    F = (rng.standard_normal((h, w, 2)) * 3).astype(f32)
    B = (rng.standard_normal((h, w, 2)) * 3).astype(f32)
    B[: h // 2] = -F[: h // 2]
    F[4, 5] = (1e30, 0)
    B[7, 3:9] = np.nan
    total, code, steps = R.chain(F[None], B[None])
    assert np.array_equal(code, FB.fb_code(F, B)) and len(np.unique(code)) == 3
    assert (total[code == 0] == F[code == 0]).all() and (steps == (code == 0)).all()
    # a non-finite vector makes the three pixels that have it as a weight-0 tap unknown as well; every other pixel is fb_check's
    F[10, 10] = (np.nan, 1)
    total, code, steps = R.chain(F[None], B[None])
    fb = FB.fb_code(F, B)
    differ = code != fb
    assert differ.sum() <= 3 and (code[differ] == 3).all() and differ[9:11, 9:11].sum() == differ.sum()


@pytest.mark.parametrize("w,h,n_seq,T,bw", R.CASES)
def test_the_seeded_inputs_cover_every_code_and_step_count(w, h, n_seq, T, bw):
    F, B = R.make_flows(w, h, n_seq, T)
    res = [R.chain(F[s], B[s] if bw else None) for s in range(n_seq)]
    code = np.concatenate([r[1].ravel() for r in res])
    steps = np.concatenate([r[2].ravel() for r in res])
    share = np.bincount(code, minlength=4) / code.size
    have = np.bincount(steps, minlength=T + 1) > 0
    print(w, h, n_seq, T, bw, share, np.bincount(steps, minlength=T + 1))
    assert (share[[0, 2, 3]] >= 0.01).all(), share
    assert share[1] >= 0.01 if bw else share[1] == 0, share  # without backward flows nothing can be called occluded
    assert have.all(), have
    # targets exactly on the last column and row are among the accepted first steps
    t1 = R.chain(F[0, :1])[0]
    ys, xs = np.mgrid[0:h, 0:w]
    assert ((xs + t1[..., 0] == w - 1) & (t1[..., 0] > 0)).any() and ((ys + t1[..., 1] == h - 1) & (t1[..., 1] > 0)).any()


def test_the_point_inputs_cover_every_start():
    for w, h in R.SIZES[:2]:
        F, B = R.make_flows(w, h, 1, 5)
        pts = R.make_points(w, h, 1, 300)[0]
        traj, code, steps, disp = R.track(pts, F[0], B[0])
        assert (np.bincount(code, minlength=4) > 0).all() and (np.bincount(steps, minlength=6) > 0).all()
        start_out = ~np.isfinite(pts).all(1) | ~R.inside(pts[:, 0], pts[:, 1], w, h)
        assert start_out.sum() >= 8 and (steps[start_out] == 0).all() and (code[start_out] >= 2).all()
        assert np.array_equal(traj[0].view(np.uint32), pts.view(np.uint32))
        fin = np.isfinite(pts).all(1)
        assert np.array_equal(traj[5][fin], (pts + disp)[fin])
        assert R.stats(code, steps)[:4].sum() == 300 and R.stats(code, steps)[4] == steps.sum()
