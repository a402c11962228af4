"""The global-motion fit's definition (tests/motion_ref.py, the numpy restatement of csrc/motion.hip.h) has the properties the
feature is for: exact on exact inputs, accurate to the quantisation on clean ones, robust to independently moving pixels, sums that
do not depend on the order, degenerate systems that clear `fitted`, and -- on flows of the CPU oracle -- the camera's true steps.
The GPU kernels are compared with this restatement byte for byte in tests/test_gpu_motion.py."""
import numpy as np
import pytest

import motion_ref as R

f32 = np.float32

# a motion per model, as [a00 a01 tx a10 a11 ty]
MOTIONS = {0: [0.0, 0.0, 3.25, 0.0, 0.0, -1.5],
           1: [0.012, -0.007, -2.0, 0.007, 0.012, 4.5],
           2: [0.004, -0.011, 1.75, 0.009, 0.006, -2.5]}


def test_constant_integer_flow_is_fitted_exactly():
    for w, h in ((67, 45), (1, 1), (5, 1)):
        flow = np.empty((h, w, 2), f32)
        flow[...] = (7.0, -3.0)
        for iters in (0, 3):
            r = R.fit(flow, None, 0, iters)
            assert np.array_equal(r["params"], [0.0, 0.0, 7.0, 0.0, 0.0, -3.0]) and r["stats"][5] == 1
            assert (r["code"] == 0).all() and not r["residual"].any()
    # the richer models find the same motion, A to rounding
    flow = np.empty((45, 67, 2), f32)
    flow[...] = (7.0, -3.0)
    for model in (1, 2):
        assert R.corner_error(R.fit(flow, None, model)["params"], [0, 0, 7.0, 0, 0, -3.0], 67, 45) < 1e-9


@pytest.mark.parametrize("model", [0, 1, 2])
def test_fit_of_a_motion_flow_reproduces_the_motion(model):
    """quantisation to 1/256 px is an error of at most 1/512 px per sample; at a corner of a uniform grid least squares amplifies
    a per-sample error by at most the mean of |1 + 3x + 3y| over [-1, 1]^2 = 2.16: 4/512 = 1/128 px bounds the corner error"""
    for w, h in ((67, 45), (640, 420)):
        P = MOTIONS[model]
        flow = R.motion_flow(P, w, h)
        for iters in (0, 3):
            r = R.fit(flow, None, model, iters)
            err = R.corner_error(r["params"], P, w, h)
            print("model %d %dx%d iters %d: corner error %.6f px" % (model, w, h, iters, err))
            assert err <= 1.0 / 128 and r["stats"][5] == 1 and r["stats"][0] == w * h
            # the residual is the flow minus the motion's flow, bit for bit
            assert np.array_equal(r["residual"], flow - R.motion_flow(r["params"], w, h))


@pytest.mark.parametrize("w,h", [(67, 45), (320, 192)])
def test_three_rounds_beat_plain_least_squares(w, h):
    flow, _, P = R.make_scene(w, h, seed=3, specials=False)
    plain = R.corner_error(R.fit(flow, None, 2, 0)["params"], P, w, h)
    robust = R.fit(flow, None, 2, 3)
    err = R.corner_error(robust["params"], P, w, h)
    print("%dx%d: corner error plain %.4f px, three rounds %.4f px; pixels in the last fit %.3f" %
          (w, h, plain, err, robust["stats"][4] / (w * h)))
    assert err < plain
    # the block that moves on its own is what the code calls independent
    assert 0.2 < (robust["code"] == 1).mean() < 0.3


def test_sums_do_not_depend_on_the_order():
    flow, mask, _ = R.make_scene(67, 45, seed=5)
    X, Y = R.coords(67, 45)
    k = R.known(flow)
    U, V = R.fixed_point(flow, k)
    sel = k & (mask == 0)
    want = R.sums(X, Y, U, V, sel)
    perm = np.random.default_rng(0).permutation(67 * 45)
    got = R.sums(*(a.reshape(-1)[perm] for a in (X, Y, U, V)), sel.reshape(-1)[perm])
    parts = [R.sums(*(a.reshape(-1)[i::7] for a in (X, Y, U, V)), sel.reshape(-1)[i::7]) for i in range(7)]
    assert got == want and [sum(p[j] for p in parts) for j in range(12)] == want
    assert want[0] == sel.sum() and want[1] == X[sel].sum()


def test_codes_and_counts():
    flow, mask, _ = R.make_scene(67, 45, seed=5)
    r = R.fit(flow, mask, 2, 3)
    code, st = r["code"], r["stats"]
    assert all((code == c).any() for c in range(4)) and st[:4].sum() == 67 * 45 and st[5] == 1
    assert np.array_equal(code == 3, ~R.known(flow)) and (code == 3).sum() == 6          # (4096, -4096) is known
    assert np.array_equal(code == 2, R.known(flow) & (mask != 0))
    assert 0 < st[4] <= st[0] + st[1]


def test_degenerate_systems_clear_fitted():
    flow, _, _ = R.make_scene(67, 45, seed=5, specials=False)
    for model in (0, 1, 2):
        r = R.fit(flow, np.ones((45, 67), np.uint8), model, 3)                           # everything masked
        assert r["stats"][5] == 0 and r["stats"][4] == 0 and not r["params"].any() and (r["code"] == 2).all()
    one = np.full((1, 1, 2), 2.5, f32)
    assert R.fit(one, None, 0)["stats"][5] == 1                                          # one pixel is a translation ...
    for model in (1, 2):                                                                 # ... and nothing more: D = det = 0
        r = R.fit(one, None, model)
        assert r["stats"][5] == 0 and not r["params"].any()
    row = R.motion_flow(MOTIONS[1], 33, 1)
    r = R.fit(row, None, 2)                                                              # h = 1: Y = 0 everywhere, det is exactly 0
    assert r["stats"][5] == 0 and not r["params"].any() and r["sums"][5] == 0
    assert R.fit(row, None, 1)["stats"][5] == 1                                          # a similarity is determined by a row
    # a later round that loses its pixels keeps the earlier parameters and clears fitted
    far = np.zeros((8, 8, 2), f32)
    far[:, :4] = 40.0
    r = R.fit(far, None, 0, 1, thresh=1.0)
    assert r["stats"][5] == 0 and np.array_equal(r["params"], [0, 0, 20.0, 0, 0, 20.0]) and r["stats"][4] == 0


# ---- flows of the oracle ------------------------------------------------------------------------------------------------------
_FLOWS = {}


def oracle_flows(natural_images, patch):
    if patch not in _FLOWS:
        from oracle import oracle as O
        frames, off = R.jittered_crops(natural_images["road_HD"], patch=patch)
        fr = frames.astype(f32)
        _FLOWS[patch] = (np.stack([O.full_flow(fr[k], fr[k + 1], op=2) for k in range(len(fr) - 1)]), off)
    return _FLOWS[patch]


def test_translations_of_jittered_crops_round_to_the_true_steps(natural_images):
    flows, off = oracle_flows(natural_images, False)
    worst = 0.0
    for k, F in enumerate(flows):
        true = (off[k] - off[k + 1]).astype(np.float64)
        t = R.fit(F, None, 0, 3)["params"][[2, 5]]
        worst = max(worst, float(np.abs(t - true).max()))
        assert np.array_equal(np.rint(t), true), (k, t, true)
    print("worst translation error over %d pairs: %.4f px" % (len(flows), worst))
    assert any((off[k] != off[k + 1]).any() for k in range(len(flows)))


def test_robust_translation_beats_the_mean_flow_with_a_moving_patch(natural_images):
    flows, off = oracle_flows(natural_images, True)
    e_robust = e_mean = 0.0
    for k, F in enumerate(flows):
        true = (off[k] - off[k + 1]).astype(np.float64)
        er = float(np.hypot(*(R.fit(F, None, 0, 3)["params"][[2, 5]] - true)))
        em = float(np.hypot(*(R.fit(F, None, 0, 0)["params"][[2, 5]] - true)))
        print("pair %d: robust %.4f px, mean flow %.4f px" % (k, er, em))
        e_robust += er
        e_mean += em
    assert e_robust < e_mean


# ---- the camera path -----------------------------------------------------------------------------------------------------------
def test_path_of_integer_translations_is_the_smoothed_offset():
    off = np.array([[0, 0], [6, 0], [6, -6], [0, -6], [-6, -12], [-6, -12], [0, -6]], np.float64)
    params = np.zeros((6, 6))
    params[:, [2, 5]] = off[:-1] - off[1:]
    W = R.smoothing_motions(params, 1)
    smooth = np.array([off[max(k - 1, 0):k + 2].mean(0) for k in range(7)])
    assert np.array_equal(W[:, [2, 5]], smooth - off) and not W[:, [0, 1, 3, 4]].any()
    assert np.array_equal(smooth, np.rint(smooth))                       # multiples of 6: every window mean is an integer
    assert not R.smoothing_motions(params, 0).any()                       # no smoothing: every frame stays


def test_path_algebra():
    rng = np.random.default_rng(11)
    params = rng.standard_normal((9, 6)) * np.array([0.01, 0.01, 3.0, 0.01, 0.01, 3.0])
    W = R.smoothing_motions(params, 2)
    # the same with 3 x 3 matrices and numpy's linear algebra
    M = [np.array([[1 + p[0], p[1], p[2]], [p[3], 1 + p[4], p[5]], [0, 0, 1]]) for p in params]
    C = [np.eye(3)]
    for m in M:
        C.append(m @ C[-1])
    for k in range(10):
        S = np.mean(C[max(k - 2, 0):k + 3], axis=0)
        want = C[k] @ np.linalg.inv(S) - np.eye(3)
        assert np.allclose(W[k], want[:2].ravel(), rtol=1e-12, atol=1e-12)
    assert np.abs(R.smoothing_motions(params, 100) - R.smoothing_motions(params, 9)).max() == 0   # a radius beyond the sequence
