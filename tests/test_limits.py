"""The closed forms of tests/limits_ref.py equal the restatements (motion_ref, layers_ref, objects_ref, tracks_ref, morph_ref) on the
materialised input at small sizes, and reach the magnitudes the headers promise at 16384 x 16384: |sum XU| = 2^61 (the top of
motion.hip.h's range is 2^62), sum U = 2^48 and area = 2^28 (components.hip.h), 2^28 votes (objtracks.hip.h, int32).  CPU only."""
import numpy as np
import pytest

import layers_ref as LR
import limits_ref as X
import morph_ref as MR
import motion_ref as M
import objects_ref as OR
import tracks_ref as TR

f32 = np.float32
SIZES = [(37, 21), (64, 48), (1, 1), (2, 2), (33, 1), (1, 18)]            # (w, h)


def f64_bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


def random_profiles(w, h, seed):
    rng = np.random.default_rng(seed)
    ux, vy = (rng.uniform(-4096, 4096, w)).astype(f32), (rng.uniform(-4096, 4096, h)).astype(f32)
    ux[rng.integers(w)], vy[rng.integers(h)] = f32(4096), f32(-4096)
    return ux, vy


@pytest.mark.parametrize("w,h", SIZES)
def test_separable_sums_equal_the_restatement(w, h):
    for ux, vy in (X.sgn_profiles(w, h), random_profiles(w, h, 3)):
        flow = X.materialise(ux, vy)
        Xc, Yc = M.coords(w, h)
        U, V = M.fixed_point(flow, M.known(flow))
        assert X.separable_sums(ux, vy) == M.sums(Xc, Yc, U, V, np.ones((h, w), bool))
        selx, sely = np.arange(w) % 3 != 1, np.arange(h) % 2 == 0
        assert X.separable_sums(ux, vy, selx, sely) == M.sums(Xc, Yc, U, V, selx[None, :] & sely[:, None])


@pytest.mark.parametrize("w,h", SIZES)
def test_motion_closed_form_equals_the_restatement(w, h):
    ux, vy = X.sgn_profiles(w, h)
    flow = X.materialise(ux, vy)
    for model in (0, 1, 2):
        for thresh in (1.0, 3000.0, 8192.0):                 # few pixels follow, a band of them, all of them
            want = M.fit(flow, None, model, 0, thresh)
            got = X.motion_expected(ux, vy, model, thresh)
            assert got["sums"] == want["sums"].tolist() and got["stats"] == want["stats"].tolist(), (model, thresh)
            assert np.array_equal(f64_bits(got["params"]), f64_bits(want["params"])), (model, thresh)
        want = M.fit(flow, X.corner_mask(w, h), model, 3, 1.0)
        got = X.motion_corners_expected(ux, vy, model, 3, 1.0)
        assert got["sums"] == want["sums"].tolist() and got["stats"] == want["stats"].tolist(), model
        assert np.array_equal(f64_bits(got["params"]), f64_bits(want["params"])), model


@pytest.mark.parametrize("w,h", SIZES)
def test_layers_closed_form_equals_the_restatement(w, h):
    ux, vy = X.sgn_profiles(w, h)
    flow = X.materialise(ux, vy)
    for model in (0, 1, 2):
        for rounds in (0, 1):
            for thresh in (1.0, 3000.0, 8192.0):
                want = LR.layers(flow, None, 1, model, 0, rounds, thresh)
                got = X.layers_expected(ux, vy, model, rounds, thresh)
                for k in ("sums", "records", "stats"):
                    assert np.array_equal(np.array(got[k], np.int64), want[k]), (model, rounds, thresh, k, got[k], want[k])
                assert np.array_equal(f64_bits(got["params"]), f64_bits(want["params"])), (model, rounds, thresh)
                if rounds == 0:                              # layer 0 without refinement is the motion fit
                    fit = X.motion_expected(ux, vy, model, thresh)
                    assert got["sums"][0] == fit["sums"] and got["params"][0] == fit["params"]


@pytest.mark.parametrize("w,h", [(37, 21), (64, 48), (1, 1), (2, 2), (16, 3)])
def test_components_closed_form_equals_the_restatement(w, h):
    values = np.empty((h, w, 2), f32)
    values[:] = (X.VALUE_U, X.VALUE_V)
    for pattern in X.PATTERNS:
        code = X.component_map(pattern, w, h)
        for max_objects in (4, 64):
            got = X.components_expected(pattern, w, h, max_objects)
            labels, ids = X.component_labels(pattern, w, h, max_objects)
            for conn in (4, 8):
                want = OR.components(code, OR.fg_set((1,)), conn, values, 1, max_objects)
                assert np.array_equal(got["objects"], want["objects"]), (pattern, conn)
                assert got["stats"] == want["stats"].tolist(), (pattern, conn)
                assert np.array_equal(np.broadcast_to(labels, (h, w)), want["labels"]), (pattern, conn)
                assert np.array_equal(np.broadcast_to(ids, (h, w)), want["ids"]), (pattern, conn)


@pytest.mark.parametrize("w,h", [(37, 21), (64, 48), (1, 1)])
def test_votes_closed_form_equals_the_restatement(w, h):
    ids = np.zeros((h, w), np.int32)
    for u, v in ((0.0, 0.0), (float(w), 0.0), (3.4, -2.5), (-5.0, 7.0), (4096.0, 0.0), (4097.0, 0.0), (16384.0, 0.0), (0.0, np.inf)):
        for masked in (False, True):
            flow = np.empty((h, w, 2), f32)
            flow[:] = (u, v)
            want = TR.overlap(ids, ids, flow, np.ones((h, w), np.uint8) if masked else None, 2, 3)
            got = X.votes_expected(w, h, u, v, masked, 2, 3)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (u, v, masked)


@pytest.mark.parametrize("w,h", [(37, 21), (64, 48), (1, 1)])
def test_morphology_closed_form_equals_the_restatement(w, h):
    x = X.pinhole_map(w, h)
    for op in X.MORPH_OPS:
        for r in (1, 8):
            out, stats = MR.morphology(x, op, r)
            assert X.pinhole_expected(w, h, op, r) == stats.tolist(), (op, r)
            for uniform in (0, 1):                          # a uniform map is its own erosion and dilation: the border does not erode
                u = np.full((h, w), uniform, np.uint8)
                assert np.array_equal(MR.morphology(u, op, r)[0], u)


def test_the_magnitudes_at_the_limit():
    n = X.LIMIT
    ux, vy = X.sgn_profiles(n, n)
    S = X.separable_sums(ux, vy)
    print("n = 2^%d, |sum XU| = 2^%d, |sum YV| = 2^%d, sum XX = %d" % (S[0].bit_length() - 1, abs(S[7]).bit_length() - 1,
                                                                       abs(S[11]).bit_length() - 1, S[3]))
    assert S[0] == 1 << 28 and S[7] == 1 << 61 and S[11] == -(1 << 61) and max(abs(s) for s in S) < 1 << 62
    assert S[1] == S[2] == S[4] == S[6] == S[8] == S[9] == S[10] == 0 and S[3] == S[5] == n * (n * (n * n - 1) // 3)
    # the sanity check of the tests themselves: a product X * U narrowed to 32 bits gives other sums on this very input
    X1 = 2 * np.arange(n, dtype=np.int64) - (n - 1)
    U1 = np.rint(ux * f32(256)).astype(np.int64)
    narrow = int((X1 * U1).astype(np.int32).astype(np.int64).sum()) * n
    print("sum XU with a 32-bit product: %d" % narrow)
    assert narrow != S[7]
    obj = X.components_expected("all", n, n, 4)["objects"][0]
    print("components: area = 2^%d, sum x = %d < 2^42, sum U = 2^%d" % (int(obj[1]).bit_length() - 1, obj[6], int(obj[9]).bit_length() - 1))
    assert obj[1] == obj[8] == 1 << 28 and obj[9] == 1 << 48 and obj[10] == -(1 << 48)
    assert obj[6] == obj[7] == (1 << 14) * ((1 << 14) * ((1 << 14) - 1) // 2) < 1 << 42
    for pattern in ("rows", "columns"):
        e = X.components_expected(pattern, n, n, 65536)
        assert e["stats"] == [1 << 27, 8192, 8192, 8192] and (e["objects"][:8192, 1] == n).all() and not e["objects"][8192:].any()
    votes, sent = X.votes_expected(n, n, 0.0, 0.0, False, 2, 2)
    assert votes[0, 0] == 1 << 28 and sent[0].tolist() == [1 << 28, 0, 0, 0]
    assert X.votes_expected(n, n, 16384.0, 0.0, False, 2, 2)[1][0].tolist() == [0, 0, 0, 1 << 28]      # beyond +-4096: inadmissible
    assert X.votes_expected(n, n, 4096.0, -4096.0, False, 2, 2)[1][0].tolist() == [9 << 24, 0, 7 << 24, 0]
    assert X.votes_expected(n, n, 0.0, 0.0, True, 2, 2)[1][0].tolist() == [0, 0, 0, 1 << 28]
    assert X.pinhole_expected(n, n, "erode", 8) == [(1 << 28) - 1, (1 << 28) - X.quarter_disc(8, n, n), 0, X.quarter_disc(8, n, n) - 1]
