"""The motion layers' definition, checked on its numpy restatement alone (tests/layers_ref.py, no GPU): the three-motion scene is
separated into its three motions, a fourth layer finds nothing, layer 0 is the global-motion fit, and the corner cases of the
assignment -- init without rounds, duplicated layers, masked and unknown pixels -- come out as include/fotg.h words them."""
import numpy as np
import pytest

import layers_ref as L
import motion_ref as M


@pytest.fixture(scope="module", params=[(320, 192), (157, 93)], ids=["320x192", "157x93"])
def scene(request):
    w, h = request.param
    flow, truth, Ps = L.three_motions(w, h, seed=3, noise=0.2)
    return w, h, flow, truth, Ps, {K: L.layers(flow, layers=K) for K in (3, 4)}


def _match(out, Ps, w, h):
    """layer -> (the true motion nearest by corner error, that error), live layers only"""
    got = {}
    for k in range(len(out["params"])):
        if out["records"][k, 2]:
            errs = [M.corner_error(out["params"][k], P, w, h) for P in Ps]
            got[k] = (int(np.argmin(errs)), min(errs))
    return got


def test_three_motions_are_separated(scene):
    w, h, flow, truth, Ps, outs = scene
    out = outs[3]
    match = _match(out, Ps, w, h)
    assert sorted(t for t, _ in match.values()) == [0, 1, 2], match
    for k, (t, err) in match.items():
        share = float((out["labels"][truth == t] == k).mean())
        print("%d x %d layer %d: motion %d, corner error %.4f px, share %.4f" % (w, h, k, t, err, share))
        assert err <= 0.25 and share >= 0.99
    assert out["stats"][3] == 3 and out["records"][:, 0].sum() + out["stats"][:3].sum() == w * h


def test_a_fourth_layer_is_dead(scene):
    w, h, flow, truth, Ps, outs = scene
    a, b = outs[3], outs[4]
    assert np.array_equal(b["params"][:3].view(np.uint64), a["params"].view(np.uint64)) and np.array_equal(b["labels"], a["labels"])
    assert b["records"][3].tolist() == [0, 0, 0, 0, -1, 0, 0, 0] and not b["params"][3].any() and not b["sums"][3].any()
    assert b["stats"][3] == 3


def test_layer_zero_is_the_global_motion_fit(scene):
    w, h, flow, truth, Ps, outs = scene
    want = M.fit(flow)                                   # (the seeding's result: the refinement may move layer 0 with the others)
    assert np.array_equal(L.layers(flow, layers=3, rounds=0)["params"][0].view(np.uint64), want["params"].view(np.uint64))
    for model in (0, 1):
        for iters, thresh in ((0, 1.0), (2, 2.5)):
            got = L.layers(flow, layers=2, model=model, iters=iters, rounds=0, thresh=thresh)
            want = M.fit(flow, None, model, iters, thresh)
            assert np.array_equal(got["params"][0].view(np.uint64), want["params"].view(np.uint64))
            assert np.array_equal(got["sums"][0], want["sums"]) and got["records"][0, 4] == -1


def test_init_without_rounds_comes_back_as_params():
    flow, truth, Ps = L.three_motions(61, 23, seed=5)
    init = np.array([Ps[2], Ps[0], Ps[1], (np.nan, 0, 0, 0, 0, np.inf)])
    out = L.layers(flow, layers=4, rounds=0, init=init)
    assert np.array_equal(out["params"].view(np.uint64), init.view(np.uint64))
    assert out["records"][:, 2:5].tolist() == [[1, 1, -2]] * 4 and not out["sums"].any() and out["stats"][3] == 4
    # layers are not reordered: the true regions carry the index their motion was given, the non-finite layer holds nothing
    for t, k in ((0, 1), (1, 2), (2, 0)):
        assert (out["labels"][truth == t] == k).mean() >= 0.99
    assert out["records"][3, 0] == 0


def test_the_higher_of_two_identical_layers_gets_no_pixels():
    flow, truth, Ps = L.three_motions(61, 23, seed=6)
    init = np.array([Ps[0], Ps[0], Ps[1]])
    out = L.layers(flow, layers=3, rounds=0, init=init)
    assert out["records"][0, 0] > 0 and out["records"][1, 0] == 0 and not (out["labels"] == 1).any()
    # one refinement round: the twin joins no pixel, so its system is unusable -- it keeps its parameters, is not fitted, stays live
    # (layer 0 has moved on by the final pass, so the twin may then be the nearer one somewhere)
    out = L.layers(flow, layers=3, rounds=1, init=init)
    assert out["records"][1, 1:4].tolist() == [0, 1, 0] and not out["sums"][1].any()
    assert np.array_equal(out["params"][1], init[1]) and not np.array_equal(out["params"][0], init[0])


def test_masked_and_unknown_pixels():
    w, h = 64, 40
    flow, mask, _ = M.make_scene(w, h, seed=11, specials=True)
    out = L.layers(flow, mask, layers=2)
    kn = M.known(flow)
    assert (~kn).sum() >= 5 and (mask[~kn] != 0).any()                # the scene masks an unknown pixel: unknown wins
    assert (out["labels"][~kn] == L.UNKNOWN).all() and (out["labels"][kn & (mask != 0)] == L.MASKED).all()
    assert (out["labels"][kn & (mask == 0)] <= L.UNASSIGNED).all()
    assert out["stats"][:3].tolist() == [int((out["labels"] == c).sum()) for c in (253, 254, 255)]
    # every pixel masked: nothing is fitted, every layer is dead, the residual is the flow itself
    out = L.layers(flow, np.ones((h, w), np.uint8), layers=3)
    assert not out["records"][:, :4].any() and out["stats"].tolist() == [0, int(kn.sum()), int((~kn).sum()), 0]
    assert not out["params"].any() and np.array_equal(out["residual"].view(np.uint32), flow.view(np.uint32))
