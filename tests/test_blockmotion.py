"""The numpy restatement of the block motion vectors (tests/blockmotion_ref.py) does what the definition says: no GPU needed.  The
GPU is compared with it byte for byte in tests/test_gpu_blockmotion.py."""
import numpy as np
import pytest

import blockmotion_ref as R


def shifted(h, w, dx, dy, seed, noc=1):
    """random 8-bit noise `ref` and `cur` with cur(x, y) = ref(x + dx, y + dy) where that lies inside the frame (noise elsewhere)"""
    rng = np.random.default_rng(seed)
    shape = (h, w) + ((noc,) if noc > 1 else ())
    ref = rng.integers(0, 256, shape, dtype=np.uint8)
    cur = rng.integers(0, 256, shape, dtype=np.uint8)
    ys, xs = np.mgrid[0:h, 0:w]
    ok = (xs + dx >= 0) & (xs + dx < w) & (ys + dy >= 0) & (ys + dy < h)
    cur[ok] = ref[(ys + dy)[ok], (xs + dx)[ok]]
    return cur, ref


@pytest.mark.parametrize("block", [8, 16, 32])
@pytest.mark.parametrize("noc", [1, 3])
def test_exact_shift_is_found_with_sad_zero(block, noc):
    h, w, dx, dy = 70, 100, 3, -2
    cur, ref = shifted(h, w, dx, dy, 1, noc)
    flow = np.empty((h, w, 2), np.float32)
    flow[:] = (dx, dy)
    for refine in (0, 2):
        mv, cost, kind, pred, st = R.block_motion_one(cur, ref, flow, None, block, refine)
        inside = 0
        for by in range(mv.shape[0]):
            for bx in range(mv.shape[1]):
                x0, x1, y0, y1 = bx * block, min(bx * block + block, w), by * block, min(by * block + block, h)
                if x0 + dx >= 0 and x1 + dx <= w and y0 + dy >= 0 and y1 + dy <= h:       # the shifted footprint is inside the frame
                    inside += 1
                    assert tuple(mv[by, bx]) == (4 * dx, 4 * dy) and cost[by, bx, 0] == 0 and kind[by, bx] == 1, (bx, by)
                    assert np.array_equal(pred[y0:y1, x0:x1], cur[y0:y1, x0:x1])
        assert inside >= 2


def test_invariants_and_stats_are_the_sums_of_the_block_outputs():
    for noc, block, refine, seed in ((1, 8, 3, 1), (3, 16, 1, 2), (1, 32, 2, 3)):
        cur, ref, flow, mask = R.scene(40, 130, noc, seed, n=2)
        mv, cost, kind, pred, st = R.block_motion(cur, ref, flow, mask, block, refine)
        assert mv.dtype == np.int16 and cost.dtype == np.uint32 and kind.dtype == np.uint8 and pred.dtype == np.uint8
        assert st.dtype == np.int64 and st.shape == (2, 11) and pred.shape == cur.shape
        assert (cost[..., 0] <= cost[..., 1]).all()
        assert (np.abs(mv.astype(int)) <= R.QMAX).all() and ((kind & 7) <= 6).all() and (kind < 16).all()
        for i in range(2):
            sse = ((cur[i].astype(np.int64) - pred[i]) ** 2).sum()
            want = [cost[i, ..., 0].sum(), cost[i, ..., 1].sum(), sse, ((kind[i] & 8) != 0).sum()]
            want += [((kind[i] & 7) == k).sum() for k in range(7)]
            assert st[i].tolist() == [int(v) for v in want]
            # the prediction is the one the vectors give, and its SAD is the cost
            for by in range(mv.shape[1]):
                for bx in range(mv.shape[2]):
                    x0, x1, y0, y1 = bx * block, min(bx * block + block, 130), by * block, min(by * block + block, 40)
                    p = R.predict(ref[i].reshape(40, 130, -1).astype(np.int64), x0, x1, y0, y1, int(mv[i, by, bx, 0]), int(mv[i, by, bx, 1]))
                    assert np.array_equal(p, pred[i].reshape(40, 130, -1)[y0:y1, x0:x1])
                    assert np.abs(cur[i].reshape(40, 130, -1)[y0:y1, x0:x1] - p).sum() == cost[i, by, bx, 0]
        # without refinement nothing moves
        assert (R.block_motion(cur, ref, flow, mask, block, 0)[2] < 8).all()


def test_a_block_without_admissible_pixels_has_only_the_zero_vector():
    cur, ref, flow, _ = R.scene(40, 70, 1, 4, n=1)
    cur, ref, flow = cur[0], ref[0], flow[0]
    mask = np.zeros((40, 70), np.uint8)
    mask[0:16, 16:32] = 2                                          # block (1, 0) of the 16-grid: masked out
    flow[16:32, 0:16] = np.nan                                     # block (0, 1): not known
    flow[16:32, 16:32, 0] = 4096.5                                 # block (1, 1): beyond the bound
    mask[16:32, 32:48] = 200                                       # block (2, 1): a byte above 3
    for refine in (0, 3):
        mv, cost, kind, pred, st = R.block_motion_one(cur, ref, flow, mask, 16, refine)
        for by, bx in ((0, 1), (1, 0), (1, 1), (1, 2)):
            assert kind[by, bx] in (0, 8)
            if refine == 0:
                assert tuple(mv[by, bx]) == (0, 0) and cost[by, bx, 0] == cost[by, bx, 1]
        assert (kind[0, 0] & 7) != 0                               # its neighbour has candidates, and one of them wins
    # one admissible pixel is enough for the mean, and for its quadrant
    mask[5, 20] = 0
    flow[5, 20] = (1.26, -0.74)                                    # Q = (5, -3)
    cands = R.block_motion_one(cur, ref, flow, mask, 16, 0)
    assert R.mean_vector(*[a[0:16, 16:32] for a in R.quantise(flow, mask)]) == (5, -3)
    assert tuple(cands[0][0, 1]) in ((0, 0), (5, -3))


def test_the_mean_is_a_floor_division_and_the_rounding_is_to_nearest_even():
    Q = np.array([[[-1, 1], [-2, 2], [0, 0]]], np.int64)          # S = (-3, 3), m = 3: floor((-6 + 3) / 6) = -1, floor(9 / 6) = 1
    assert R.mean_vector(Q, np.ones((1, 3), bool)) == (-1, 1)
    Q = np.array([[[-1, 1], [0, 0]]], np.int64)                    # S = (-1, 1), m = 2: floor((-2 + 2) / 4) = 0, floor(4 / 4) = 1
    assert R.mean_vector(Q, np.ones((1, 2), bool)) == (0, 1)
    assert R.mean_vector(Q, np.zeros((1, 2), bool)) is None
    f = np.array([[[0.125, -0.125], [0.375, -0.375], [4096.0, -4096.0], [np.nan, 0.0], [0.0, np.inf], [4096.5, 0.0]]], np.float32)
    q, adm = R.quantise(f)
    assert q[0, :3].tolist() == [[0, 0], [2, -2], [16384, -16384]] and adm[0].tolist() == [True, True, True, False, False, False]
    assert R.quantise(f, np.array([[0, 1, 200, 0, 0, 0]], np.uint8))[1][0].tolist() == [True, False, False, False, False, False]


def test_vectors_at_the_bound_stay_inside_it():
    ref = np.random.default_rng(5).integers(0, 256, (19, 67), dtype=np.uint8)
    for sign in (1, -1):
        flow = np.empty((19, 67, 2), np.float32)
        flow[:] = (-4096.0 * sign, 4096.0 * sign)
        # every tap clamps to one corner pixel of ref: a cur of that value is predicted exactly by the vector at the bound and by
        # its inward neighbours alike (none strictly better), the outward ones are skipped
        corner = ref[18 if sign > 0 else 0, 0 if sign > 0 else 66]
        cur = np.full((19, 67), corner, np.uint8)
        mv, cost, kind, pred, st = R.block_motion_one(cur, ref, flow, None, 16, 3)
        assert (mv == (-16384 * sign, 16384 * sign)).all() and (kind == 1).all() and (cost[..., 0] == 0).all()
        assert (cost[..., 1] > 0).all() and (pred == corner).all()
        # noise instead: whatever wins, no component leaves the bound
        cur = np.random.default_rng(6).integers(0, 256, (19, 67), dtype=np.uint8)
        mv, cost, kind, pred, st = R.block_motion_one(cur, ref, flow, None, 16, 3)
        assert (np.abs(mv.astype(int)) <= R.QMAX).all()
        assert ((mv == (-16384 * sign, 16384 * sign)).all(-1) == ((kind & 7) != 0)).all()


def test_golden_pair_halves_the_zero_vector_sad(alley, alley_golden_flow):
    cur, ref = alley["frame_0001"], alley["frame_0002"]
    mv, cost, kind, pred, st = R.block_motion_one(cur, ref, alley_golden_flow, None, 16, 0)
    print("alley_1, block 16, refine 0: SAD %d, zero-vector SAD %d, PSNR %.2f dB, winners %s"
          % (st[0], st[1], R.psnr(st[2], cur.size), st[4:].tolist()))
    assert 2 * st[0] < st[1]
    assert st[:2].tolist() == [1001155, 3095382] and st[4:].tolist() == [72, 1062, 46, 237, 138, 150, 87]    # the issue's prototype
    assert abs(R.psnr(st[2], cur.size) - 34.43) < 0.005
