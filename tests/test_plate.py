"""The background plate's definition, without a GPU: the numpy restatement tests/plate_ref.py on the jittered-crops scene with its
known integer motions (the median plate is exact where the definition says it must be, the mean is not), the path algebra and the
canvas of flowonthego_amd.plate against their numpy twins, the restatement against warp_ref for one sample, and the two inequalities
of the end-to-end GPU test on the oracle's flows."""
import numpy as np
import pytest

import motion_ref as M
import plate_ref as R
import warp_ref as WR

f32 = np.float32


@pytest.fixture(scope="module")
def scene(natural_images):
    frames, motions, canvas, truth, foot = R.crops_scene(natural_images["road_HD"], T=8)
    K = len(frames)
    W, H, ox, oy = canvas
    index = np.arange(K)[None]
    out = {}
    for name, kw in (("excl", dict(exclude=foot)), ("plain", {}), ("mean", dict(mode=1))):
        out[name] = R.plate(frames, index, W, H, ox, oy, params=motions[None], **kw)
    return dict(frames=frames, motions=motions, canvas=canvas, truth=truth, foot=foot, out=out,
                hit=R.stamp(foot, motions, canvas), cover=R.stamp(np.ones_like(foot), motions, canvas))


def test_scene_is_the_documented_one(scene):
    assert scene["frames"].shape == (9, 192, 320) and scene["canvas"] == (338, 204, 0, 0)
    assert np.array_equal(scene["cover"], scene["out"]["plain"][4][0])
    # where no patch is in the way a frame shows the underlying image
    dst = R.plate(scene["frames"][:1], [[0]], 338, 204, params=scene["motions"][None, :1])[0][0]
    clear = (scene["cover"] > 0) & (R.stamp(scene["foot"][:1], scene["motions"][:1], scene["canvas"]) == 0)
    clear &= R.stamp(np.ones_like(scene["foot"][:1]), scene["motions"][:1], scene["canvas"]) > 0
    assert np.array_equal(dst[clear], scene["truth"][clear])


def test_median_with_exclude_is_exact_at_every_estimated_pixel(scene):
    dst, count, code, stats, cover = scene["out"]["excl"]
    ok = code[0] == 0
    assert np.array_equal(dst[0][ok], scene["truth"][ok])
    n = np.bincount(code[0].ravel(), minlength=3)
    print("codes 0, 1, 2:", n)
    assert n.tolist() == [67557, 1215, 180]
    assert np.array_equal(stats[0, :4], [67557, 1215, 180, count[0].sum()])
    # a sample leaves when any of its four taps is excluded: the footprint grows by the tap to the right and below
    assert (count[0] <= scene["cover"] - scene["hit"]).all() and (count[0] == scene["cover"] - scene["hit"]).mean() > 0.95
    # hidden = covered, but by no frame that may be used; uncovered = no frame at all
    assert ((scene["cover"] > 0) & (scene["cover"] == scene["hit"]) <= (code[0] == 1)).all()
    assert np.array_equal(code[0] == 2, scene["cover"] == 0)
    assert not dst[0][~ok].any()                                                # fill


def test_median_without_exclude_is_exact_where_the_patch_is_in_the_minority(scene):
    dst, count, code, _, cover = scene["out"]["plain"]
    minority = (2 * scene["hit"] < scene["cover"])
    share = minority.sum() / minority.size
    print("patch in the minority at %.1f %% of the canvas" % (100 * share))
    assert 0.90 < share < 0.93
    assert np.array_equal(dst[0][minority], scene["truth"][minority])
    assert (dst[0][(code[0] == 0) & ~minority] != scene["truth"][(code[0] == 0) & ~minority]).any()
    assert np.array_equal(count[0], scene["cover"])


def test_mean_is_not_exact_there(scene):
    dst = scene["out"]["mean"][0][0]
    minority = (2 * scene["hit"] < scene["cover"])
    exact = (dst == scene["truth"])[scene["cover"] > 0].mean()
    print("the mean is exact at %.1f %% of the covered pixels" % (100 * exact))
    assert (dst[minority] != scene["truth"][minority]).any() and exact < 0.85
    # where no frame shows the patch the mean of equal bytes is the byte
    same = (scene["hit"] == 0) & (scene["cover"] > 0)
    assert np.array_equal(dst[same], scene["truth"][same])


def test_min_count_moves_pixels_to_the_other_codes(scene):
    f, mo, (W, H, ox, oy) = scene["frames"], scene["motions"], scene["canvas"]
    dst, count, code, stats, cover = R.plate(f, np.arange(9)[None], W, H, ox, oy, params=mo[None], exclude=scene["foot"], min_count=9, fill=7)
    assert np.array_equal(code[0] == 0, count[0] == 9) and np.array_equal(code[0] == 2, cover[0] < 9)
    assert (code[0] == 1).any() and (code[0] == 2).any() and (code[0] == 0).any()
    assert (dst[0][code[0] != 0] == 7).all()


def test_motions_and_canvas_agree_with_their_twins_and_the_known_offsets(natural_images):
    import torch
    from flowonthego_amd.plate import mosaic_canvas, plate_motions
    frames, off = M.jittered_crops(natural_images["road_HD"], T=8, patch=True)
    steps = np.zeros((8, 6))
    steps[:, 2] = off[:-1, 0] - off[1:, 0]
    steps[:, 5] = off[:-1, 1] - off[1:, 1]
    for ref in (0, 3, 8):
        got = plate_motions(torch.from_numpy(steps), ref).numpy()
        assert np.array_equal(got, R.plate_motions(steps, ref))
        assert np.array_equal(got[:, 2], off[ref, 0] - off[:, 0]) and np.array_equal(got[:, 5], off[ref, 1] - off[:, 1])
        assert not got[:, [0, 1, 3, 4]].any() and not got[ref].any()
        assert mosaic_canvas(torch.from_numpy(got), 320, 192) == R.mosaic_canvas(got, 320, 192)
    assert mosaic_canvas(plate_motions(torch.from_numpy(steps), 0), 320, 192) == (338, 204, 0, 0)
    W, H, ox, oy = mosaic_canvas(plate_motions(torch.from_numpy(steps), 3), 320, 192)
    assert (W, H) == (338, 204) and (ox, oy) == (int(off[3, 0] - off[:, 0].min()), int(off[3, 1] - off[:, 1].min()))
    # a general affine path: composing and inverting in the written order, bit for bit
    rng = np.random.default_rng(3)
    P = rng.normal(0, 0.01, (5, 6))
    P[:, [2, 5]] = rng.normal(0, 4, (5, 2))
    for ref in (0, 2, 5):
        got = plate_motions(torch.from_numpy(P), ref)
        assert np.array_equal(got.numpy(), R.plate_motions(P, ref))
        assert mosaic_canvas(got, 61, 23) == R.mosaic_canvas(got.numpy(), 61, 23)
    W, H, ox, oy = R.mosaic_canvas(R.plate_motions(P, 2), 61, 23)
    assert W >= 61 and H >= 23 and 0 <= ox < W and 0 <= oy < H                            # the reference frame's corner is on it
    from flowonthego_amd import FotgError
    with pytest.raises(FotgError):
        mosaic_canvas([[0, 0, 20000.0, 0, 0, 0], [0, 0, 0, 0, 0, 0]], 320, 192)              # wider than the largest canvas
    with pytest.raises(FotgError):
        mosaic_canvas([[-1.0, 0, 0, 0, 0, 0]], 8, 8)                                          # cannot be inverted
    with pytest.raises(FotgError):
        plate_motions(torch.from_numpy(steps), 9)
    with pytest.raises(FotgError):
        plate_motions(torch.from_numpy(steps.astype(f32)), 0)


def test_one_sample_is_the_warp_at_its_valid_pixels():
    rng = np.random.default_rng(5)
    h, w = 23, 31
    for noc, dtype in ((1, np.uint8), (3, f32)):
        frame = rng.integers(0, 256, (h, w) if noc == 1 else (h, w, noc)).astype(dtype)
        flow = WR.case_flow("smooth", h, w, 1)
        flow[3, 4] = (np.nan, 0)
        wd, wc, _ = WR.warp(frame, flow)
        dst, count, code, stats, _ = R.plate(frame[None], [[0]], w, h, flows=flow[None, None])
        assert np.array_equal(code[0] == 0, wc == 0) and (wc == 2).any() and (wc == 3).sum() == 1
        assert np.array_equal(dst[0][wc == 0], wd[wc == 0]) and np.array_equal(count[0], (wc == 0).astype(np.uint8))


def test_median_order_and_ties():
    """two to five samples of one pixel: the even rule, the stable order, NaN pixels and non-finite vectors leave"""
    frames = np.array([3, 1, np.nan, 2, 1, np.inf], f32).reshape(6, 1, 1)
    z = np.zeros((1, 6, 1, 1, 2), f32)
    dst, count, _, _, _ = R.plate(frames, [[0, 1, 2, 3, 4, -1]], 1, 1, flows=z[:, :6])
    assert count[0, 0, 0] == 4 and dst[0, 0, 0] == f32(1.5)                                  # 1 1 2 3
    dst, count, _, _, _ = R.plate(frames, [[0, 1, 3, 5, -1, -1]], 1, 1, flows=z)
    assert count[0, 0, 0] == 3 and dst[0, 0, 0] == f32(2.0)                                  # 1 2 3: inf x 0 in the taps is NaN
    dst, count, _, _, _ = R.plate(frames, [[5, 1, 3, 5, 0, -1]], 1, 1, flows=z, mode=1)
    assert count[0, 0, 0] == 3 and dst[0, 0, 0] == f32(2.0)                                  # (1 + 2 + 3) / 3
    z[0, 1, 0, 0] = (np.inf, 0)
    z[0, 2, 0, 0] = (0.25, 0)                                                                 # leaves the 1 x 1 frame
    dst, count, code, _, cover = R.plate(frames, [[0, 1, 3, 4, -1, -1]], 1, 1, flows=z)
    assert count[0, 0, 0] == 2 and cover[0, 0, 0] == 2 and dst[0, 0, 0] == f32(2.0)
    dst, count, code, _, cover = R.plate(frames, [[0, 1, 3, 4, -1, -1]], 1, 1, flows=z, min_count=3, fill=9)
    assert code[0, 0, 0] == 2 and dst[0, 0, 0] == 9
    assert R.plate(frames, [[2, 0, -1]], 1, 1, flows=0 * z[:, 3:], min_count=2)[2][0, 0, 0] == 1     # covered twice, one sample NaN


def test_statistics_are_added_in_the_kernels_order():
    rng = np.random.default_rng(9)
    part = rng.uniform(0, 1, 1000)
    assert abs(R.fold(part) - part.sum()) < 1e-9 and R.fold(part[:1]) == part[0] and R.fold(part[:0]) == 0.0
    terms = rng.uniform(0, 1, (5, 130, 3))
    assert abs(R._sum_in_kernel_order(terms) - terms.sum()) < 1e-9


# ---- the end-to-end inequalities on the oracle's flows --------------------------------------------------------------------------
def test_median_plate_beats_the_mean_and_the_unaligned_median_on_the_oracles_flows(natural_images):
    """what tests/test_gpu_plate.py asserts of OFClass.background on the GPU, here through the oracle's flows (the recipe of
    tests/test_motion.py::oracle_flows), motion_ref.fit and plate_ref: the default mode is bit-identical to the oracle"""
    from oracle import oracle as O
    image = natural_images["road_HD"]
    frames, motions, (_, _, ox, oy), truth, foot = R.crops_scene(image, T=8, w=R.BIG_W, h=R.BIG_H)
    K, h, w = frames.shape
    assert np.array_equal(frames[:, :M.CROP_H, :M.CROP_W], M.jittered_crops(image, T=8, patch=True)[0])   # the same scene, larger crops
    fr = frames.astype(f32)
    fits = [M.fit(O.full_flow(fr[k], fr[k + 1], op=2), None, 2, 3) for k in range(K - 1)]
    params = np.stack([f["params"] for f in fits])
    exclude = np.zeros((K, h, w), np.uint8)
    exclude[:K - 1] = np.stack([f["code"] == 1 for f in fits])
    est = R.plate_motions(params, 0)
    grid = (w, h, 0, 0)
    index = np.arange(K)[None]
    med = R.plate(frames, index, w, h, params=est[None], exclude=exclude)
    mean = R.plate(frames, index, w, h, params=est[None], exclude=exclude, mode=1)
    ident = R.plate(frames, index, w, h, params=np.zeros((1, K, 6)))
    hit, cover = R.stamp(foot, motions, grid), R.stamp(np.ones_like(foot), motions, grid)
    sel = (med[2][0] == 0) & (mean[2][0] == 0) & (ident[2][0] == 0) & (2 * hit < cover)
    T0 = truth[oy:oy + h, ox:ox + w].astype(np.float64)                        # the underlying image on the reference frame's grid
    e = [float(np.abs(d[0][0].astype(np.float64) - T0)[sel].mean()) for d in (med, mean, ident)]
    mse = float(((med[0][0].astype(np.float64) - T0)[sel] ** 2).mean())
    print("mean absolute error over %d pixels: median %.4f, mean %.4f, median with identity motions %.4f; PSNR of the median plate %.2f dB"
          % (sel.sum(), e[0], e[1], e[2], 10 * np.log10(255.0 ** 2 / mse)))
    assert sel.sum() > 0.8 * h * w
    assert e[0] < e[1] and e[0] < e[2]
