"""The object removal's definition, without a GPU: the numpy restatement tests/erase_ref.py against first principles -- the weight
table against a big-integer evaluation, its disc, its reach and its monotony; on the jittered-crops scene with its known integer
translations the patch is replaced by exactly the clean image; and the refusals of the Python forms, decided before anything is
launched."""
from fractions import Fraction

import numpy as np
import pytest

import erase_ref as R
import plate_ref as PR
from flowonthego_amd.erase import CODES, FULL, MAX_FEATHER, MAX_GROW, STATS

f32 = np.float32
assert (R.MAX_GROW, R.MAX_FEATHER) == (MAX_GROW, MAX_FEATHER) and len(CODES) == 5 and len(STATS) == 8 and FULL == 256
ALL_GF = [(G, F) for G in range(MAX_GROW + 1) for F in range(MAX_FEATHER + 1)]


# ---- the weight ------------------------------------------------------------------------------------------------------------------
def test_alpha_table_equals_a_big_integer_evaluation():
    """floor(sqrt(256 D2)) found by comparing squares of Python integers, the quotient as an exact fraction rounded down"""
    for G, F in ALL_GF:
        tab = R.alpha_table(G, F)
        assert len(tab) == 2 * (G + F) ** 2 + 1
        for D2, got in enumerate(tab.tolist()):
            if D2 <= G * G:
                want = 256
            elif F == 0:
                want = 0
            else:
                D16 = 0
                while (D16 + 1) ** 2 <= 256 * D2:
                    D16 += 1
                E = 16 * (G + F) - D16
                want = 0 if E <= 0 else min(256, int(Fraction(256 * E + 8 * F, 16 * F)))     # int() of a positive fraction: rounded down
            assert got == want, (G, F, D2)


def test_alpha_is_full_on_the_disc_zero_beyond_the_feather_and_monotone():
    for G, F in ALL_GF:
        tab = R.alpha_table(G, F)
        D2 = np.arange(len(tab))
        # 256 exactly on the disc of radius G.  The ramp has 16 steps per pixel, so a distance less than 1/16 pixel beyond G still
        # rounds to 256: among integer D2 that is D2 = G^2 + 1 <= G^2 + G / 8, the one case G = 8, D2 = 65 (sqrt(65) = 8.062)
        beyond = (tab == 256) & (D2 > G * G)
        assert (tab[D2 <= G * G] == 256).all() and beyond.sum() == (1 if G == 8 and F > 0 else 0) and (not beyond.any() or beyond[65])
        if F == 0:
            assert not tab[D2 > G * G].any()                              # without a feather the disc is all there is
        assert not tab[D2 >= (G + F) ** 2].any() or F == 0                # with a feather: nothing from distance G + F on
        assert not tab[D2 > (G + F) ** 2].any()                           # nothing beyond G + F
        assert (np.diff(tab) <= 0).all()                                  # monotone in D2
        assert tab.min() >= 0 and tab.max() <= 256
    # the ramp: 16 steps per pixel, 256 at distance G, half way at G + F / 2
    tab = R.alpha_table(2, 4)
    assert tab[4] == 256 and tab[16] == 128 and tab[36] == 0 and tab[25] == 64
    # a single pixel: the weights are those of its distances
    rm = np.zeros((21, 23), np.uint8)
    rm[10, 11] = 1
    al = R.weights(rm, 2, 3)
    yy, xx = np.mgrid[:21, :23]
    d2 = (yy - 10) ** 2 + (xx - 11) ** 2
    assert np.array_equal(al == 256, d2 <= 4) and np.array_equal(al > 0, d2 < 25)
    assert np.array_equal(R.disc_dilation(rm, 2), (d2 <= 4).astype(np.uint8))
    # pixels outside the frame hold nothing; a set pixel on the border reaches inwards only
    rm = np.zeros((5, 7), np.uint8)
    rm[0, 0] = rm[4, 6] = 9
    al = R.weights(rm, 1, 0)
    assert al.sum() == 256 * 6 and al[0, 1] == 256 and al[1, 0] == 256 and al[3, 6] == 256 and al[1, 1] == 0


def test_distance_is_capped_by_the_window():
    rm = np.zeros((9, 40), np.uint8)
    rm[4, 3] = 1
    d2 = R.distance2(rm, 5)
    assert d2[4, 8] == 25 and d2[4, 9] == R.FAR and d2[0, 3] == 16 and d2[4, 3] == 0
    assert d2[0, 8] == 41                                                 # inside the window although beyond the disc of R


# ---- the scene with known translations ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene(natural_images):
    frames, motions, canvas, truth, foot = PR.crops_scene(natural_images["road_HD"], T=8)
    back = np.zeros_like(motions)
    back[:, 2], back[:, 5] = -motions[:, 2], -motions[:, 5]                # frame -> reference
    return dict(frames=frames, back=back, canvas=canvas, truth=truth, foot=foot)


def _clean_crops(scene):
    """the underlying image under every frame, and where the frame's pixel lies inside the canvas"""
    frames, back = scene["frames"], scene["back"]
    W, H, ox, oy = scene["canvas"]
    K, h, w = frames.shape
    crops = np.zeros_like(frames)
    inside = np.zeros((K, h, w), bool)
    for k in range(K):
        X0, Y0 = ox + int(back[k, 2]), oy + int(back[k, 5])
        xs, ys = np.arange(w) + X0, np.arange(h) + Y0
        ok = ((ys >= 0) & (ys < H))[:, None] & ((xs >= 0) & (xs < W))[None, :]
        crops[k] = scene["truth"][np.clip(ys, 0, H - 1)[:, None], np.clip(xs, 0, W - 1)[None, :]]
        inside[k] = ok
    return crops, inside


def test_the_patch_is_replaced_by_exactly_the_clean_image(scene):
    frames, foot = scene["frames"], scene["foot"]
    W, H, ox, oy = scene["canvas"]
    crops, inside = _clean_crops(scene)
    dst, code, alpha, stats = R.erase(frames, scene["truth"][None], foot, None, ox, oy, params=scene["back"], grow=0, feather=0)
    on = (foot != 0) & inside
    assert on.sum() > 0.9 * (foot != 0).sum() and (foot != 0).any()
    assert np.array_equal(dst[on], crops[on])                             # the clean crop, exactly
    assert np.array_equal(dst[~on], frames[~on])                          # the frame, bit for bit, elsewhere
    assert np.array_equal(alpha, 256 * (foot != 0)) and np.array_equal(code[on], np.ones(on.sum(), np.uint8))
    assert np.array_equal(stats[:, 5], ((foot != 0) & ~inside).sum((1, 2)))
    assert not stats[inside.all((1, 2)), 5].any()                         # no holes where the canvas holds the whole frame
    assert np.array_equal(stats[:, 6], (foot != 0).sum((1, 2))) and np.array_equal(stats[:, 7], alpha.astype(np.int64).sum((1, 2)))
    assert np.array_equal(stats[:, :5], np.stack([np.bincount(c.ravel(), minlength=5) for c in code]))
    # the frame differs from the clean crop under the patch, and no longer after the removal
    assert (frames[on] != crops[on]).mean() > 0.5


def test_grown_and_feathered_every_pixel_of_weight_zero_is_the_frames(scene):
    frames, foot = scene["frames"], scene["foot"]
    W, H, ox, oy = scene["canvas"]
    crops, inside = _clean_crops(scene)
    dst, code, alpha, stats = R.erase(frames, scene["truth"][None], foot, None, ox, oy, params=scene["back"], grow=2, feather=3)
    assert np.array_equal(dst[alpha == 0], frames[alpha == 0]) and not code[alpha == 0].any()
    assert np.array_equal(alpha == 256, R.disc_dilation(foot, 2) == 1)
    full = (alpha == 256) & inside
    assert np.array_equal(dst[full], crops[full]) and (code[full] == 1).all()
    ramp = (alpha > 0) & (alpha < 256) & inside
    assert ramp.any() and (code[ramp] == 4).all()
    # outside the patch the frame is the clean crop, so a blend of the two changes nothing there
    calm = ramp & (frames == crops)
    assert calm.any() and np.array_equal(dst[calm], frames[calm])
    lo, hi = np.minimum(frames, crops), np.maximum(frames, crops)
    assert (dst[ramp] >= lo[ramp]).all() and (dst[ramp] <= hi[ramp]).all()


def test_codes_and_the_order_of_the_tests_by_hand():
    frame = np.full((1, 3, 6), 10.0, f32)
    frame[0, 0, 0] = np.nan
    plate = np.full((1, 3, 6), 50.0, f32)
    plate[0, 0, 5] = np.nan
    z = np.zeros((1, 3, 6, 2), f32)
    z[0, 0, 1] = (np.nan, 0)
    z[0, 0, 2] = (-3.0, 0)
    z[0, 1, 1] = (0.5, 0)
    rm = np.zeros((1, 3, 6), np.uint8)
    rm[0, 0] = 1
    rm[0, 1, 1] = 1
    mask = np.zeros((1, 3, 6), np.uint8)
    mask[0, 0, 5] = 7
    pcode = np.zeros((1, 3, 6), np.uint8)
    pcode[0, 1, 2] = 1
    dst, code, alpha, stats = R.erase(frame, plate, rm, flows=z, mask=mask, plate_code=pcode, grow=0, feather=0)
    # (0, 0): a NaN frame pixel does not disqualify: replaced; (0, 1): NaN vector; (0, 2): outside; (0, 3): good; (0, 4): a NaN
    # sample, through its right tap of weight 0; (0, 5): masked; (1, 1): a tap (1, 2) with plate_code, although the other would do
    assert code[0, 0].tolist() == [1, 3, 2, 1, 3, 3] and code[0, 1].tolist() == [0, 2, 0, 0, 0, 0]
    assert dst[0, 0, 0] == 50.0 and dst[0, 0, 3] == 50.0 and dst[0, 0, 1] == 10.0 and dst[0, 1, 1] == 10.0
    assert stats[0].tolist() == [11, 2, 2, 3, 0, 5, 7, 7 * 256]
    # a blend: 10 + (50 - 10) * alpha / 256
    one = np.zeros((1, 3, 6), np.uint8)
    one[0, 2, 3] = 1
    dst, code, alpha, _ = R.erase(frame, plate, one, flows=np.zeros_like(z), grow=0, feather=2)
    assert alpha[0, 2].tolist() == [0, 0, 128, 256, 128, 0] and alpha[0, 1, 3] == 128 and alpha[0, 1, 2] == 80
    assert dst[0, 2, 2] == 30.0 and code[0, 2, 2] == 4 and dst[0, 2, 3] == 50.0 and dst[0, 1, 2] == 22.5 and code[0, 2, 3] == 1
    # 8-bit: rounded once, at the store, halves to even
    d8 = R.erase(np.full((1, 3, 6), 10, np.uint8), np.full((1, 3, 6), 51, np.uint8), one, flows=np.zeros_like(z), grow=0, feather=2)[0]
    assert d8.dtype == np.uint8 and d8[0, 2, 2] == 30 and d8[0, 2, 3] == 51 and d8[0, 1, 2] == 23 and d8[0, 0, 0] == 10


# ---- the refusals of the Python forms ----------------------------------------------------------------------------------------------
class _Ctx:
    """what the fused form reads of a context before it touches the device"""
    nch, max_batch, height_org, width_org, device, _h = 2, 2, 8, 12, None, None

    def out_size(self):
        return 6, 4


def test_python_refusals_launch_nothing():
    import torch
    from flowonthego_amd import FotgError
    from flowonthego_amd.erase import grow_mask, remove_objects, upsample_crop_remove_objects
    fr, pl, rm = torch.zeros((2, 8, 12)), torch.zeros((8, 12)), torch.zeros((2, 8, 12), dtype=torch.uint8)
    fl, mo = torch.zeros((2, 8, 12, 2)), torch.zeros((2, 6), dtype=torch.float64)
    plain = (dict(grow=-1), dict(grow=9), dict(feather=-1), dict(feather=9), dict(grow=1.5), dict(feather="a"), dict(grow=True),
             dict(origin=5), dict(origin=(1 << 21, 0)), dict(origin=(0, 1, 2)), dict(dst=False))
    for kw in plain:
        with pytest.raises(FotgError):
            remove_objects(fr, pl, rm, flows=fl, **kw)
        with pytest.raises(FotgError):
            remove_objects(fr, pl, rm, motions=mo, **kw)
        with pytest.raises(FotgError):
            upsample_crop_remove_objects(_Ctx(), torch.zeros((2, 4, 6, 2)), fr, pl, rm, **kw)
    for kw in (dict(), dict(flows=fl, motions=mo), dict(flows=[1, 2]), dict(motions=torch.zeros((2, 3, 6), dtype=torch.float64)),
               dict(flows=torch.zeros((8, 12))), dict(flows=fl), dict(motions=mo)):        # the last two: host tensors
        with pytest.raises(FotgError):
            remove_objects(fr, pl, rm, **kw)
    for ctx, cf in ((_Ctx(), torch.zeros((3, 4, 6, 2))), (_Ctx(), torch.zeros((4, 6, 2))), (_Ctx(), None), (_Ctx(), torch.zeros((2, 4, 6, 2)))):
        for fused in (True, False):
            with pytest.raises(FotgError):
                upsample_crop_remove_objects(ctx, cf, fr, pl, rm, fused=fused)
    for bad in ((rm, 9), (rm, -1), (rm, 1.0), (rm.float(), 1), (rm[0, 0], 1), (rm, 1)):      # the last: a host tensor
        with pytest.raises(FotgError):
            grow_mask(*bad)
