"""The background subtraction's definition, without a GPU: the numpy restatement tests/subtract_ref.py pinned by a formula that does
not share its code, on the jittered-crops scene with its known integer translations; frame_motions against its twin and as the
inverse of plate_motions; the hysteresis on a hand-made map; the refusals of the Python forms, decided before anything is launched;
and the two inequalities of the end-to-end GPU test on the oracle's flows."""
import numpy as np
import pytest

import motion_ref as M
import objects_ref as OR
import plate_ref as PR
import subtract_ref as R
from flowonthego_amd.subtract import CODES, MAX_Q, STATS

f32 = np.float32
assert R.MAX_Q == MAX_Q and len(CODES) == 5 and len(STATS) == 7                         # the restatement's alphabet is the binding's


# ---- the restatement against a formula of its own ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene(natural_images):
    frames, motions, canvas, truth, foot = PR.crops_scene(natural_images["road_HD"], T=8)
    W, H, ox, oy = canvas
    dst, _, pcode, _, _ = PR.plate(frames, np.arange(len(frames))[None], W, H, ox, oy, params=motions[None], exclude=foot)
    assert np.array_equal(dst[0][pcode[0] == 0], truth[pcode[0] == 0])                 # exact at every code-0 pixel
    back = np.zeros_like(motions)
    back[:, 2], back[:, 5] = -motions[:, 2], -motions[:, 5]                            # frame -> reference
    # step 3 of the definition looks at all four tap pixels, also where a tap has no weight: a plate pixel that is not code 0 hides
    # its left, upper and upper-left neighbours as well (the last row and column clamp onto themselves)
    hidden4 = pcode[0] != 0
    hidden4[:, :-1] |= hidden4[:, 1:].copy()
    hidden4[:-1, :] |= hidden4[1:, :].copy()
    return dict(frames=frames, motions=motions, back=back, canvas=canvas, truth=truth, foot=foot, plate=dst, pcode=pcode, hidden4=hidden4)


@pytest.mark.parametrize("r", [0, 1, 2])
def test_restatement_equals_the_plain_formula_on_known_translations(scene, r):
    frames, back, foot = scene["frames"], scene["back"], scene["foot"]
    W, H, ox, oy = scene["canvas"]
    K, h, w = frames.shape
    low, high = 8.0, 24.0
    code, diff, evidence, stats = R.subtract(frames, scene["plate"], None, ox, oy, params=back, plate_code=scene["pcode"], low=low,
                                             high=high, window=r)
    flows = np.zeros((K, h, w, 2), f32)
    flows[..., 0], flows[..., 1] = back[:, 2, None, None], back[:, 5, None, None]
    dense = R.subtract(frames, scene["plate"], [0] * K, ox, oy, flows=flows, plate_code=scene["pcode"], low=low, high=high, window=r)
    for a, b in zip((code, diff, evidence, stats), dense):
        assert np.array_equal(a, b)
    checked = 0
    for k in range(K):
        X0, Y0 = ox + int(back[k, 2]), oy + int(back[k, 5])                             # where the frame's pixel (0, 0) lies on the canvas
        crop = scene["truth"][Y0:Y0 + h, X0:X0 + w].astype(np.int64)
        known = ~scene["hidden4"][Y0:Y0 + h, X0:X0 + w]
        assert crop.shape == (h, w)                                                     # the canvas holds every frame
        dq = 16 * np.abs(frames[k].astype(np.int64) - crop)
        # plain box sums over the pixels of the frame
        S = np.zeros((h, w), np.int64)
        C = np.zeros((h, w), np.int64)
        bad = np.zeros((h, w), np.int64)
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                ya, yb, xa, xb = max(0, -dy), min(h, h - dy), max(0, -dx), min(w, w - dx)
                S[ya:yb, xa:xb] += dq[ya + dy:yb + dy, xa + dx:xb + dx]
                C[ya:yb, xa:xb] += 1
                bad[ya:yb, xa:xb] += ~known[ya + dy:yb + dy, xa + dx:xb + dx]
        want = np.where(S >= 16 * 24 * C, 4, np.where(S >= 16 * 8 * C, 1, 0))
        sel = bad == 0
        assert np.array_equal(diff[k][sel], dq[sel]) and np.array_equal(code[k][sel], want[sel])
        assert np.array_equal(code[k] == 2, ~known)
        # outside the footprint grown by r: background, no difference
        grown = R.box(foot[k].astype(np.int64), r) > 0
        calm = sel & ~grown
        assert not code[k][calm].any() and not diff[k][calm].any()
        inside = sel & (foot[k] == 1)
        assert (code[k][inside] == 4).mean() > 0.5
        assert np.array_equal(evidence[k][..., 0], (code[k] == 4).astype(f32)) and np.array_equal(evidence[k][..., 1] * 16, diff[k].astype(f32))
        assert np.array_equal(stats[k], list(np.bincount(code[k].ravel(), minlength=5)) + [diff[k].sum(), diff[k][(code[k] == 1) | (code[k] == 4)].sum()])
        checked += sel.sum()
    assert checked > 0.95 * K * h * w


def test_thresholds_window_and_saturation_by_hand():
    frame = np.zeros((1, 3, 5), f32)
    frame[0, 1, 2] = 9.0
    plate = np.zeros((1, 3, 5), f32)
    z = np.zeros((1, 3, 5, 2), f32)
    code, diff, _, stats = R.subtract(frame, plate, flows=z, low=1.0, high=1.0, window=1)
    assert diff[0, 1, 2] == 144 and diff.sum() == 144
    assert (code[0, :, 1:4] == 4).all() and not code[0, :, [0, 4]].any()                # 144 >= 16 C for C = 9 and for the 6 of an edge
    code = R.subtract(frame, plate, flows=z, low=1.0, high=1.0 + 1 / 16, window=1)[0]
    assert code[0, 1, 2] == 1 and (code[0, :, 1:4] >= 1).all() and (code[0, 0, 1:4] == 4).all()   # S = L C exactly in the middle; C = 6 at the edge
    code = R.subtract(frame, plate, flows=z, low=0.0, high=2047.9375, window=0)[0]
    assert (code == 1).all()                                                            # L = 0: S >= 0 everywhere
    frame[0, 0, 0] = 1e9
    code, diff, ev, _ = R.subtract(frame, plate, flows=z, low=0.0, high=2047.9375, window=0)
    assert diff[0, 0, 0] == 32767 and code[0, 0, 0] == 4 and ev[0, 0, 0, 1] == f32(32767 / 16)
    with pytest.raises(AssertionError):
        R.thresholds(8.0, 7.0)
    with pytest.raises(AssertionError):
        R.thresholds(0.0, 2048.0)
    # the order of the tests: an unknown vector before the plate's edge, the edge before a NaN pixel
    frame[0, 0, 0] = np.nan
    z[0, 0, 0] = (np.nan, 0)
    z[0, 0, 1] = (-2.0, 0)
    z[0, 0, 2] = (0.5, 0)
    plate[0, 0, 3] = np.nan
    mask = np.zeros((1, 3, 5), np.uint8)
    mask[0, 2, 4] = 7
    pcode = np.zeros((1, 3, 5), np.uint8)
    pcode[0, 2, 0] = 1
    code = R.subtract(frame, plate, flows=z, mask=mask, plate_code=pcode, window=0)[0]
    assert code[0, 0].tolist() == [3, 2, 3, 3, 0] and code[0, 2, 4] == 3 and code[0, 2, 0] == 2 and code[0, 2, 1] == 0


# ---- the motions -------------------------------------------------------------------------------------------------------------------
def test_frame_motions_inverts_plate_motions():
    import torch
    from flowonthego_amd import FotgError
    from flowonthego_amd.plate import plate_motions
    from flowonthego_amd.subtract import frame_motions
    rng = np.random.default_rng(11)
    for ref in (0, 3, 6):
        P = rng.normal(0, 0.02, (6, 6))
        P[:, [2, 5]] = rng.normal(0, 5, (6, 2))
        fwd = plate_motions(torch.from_numpy(P), ref)
        back = frame_motions(fwd)
        assert back.dtype == torch.float64 and back.shape == (7, 6)
        assert np.array_equal(back.numpy(), R.frame_motions(fwd.numpy()))               # the written order, bit for bit
        a, b = fwd.numpy(), back.numpy()
        A = (a[:, 0] + 1, a[:, 1], a[:, 2], a[:, 3], a[:, 4] + 1, a[:, 5])
        B = (b[:, 0] + 1, b[:, 1], b[:, 2], b[:, 3], b[:, 4] + 1, b[:, 5])
        for first, second in ((A, B), (B, A)):
            ident = np.stack(M._compose(first, second), axis=1)
            assert np.abs(ident - np.array([1, 0, 0, 0, 1, 0.0])).max() < 1e-9
    with pytest.raises(FotgError):
        frame_motions(torch.tensor([[-1.0, 0, 0, 0, 0, 0]], dtype=torch.float64))         # singular
    with pytest.raises(FotgError):
        frame_motions(torch.tensor([[0.0, 0, 0, 0, 0, float("nan")], [0, 0, 0, 0, float("inf"), 0]], dtype=torch.float64)[1:])
    with pytest.raises(FotgError):
        frame_motions(torch.zeros((2, 6)))
    with pytest.raises(FotgError):
        frame_motions(torch.zeros(6, dtype=torch.float64))


# ---- the hysteresis ----------------------------------------------------------------------------------------------------------------
def test_a_weak_blob_counts_only_with_a_strong_pixel():
    import torch
    from flowonthego_amd import FotgError
    from flowonthego_amd.subtract import FG, foreground_mask
    code = np.zeros((2, 12, 20), np.uint8)
    code[0, 2:6, 2:7] = 1
    code[0, 3, 4] = 4                                                                    # confirmed
    code[0, 7:11, 10:16] = 1                                                             # weak only
    code[0, 0, 18] = 2
    code[0, 1, 18] = 3
    code[1, 4:8, 4:8] = 4                                                                # strong throughout
    evidence = np.zeros((2, 12, 20, 2), f32)
    evidence[..., 0] = code == 4
    evidence[..., 1] = np.where((code == 1) | (code == 4), 10.5, 0)
    res = OR.components_batch(code, OR.fg_set(FG), 8, evidence, min_area=4, max_objects=5)
    objects, ids = res["objects"], res["ids"]
    assert objects[0, 0, 9] == 256 and objects[0, 1, 9] == 0 and objects[1, 0, 9] == 16 * 256      # sum_u / 256: the strong pixels
    assert objects[0, 0, 10] == 16 * 20 * 168                                            # sum_v = 16 sum of Dq
    confirmed = torch.from_numpy(objects[..., 9] > 0)
    assert confirmed.tolist() == [[True, False, False, False, False], [True, False, False, False, False]]
    mask = foreground_mask(torch.from_numpy(ids), confirmed)
    want = np.zeros((2, 12, 20), np.uint8)
    want[0, 2:6, 2:7] = 1
    want[1, 4:8, 4:8] = 1
    assert mask.dtype == torch.uint8 and np.array_equal(mask.numpy(), want)
    assert np.array_equal(foreground_mask(torch.from_numpy(ids[0]), confirmed[0]).numpy(), want[0])
    for bad in ((torch.from_numpy(ids), confirmed[0]), (torch.from_numpy(ids), confirmed.to(torch.uint8)), (ids, confirmed)):
        with pytest.raises(FotgError):
            foreground_mask(*bad)


# ---- the refusals of the Python forms ----------------------------------------------------------------------------------------------
class _Ctx:
    """what the fused form reads of a context before it touches the device"""
    nch, max_batch, height_org, width_org, device, _h = 2, 2, 8, 12, None, None

    def out_size(self):
        return 6, 4


def test_python_refusals_launch_nothing():
    import torch
    from flowonthego_amd import FotgError
    from flowonthego_amd.subtract import subtract_background, upsample_crop_subtract_background
    fr, pl = torch.zeros((2, 8, 12)), torch.zeros((8, 12))
    fl, mo = torch.zeros((2, 8, 12, 2)), torch.zeros((2, 6), dtype=torch.float64)
    plain = (dict(low=-1.0), dict(low=9.0, high=8.0), dict(high=2048.0), dict(low=float("nan")), dict(high=float("inf")), dict(low="a"),
             dict(window=3), dict(window=-1), dict(window=True), dict(window=1.5), dict(origin=5), dict(origin=(1 << 21, 0)),
             dict(origin=(0, 1, 2)), dict(code=False))
    for kw in plain:
        with pytest.raises(FotgError):
            subtract_background(fr, pl, flows=fl, **kw)
        with pytest.raises(FotgError):
            subtract_background(fr, pl, motions=mo, **kw)
        with pytest.raises(FotgError):
            upsample_crop_subtract_background(_Ctx(), torch.zeros((2, 4, 6, 2)), fr, pl, **kw)
    for kw in (dict(), dict(flows=fl, motions=mo), dict(flows=[1, 2]), dict(motions=torch.zeros((2, 3, 6), dtype=torch.float64)),
               dict(flows=torch.zeros((8, 12))), dict(flows=fl), dict(motions=mo)):        # the last two: host tensors
        with pytest.raises(FotgError):
            subtract_background(fr, pl, **kw)
    depth = _Ctx()
    depth.nch = 1
    for ctx, cf in ((depth, torch.zeros((2, 4, 6, 2))), (_Ctx(), torch.zeros((3, 4, 6, 2))), (_Ctx(), torch.zeros((4, 6, 2))), (_Ctx(), None),
                    (_Ctx(), torch.zeros((2, 4, 6, 2)))):                                     # the last: host tensors
        for fused in (True, False):
            with pytest.raises(FotgError):
                upsample_crop_subtract_background(ctx, cf, fr, pl, fused=fused)


# ---- the end-to-end inequalities on the oracle's flows ---------------------------------------------------------------------------
def test_fitted_motions_align_the_plate_and_the_patch_stands_out_on_the_oracles_flows(natural_images):
    """what tests/test_gpu_subtract.py asserts of OFClass.foreground on the GPU, here through the oracle's flows, motion_ref.fit,
    plate_ref and the restatement"""
    from oracle import oracle as O
    frames, _, _, _, foot = PR.crops_scene(natural_images["road_HD"], T=8, w=PR.BIG_W, h=PR.BIG_H)
    K, h, w = frames.shape
    fr = frames.astype(f32)
    fits = [M.fit(O.full_flow(fr[k], fr[k + 1], op=2), None, 2, 3) for k in range(K - 1)]
    exclude = np.zeros((K, h, w), np.uint8)
    exclude[:K - 1] = np.stack([f["code"] == 1 for f in fits])
    est = PR.plate_motions(np.stack([f["params"] for f in fits]), 0)
    plate, _, pcode, _, _ = PR.plate(frames, np.arange(K)[None], w, h, params=est[None], exclude=exclude)
    fitted = R.subtract(frames, plate, params=R.frame_motions(est), plate_code=pcode)
    ident = R.subtract(frames, plate, params=np.zeros((K, 6)), plate_code=pcode)
    out_f, in_f, out_i, in_i = figures(fitted, ident, foot)
    assert out_f < out_i and in_f > out_f


def figures(fitted, ident, foot):
    """mean Dq in grey levels: outside and inside the patch's footprint with the fitted motions, then with identity motions;
    printed, for the two inequalities of the end-to-end tests"""
    out = []
    for code, diff in (fitted[:2], ident[:2]):
        adm = (code != 2) & (code != 3)
        out += [diff[adm & (foot == 0)].mean() / 16.0, diff[adm & (foot == 1)].mean() / 16.0]
    print("mean difference in grey levels, outside / inside the footprint: fitted motions %.3f / %.3f, identity motions %.3f / %.3f"
          % tuple(out))
    return out
