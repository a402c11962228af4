"""The background subtraction on the GPU: fotg_subtract / fotg_subtract_motion / fotg_upsample_crop_subtract equal the numpy
restatement tests/subtract_ref.py byte for byte in code, diff, evidence and stats, for both sources, both pixel types, one and three
channels and every window, on frames that leave the plate on every side, that cross the tile in both directions and that are
smaller than the window; the three sources agree; each output alone, single and batched calls and repeated calls give the same
bytes; OFClass.foreground is the documented composition, and on the jittered-crops scene the fitted motions align the plate and
the patch stands out."""
import numpy as np
import pytest
import torch

import plate_ref as PR
import subtract_ref as R
from test_gpu_warp import dev, make_ctx, np_same_bits, same_bits
from test_subtract import figures

pytestmark = pytest.mark.gpu

f32 = np.float32
FRAME = (23, 61)                      # h, w
CANVAS = (67, 19, 5, -3)              # W, H, ox, oy: frame pixels leave the plate on every side
NAMES = ("code", "diff", "evidence", "stats")


def host(t):
    return None if t is None else t.cpu().numpy()


def images(rng, shape, noc, u8, ramp=False):
    """grey levels 100 .. 130; with ramp a noise is added whose amplitude grows from 0 at the left edge to 200 at the right one, so
    that against a plate without it the difference passes both thresholds on the way; float images get NaN pixels"""
    shape = tuple(shape) + ((noc,) if noc > 1 else ())
    a = rng.uniform(100, 130, shape)
    if ramp:
        amp = 200.0 * np.arange(shape[2]) / max(shape[2] - 1, 1)
        a = a + rng.uniform(-1, 1, shape) * amp.reshape((1, 1, -1) + (1,) * (len(shape) - 3))
    if u8:
        return np.clip(np.rint(a), 0, 255).astype(np.uint8)
    a = a.astype(f32)
    if a.size >= 97:
        flat = a.reshape(-1)
        flat[rng.choice(flat.size, flat.size // 97, replace=False)] = np.nan
    return a


def case(noc, u8, seed, frame=FRAME, canvas=CANVAS, n=3, P=2):
    """frames, plates, index, dense flows, motions, plate_code, mask of one comparison"""
    rng = np.random.default_rng(seed)
    W, H, ox, oy = canvas
    h, w = frame
    frames = images(rng, (n, h, w), noc, u8, ramp=True)
    plates = images(rng, (P, H, W), noc, u8)
    if not u8:
        frames.reshape(n, -1)[:, ::1009] = 1e6                                     # differences beyond 2047.9 levels
    index = rng.integers(0, P, n)
    flows = (rng.standard_normal((n, h, w, 2)) * 2.0).astype(f32)
    flows[:, :, : w // 2] = np.round(flows[:, :, : w // 2] * 4) / 4                 # quarter pixels and whole pixels among the fractions
    flows[0, : h // 2] = np.round(flows[0, : h // 2])
    flat = flows.reshape(-1)
    if flat.size >= 61:
        bad = rng.choice(flat.size, flat.size // 61, replace=False)
        flat[bad] = np.array([np.nan, np.inf, -np.inf, 3e38, -1e30], f32)[np.arange(bad.size) % 5]
    motions = rng.normal(0, 0.02, (n, 6))
    motions[:, [2, 5]] = rng.normal(0, 2.5, (n, 2))
    motions[0] = 0
    pcode = rng.choice(np.array([0] * 20 + [1, 2], np.uint8), (P, H, W))
    mask = rng.choice(np.array([0] * 20 + [1, 3, 200], np.uint8), (n, h, w))
    return frames, plates, index, flows, motions, pcode, mask


def gpu(frames, plates, canvas, src, index=None, **kw):
    from flowonthego_amd.subtract import subtract_background
    ox, oy = canvas[2:]
    a = {k: (dev(v) if isinstance(v, np.ndarray) else v) for k, v in dict(kw, **src).items()}
    out = subtract_background(dev(frames), dev(plates), index=None if index is None else list(index), origin=(ox, oy), code=True, diff=True,
                              evidence=True, stats=True, **a)
    torch.cuda.synchronize()
    return [host(o) for o in out]


def ref(frames, plates, canvas, src, index=None, **kw):
    src = {("params" if k == "motions" else k): v for k, v in src.items()}
    return R.subtract(frames, plates, index, canvas[2], canvas[3], **src, **kw)


def assert_same(got, want, what):
    for g, w_, nm in zip(got, want, NAMES):
        assert np_same_bits(g, w_), (what, nm, np.argwhere(g != w_)[:5])


def sources(flows, motions):
    return dict(dense=dict(flows=flows), motion=dict(motions=motions))


@pytest.mark.parametrize("r", [0, 1, 2])
@pytest.mark.parametrize("noc,u8", [(1, False), (1, True), (3, False), (3, True)])
@pytest.mark.parametrize("source", ["dense", "motion"])
def test_gpu_equals_the_restatement(source, noc, u8, r):
    frames, plates, index, flows, motions, pcode, mask = case(noc, u8, 100 * r + 10 * noc + u8)
    src = sources(flows, motions)[source]
    kw = dict(plate_code=pcode, mask=mask, low=20.0, high=60.0, window=r)
    want = ref(frames, plates, CANVAS, src, index, **kw)
    assert_same(gpu(frames, plates, CANVAS, src, index, **kw), want, "masks")
    seen = set(np.unique(want[0]).tolist())
    assert seen == {0, 1, 2, 3, 4}, seen
    # without masks, at the default thresholds
    assert_same(gpu(frames, plates, CANVAS, src, index, window=r), ref(frames, plates, CANVAS, src, index, window=r), "plain")


@pytest.mark.parametrize("r", [0, 1, 2])
@pytest.mark.parametrize("h,w", [(17, 65), (33, 129), (5, 3), (1, 1)])
def test_one_pixel_past_the_tile_and_frames_smaller_than_the_window(h, w, r):
    """65 x 17 and 129 x 33: the halo crosses tile borders in both directions; 3 x 5 and 1 x 1: the store tail and a window larger
    than the frame.  P = 1, P = n without an index, and an explicit index."""
    canvas = (w + 4, h + 3, 2, 1)
    for noc, u8, source, n, P, explicit in ((3, False, "dense", 2, 1, False), (1, True, "motion", 3, 3, False), (1, False, "dense", 3, 2, True)):
        frames, plates, index, flows, motions, pcode, mask = case(noc, u8, h + 7 * r + noc, (h, w), canvas, n, P)
        src = sources(flows, motions)[source]
        ix = index if explicit else None
        kw = dict(plate_code=pcode, mask=mask, low=30.0, high=70.0, window=r)
        assert_same(gpu(frames, plates, canvas, src, ix, **kw), ref(frames, plates, canvas, src, ix, **kw), (h, w, r, noc, source))


def test_thresholds_at_zero_at_equality_and_at_the_cap():
    h, w = 6, 9
    frame = np.zeros((1, h, w), f32)
    frame[0, 2, 3] = 9.0
    frame[0, 4, 7] = 1e9
    plate = np.zeros((1, h, w), f32)
    z = np.zeros((1, h, w, 2), f32)
    for low, high, r in ((1.0, 1.0, 1), (1.0, 1.0 + 1 / 16, 1), (0.0, 0.0, 0), (0.0, 2047.9375, 0), (2047.9375, 2047.9375, 2), (0.5, 3.0, 2)):
        want = R.subtract(frame, plate, flows=z, low=low, high=high, window=r)
        assert_same(gpu(frame, plate, (w, h, 0, 0), dict(flows=z), low=low, high=high, window=r), want, (low, high, r))
    eq = R.subtract(frame, plate, flows=z, low=1.0, high=1.0 + 1 / 16, window=1)[0]
    assert eq[0, 2, 3] == 1 and eq[0, 0, 3] == 0                                    # S = 144 = L C at the centre
    cap = R.subtract(frame, plate, flows=z, low=0.0, high=2047.9375, window=0)
    assert cap[1][0, 4, 7] == 32767 and cap[0][0, 4, 7] == 4 and (cap[0] >= 1).all()


# ---- the routes agree --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noc,u8", [(1, True), (3, False)])
def test_motion_source_equals_dense_on_motion_flow(noc, u8):
    from flowonthego_amd.motion import motion_flow
    from flowonthego_amd.subtract import subtract_background
    frames, plates, index, _, motions, pcode, mask = case(noc, u8, 40 + noc)
    h, w = FRAME
    mo = dev(motions)
    kw = dict(index=list(index), origin=CANVAS[2:], plate_code=dev(pcode), mask=dev(mask), low=20.0, high=60.0, window=2, code=True, diff=True,
              evidence=True, stats=True)
    a = subtract_background(dev(frames), dev(plates), motions=mo, **kw)
    b = subtract_background(dev(frames), dev(plates), flows=motion_flow(mo, w, h), **kw)
    torch.cuda.synchronize()
    for x, y, nm in zip(a, b, NAMES):
        assert same_bits(x, y), nm
    assert (a[0] == 0).any() and (a[0] == 2).any()


@pytest.mark.parametrize("noc,u8", [(1, False), (3, True)])
def test_fused_equals_dense_on_the_upsampled_flow(noc, u8):
    from flowonthego_amd.subtract import subtract_background
    n = 3
    for w, h in ((130, 40), (67, 37)):                        # 67 x 37: the pyramid pads to 68 x 40
        rng = np.random.default_rng(500 + noc + w)
        o = make_ctx(2, w, h, max_batch=n, finest_scale=1, coarsest_scale=2, use_var_ref=False)
        wl, hl = o.out_size()
        cf = (rng.standard_normal((n, hl, wl, 2)) * 0.6).astype(f32)
        cf[0, 0, :3] = (np.nan, 0.0)
        cf[-1, hl // 2, :2] = (np.inf, 1.0)
        frames, plates = dev(images(rng, (n, h, w), noc, u8, ramp=True)), dev(images(rng, (2, h + 2, w + 3), noc, u8))
        kw = dict(index=[1, 0, 1], origin=(1, 2), plate_code=dev(rng.choice(np.array([0] * 15 + [1], np.uint8), (2, h + 2, w + 3))),
                  mask=dev(rng.choice(np.array([0] * 15 + [3], np.uint8), (n, h, w))), window=1, code=True, diff=True, evidence=True, stats=True)
        got = o.upsample_crop_subtract_background(dev(cf), frames, plates, fused=True, **kw)
        unf = o.upsample_crop_subtract_background(dev(cf), frames, plates, fused=False, **kw)
        want = subtract_background(frames, plates, flows=o.upsample_crop(dev(cf)), **kw)
        torch.cuda.synchronize()
        for g, u, w_, nm in zip(got, unf, want, NAMES):
            assert same_bits(g, w_) and same_bits(u, w_), nm
        assert len(torch.unique(want[0])) >= 4
        o.close()


# ---- properties --------------------------------------------------------------------------------------------------------------------
def test_each_output_alone_single_calls_repeats_and_the_sums_of_the_maps():
    from flowonthego_amd.subtract import subtract_background
    frames, plates, index, flows, motions, pcode, mask = case(3, False, 9, (33, 129), (131, 30, 1, -2))
    fr, pl, fl, mo, pc, mk = (dev(v) for v in (frames, plates, flows, motions, pcode, mask))
    kw = dict(index=list(index), origin=(1, -2), plate_code=pc, mask=mk, window=2, low=20.0, high=60.0)
    flags = ("code", "diff", "evidence", "stats")
    for src in (dict(flows=fl), dict(motions=mo)):
        full = subtract_background(fr, pl, **src, **kw, code=True, diff=True, evidence=True, stats=True)
        again = subtract_background(fr, pl, **src, **kw, code=True, diff=True, evidence=True, stats=True)
        torch.cuda.synchronize()
        for x, y, nm in zip(full, again, NAMES):
            assert same_bits(x, y), nm                                             # the same bytes every time, stats included
        for j, keep in enumerate(flags):
            one = subtract_background(fr, pl, **src, **kw, **{f: f == keep for f in flags})
            assert isinstance(one, torch.Tensor) and same_bits(one, full[j]), keep
        # single calls against the batch
        for i in range(len(frames)):
            s = {k: v[i] for k, v in src.items()}
            one = subtract_background(fr[i], pl[int(index[i])], **s, origin=(1, -2), plate_code=pc[int(index[i])], mask=mk[i], window=2,
                                      low=20.0, high=60.0, code=True, diff=True, evidence=True, stats=True)
            for x, y, nm in zip(one, full, NAMES):
                assert same_bits(x, y[i]), (i, nm)
        # stats are the sums of the returned maps
        code, diff, evidence, stats = (host(t) for t in full)
        for i in range(len(frames)):
            fg = (code[i] == 1) | (code[i] == 4)
            assert stats[i].tolist() == np.bincount(code[i].ravel(), minlength=5).tolist() + [diff[i].astype(np.int64).sum(), diff[i][fg].astype(np.int64).sum()]
        assert np.array_equal(evidence[..., 0], (code == 4).astype(f32)) and np.array_equal(evidence[..., 1] * 16, diff.astype(f32))
        assert not diff[(code == 2) | (code == 3)].any()


def test_foreground_objects_is_the_hysteresis():
    import flowonthego_amd as F
    import objects_ref as OR
    code = np.zeros((2, 40, 50), np.uint8)
    code[0, 5:15, 5:20] = 1
    code[0, 9, 9] = 4
    code[0, 22:34, 25:40] = 1                                                       # weak only: not confirmed
    code[1, 3:13, 30:42] = 4
    evidence = np.zeros((2, 40, 50, 2), f32)
    evidence[..., 0] = code == 4
    evidence[..., 1] = np.where(code > 0, 12.25, 0)
    objects, ids, confirmed = F.foreground_objects(dev(code), dev(evidence))
    want = OR.components_batch(code, OR.fg_set((1, 4)), 8, evidence, min_area=64, max_objects=256)
    assert np.array_equal(host(objects), want["objects"]) and np.array_equal(host(ids), want["ids"])
    assert host(confirmed)[:, :3].tolist() == [[True, False, False], [True, False, False]] and confirmed.sum().item() == 2
    mask = host(F.foreground_mask(ids, confirmed))
    assert mask.dtype == np.uint8 and mask[0, 5:15, 5:20].all() and mask[1, 3:13, 30:42].all() and mask.sum() == 150 + 120


# ---- OFClass.foreground ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bidir", [False, True])
def test_ofclass_foreground_is_the_documented_composition(bidir, natural_images):
    import flowonthego_amd as F
    import motion_ref as M
    frames_np, _ = M.jittered_crops(natural_images["road_HD"], T=4, patch=True)
    frames = dev(frames_np)
    K, h, w = frames_np.shape
    o = make_ctx(2, w, h, max_batch=K - 1, bidir=bidir)
    for ref_, model, window, kw in ((0, "affine", 1, {}), (2, "similarity", 2, dict(low=6.0, high=30.0, min_area=32, max_objects=16))):
        mask, objects, confirmed, plate, code = o.foreground(frames, ref=ref_, model=model, window=window, **kw)
        pl, pcode, _ = o.background(frames, ref=ref_, model=model)
        if bidir:
            fw, bw = o.calc_sequence_bidirectional(frames)
            fmask = o.upsample_crop_fb_check(fw, bw)[0]
        else:
            fw, fmask = o.calc_sequence(frames), None
        motions = F.plate_motions(F.upsample_crop_fit_motion(o, fw, fmask, model, code=True)[0], ref_)
        c, ev = F.subtract_background(frames, pl, motions=F.frame_motions(motions), plate_code=pcode, low=kw.get("low", 8.0),
                                      high=kw.get("high", 24.0), window=window, code=True, evidence=True)
        ob, ids, conf = F.foreground_objects(c, ev, 8, kw.get("min_area", 64), kw.get("max_objects", 256))
        m = F.foreground_mask(ids, conf)
        torch.cuda.synchronize()
        for x, y, nm in zip((mask, objects, confirmed, plate, code), (m, ob, conf, pl, c), ("mask", "objects", "confirmed", "plate", "code")):
            assert same_bits(x, y), nm
        assert mask.shape == (K, h, w) and mask.dtype == torch.uint8 and confirmed.any() and mask.any()
    with pytest.raises(F.FotgError):
        o.foreground(frames[:1])
    with pytest.raises(F.FotgError):
        o.foreground(frames, low=30.0)
    o.close()


def test_fitted_motions_align_the_plate_and_the_patch_stands_out(natural_images):
    """the scene of tests/test_subtract.py's CPU form of this test: 640 x 384 crops of the jittered-crops walk"""
    import flowonthego_amd as F
    frames_np, _, _, _, foot = PR.crops_scene(natural_images["road_HD"], T=8, w=PR.BIG_W, h=PR.BIG_H)
    K, h, w = frames_np.shape
    frames = dev(frames_np)
    o = make_ctx(2, w, h, max_batch=K - 1)
    mask, objects, confirmed, plate, code = o.foreground(frames)
    pl, pcode, _ = o.background(frames)
    assert same_bits(pl, plate)
    params = F.upsample_crop_fit_motion(o, o.calc_sequence(frames), None, "affine", code=True)[0]
    motions = F.frame_motions(F.plate_motions(params, 0))
    fitted = F.subtract_background(frames, plate, motions=motions, plate_code=pcode, diff=True)
    ident = F.subtract_background(frames, plate, motions=torch.zeros_like(motions), plate_code=pcode, diff=True)
    torch.cuda.synchronize()
    assert same_bits(fitted[0], code)
    out_f, in_f, out_i, in_i = figures([host(t) for t in fitted], [host(t) for t in ident], foot)
    assert out_f < out_i and in_f > out_f
    m = host(mask)
    print("confirmed objects per frame: %s; the mask covers %.3f of the footprint and %.4f of the rest"
          % (host(confirmed).sum(1).tolist(), m[foot == 1].mean(), m[foot == 0].mean()))
    o.close()
