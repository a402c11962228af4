"""The object removal on the GPU: fotg_erase / fotg_erase_motion / fotg_upsample_crop_erase equal the numpy restatement
tests/erase_ref.py byte for byte in dst, code, alpha and stats, for both sources, both pixel types, one and three channels and six
(grow, feather) pairs, on frames that leave the plate on every side; masks placed against the tile's geometry (corners, borders,
exactly G, G + F and G + F + 1 pixels from a tile edge, empty, full) on frames that cross the tile in both directions and on
frames smaller than the halo; the pixels it keeps for want of a plate are those the background subtraction calls 2 or 3; the
fused form equals the dense one; each output alone, single and batched calls and repeated calls give the same bytes; grow_mask is
a disc dilation; OFClass.remove_objects is the documented composition and on the jittered-crops scene brings the patch's footprint
back to the underlying image as closely as the plate allows; the tool writes what the call returns."""
import numpy as np
import pytest
import torch

import erase_ref as R
import plate_ref as PR
from host_checks import read_png_rgb, run_cli
from test_erase import _clean_crops
from test_gpu_subtract import CANVAS, FRAME, case, host, images, sources
from test_gpu_warp import dev, make_ctx, np_same_bits, same_bits

pytestmark = pytest.mark.gpu

f32 = np.float32
NAMES = ("dst", "code", "alpha", "stats")
GF = [(0, 0), (0, 1), (2, 3), (8, 8), (0, 8), (8, 0)]


def removal(frame=FRAME, n=3):
    """a blob with masked and unknown pixels under it; single pixels near two corners; the left border and the opposite corner"""
    h, w = frame
    rm = np.zeros((n, h, w), np.uint8)
    rm[0, 5:12, 4:15] = 1
    rm[1 % n, 2, w - 11] = 255
    rm[1 % n, h - 3, 8] = 2
    rm[2 % n, :, 0] = 1
    rm[2 % n, h - 1, w - 1] = 7
    return rm


def gpu(frames, plates, remove, canvas, src, index=None, **kw):
    from flowonthego_amd.erase import remove_objects
    ox, oy = canvas[2:]
    a = {k: (dev(v) if isinstance(v, np.ndarray) else v) for k, v in dict(kw, **src).items()}
    out = remove_objects(dev(frames), dev(plates), dev(remove), index=None if index is None else list(index), origin=(ox, oy), dst=True,
                         code=True, alpha=True, stats=True, **a)
    torch.cuda.synchronize()
    return [host(o) for o in out]


def ref(frames, plates, remove, canvas, src, index=None, **kw):
    src = {("params" if k == "motions" else k): v for k, v in src.items()}
    return R.erase(frames, plates, remove, index, canvas[2], canvas[3], **src, **kw)


def assert_same(got, want, what):
    for g, w_, nm in zip(got, want, NAMES):
        assert np_same_bits(g, w_), (what, nm, np.argwhere(g != w_)[:5])


@pytest.mark.parametrize("G,F", GF)
@pytest.mark.parametrize("noc,u8", [(1, False), (1, True), (3, False), (3, True)])
@pytest.mark.parametrize("source", ["dense", "motion"])
def test_gpu_equals_the_restatement(source, noc, u8, G, F):
    frames, plates, index, flows, motions, pcode, mask = case(noc, u8, 100 * G + 10 * F + 2 * noc + u8)
    src = sources(flows, motions)[source]
    rm = removal()
    kw = dict(plate_code=pcode, mask=mask, grow=G, feather=F)
    want = ref(frames, plates, rm, CANVAS, src, index, **kw)
    assert_same(gpu(frames, plates, rm, CANVAS, src, index, **kw), want, "masks")
    # the case is not an empty one: every code the pair allows (without a ramp nothing is blended), holes, and for float frames
    # a NaN pixel that was replaced
    tab = R.alpha_table(G, F)
    ramp = bool(((tab > 0) & (tab < 256)).any())              # (0, 0), (8, 0) and (0, 1), whose only weight below 256 is that of D2 = 1: 0
    seen = set(np.unique(want[1]).tolist())
    assert seen == ({0, 1, 2, 3, 4} if ramp else {0, 1, 2, 3}) and ramp == ((G, F) in ((2, 3), (8, 8), (0, 8))), seen
    assert want[3][:, 5].sum() > 0 and (want[3][:, 6] == (rm != 0).sum((1, 2))).all()
    # without masks
    assert_same(gpu(frames, plates, rm, CANVAS, src, index, grow=G, feather=F), ref(frames, plates, rm, CANVAS, src, index, grow=G, feather=F), "plain")


def tile_masks(h, w, G, F):
    """one frame per pattern: single pixels at the corners of the 64 x 16 tiles; each frame border; pixels exactly d = G, G + F and
    G + F + 1 away from the first tile edge on both axes, on either side of it; nothing; everything"""
    pats = []
    rm = np.zeros((h, w), np.uint8)
    for y in (0, 15, 16, 31, 32, h - 1):
        for x in (0, 63, 64, 127, 128, w - 1):
            if y < h and x < w:
                rm[y, x] = 1
    pats.append(rm)
    for sl in ((0, slice(None)), (h - 1, slice(None)), (slice(None), 0), (slice(None), w - 1)):
        rm = np.zeros((h, w), np.uint8)
        rm[sl] = 1
        pats.append(rm)
    for d in (G, G + F, G + F + 1):
        rm = np.zeros((h, w), np.uint8)
        for x, y in ((63 + d, 5), (64 - d, h - 6), (10, 15 + d), (w - 10, 16 - d)):      # d beyond the tile's last / first column and row
            if 0 <= x < w and 0 <= y < h:
                rm[y, x] = 1
        pats.append(rm)
    pats.append(np.zeros((h, w), np.uint8))
    pats.append(np.full((h, w), 1, np.uint8))
    return np.stack(pats)


@pytest.mark.parametrize("h,w", [(37, 131), (17, 65), (5, 3), (1, 1)])
def test_masks_against_the_tile_geometry(h, w):
    canvas = (w + 4, h + 3, 2, 1)
    for noc, u8, source, G, F in ((3, True, "dense", 8, 8), (1, False, "motion", 8, 8), (1, True, "motion", 2, 3), (3, False, "dense", 0, 1)):
        rm = tile_masks(h, w, G, F)
        n = len(rm)
        frames, plates, index, flows, motions, pcode, mask = case(noc, u8, h + 7 * G + noc, (h, w), canvas, n, 2)
        src = sources(flows, motions)[source]
        kw = dict(plate_code=pcode, mask=mask, grow=G, feather=F)
        got, want = gpu(frames, plates, rm, canvas, src, index, **kw), ref(frames, plates, rm, canvas, src, index, **kw)
        assert_same(got, want, (h, w, noc, source, G, F))
        # the empty mask: the frame bit for bit, nothing else; the full one: every pixel under full weight
        assert np_same_bits(got[0][n - 2], frames[n - 2]) and not got[1][n - 2].any() and not got[2][n - 2].any()
        assert got[3][n - 2].tolist() == [h * w, 0, 0, 0, 0, 0, 0, 0]
        assert (got[2][n - 1] == 256).all() and got[3][n - 1, 6] == h * w and got[3][n - 1, 7] == 256 * h * w and got[3][n - 1, 0] == 0
        # no mask at all in the batch: every workgroup takes the copy path
        none = np.zeros_like(rm)
        e = gpu(frames, plates, none, canvas, src, index, **kw)
        assert np_same_bits(e[0], frames) and not e[1].any() and not e[2].any() and (e[3][:, 0] == h * w).all() and not e[3][:, 1:].any()


def test_the_copy_path_on_frames_that_are_not_aligned():
    """slices whose first byte sits at every offset from a 16-byte boundary, source and destination aligned alike or not"""
    from flowonthego_amd import lib
    from flowonthego_amd._args import _ptr, _stream
    h, w, n = 19, 83, 2
    rng = np.random.default_rng(5)
    for noc, dt in ((1, torch.uint8), (3, torch.uint8), (1, torch.float32)):
        el = 1 if dt == torch.uint8 else 4
        size = n * h * w * noc
        src_buf = torch.from_numpy(rng.integers(0, 255, size + 64, dtype=np.uint8) if el == 1 else rng.random(size + 64, dtype=f32)).cuda()
        rm = torch.zeros((n, h, w), dtype=torch.uint8, device="cuda")
        mo = torch.zeros((n, 6), dtype=torch.float64, device="cuda")
        pl = torch.zeros((1, h, w, noc), dtype=dt, device="cuda")
        fn = lib().fotg_erase_motion_u8 if el == 1 else lib().fotg_erase_motion
        for so, do in ((0, 0), (1, 1), (5, 5), (15, 15), (3, 8), (0, 7)) if el == 1 else ((0, 0), (1, 1), (3, 3), (1, 2)):
            dst_buf = torch.full((size + 64,), 77, dtype=dt, device="cuda")
            s, d = src_buf[so:so + size], dst_buf[do:do + size]
            assert fn(0, n, _ptr(s), w, h, noc, 1, _ptr(pl), w, h, 0, 0, None, _ptr(mo), None, None, _ptr(rm), 2, 3, _ptr(d), None, None, None,
                      _stream(torch.device("cuda", 0))) == 0
            torch.cuda.synchronize()
            assert same_bits(d, s), (noc, dt, so, do)
            assert (dst_buf[:do] == 77).all() and (dst_buf[do + size:] == 77).all()          # nothing written outside


@pytest.mark.parametrize("noc", [1, 3])
def test_kept_pixels_are_those_the_subtraction_calls_2_or_3(noc):
    from flowonthego_amd.subtract import subtract_background
    frames, plates, index, flows, motions, pcode, mask = case(noc, True, 70 + noc)
    for rm in (removal(), np.ones((3,) + FRAME, np.uint8)):
        for source, src in sources(flows, motions).items():
            _, code, alpha, _ = gpu(frames, plates, rm, CANVAS, src, index, plate_code=pcode, mask=mask, grow=2, feather=3)
            a = {k: dev(v) for k, v in src.items()}
            sub = host(subtract_background(dev(frames), dev(plates), index=list(index), origin=CANVAS[2:], plate_code=dev(pcode), mask=dev(mask),
                                           window=0, **a))
            kept = (alpha > 0) & ((code == 2) | (code == 3))
            assert np.array_equal(kept, (alpha > 0) & ((sub == 2) | (sub == 3))), source
            assert np.array_equal(code[kept], sub[kept]) and kept.any() and (alpha > 0).any()


@pytest.mark.parametrize("noc,u8", [(1, False), (3, True)])
def test_fused_equals_dense_on_the_upsampled_flow(noc, u8):
    from flowonthego_amd.erase import remove_objects
    n = 3
    for w, h in ((130, 40), (67, 37)):                        # 67 x 37: the pyramid pads to 68 x 40
        rng = np.random.default_rng(600 + noc + w)
        o = make_ctx(2, w, h, max_batch=n, finest_scale=1, coarsest_scale=2, use_var_ref=False)
        wl, hl = o.out_size()
        cf = (rng.standard_normal((n, hl, wl, 2)) * 0.6).astype(f32)
        cf[0, 0, :3] = (np.nan, 0.0)
        cf[-1, hl // 2, :2] = (np.inf, 1.0)
        frames, plates = dev(images(rng, (n, h, w), noc, u8, ramp=True)), dev(images(rng, (2, h + 2, w + 3), noc, u8))
        rm = np.zeros((n, h, w), np.uint8)
        rm[0, :9, :40] = 1
        rm[1, h // 2, w // 2] = 1
        rm[2, h - 4:, w - 30:] = 1
        kw = dict(index=[1, 0, 1], origin=(1, 2), plate_code=dev(rng.choice(np.array([0] * 15 + [1], np.uint8), (2, h + 2, w + 3))),
                  mask=dev(rng.choice(np.array([0] * 15 + [3], np.uint8), (n, h, w))), grow=3, feather=5, dst=True, code=True, alpha=True, stats=True)
        got = o.upsample_crop_remove_objects(dev(cf), frames, plates, dev(rm), fused=True, **kw)
        unf = o.upsample_crop_remove_objects(dev(cf), frames, plates, dev(rm), fused=False, **kw)
        want = remove_objects(frames, plates, dev(rm), flows=o.upsample_crop(dev(cf)), **kw)
        torch.cuda.synchronize()
        for g, u, w_, nm in zip(got, unf, want, NAMES):
            assert same_bits(g, w_) and same_bits(u, w_), nm
        assert len(torch.unique(want[1])) >= 4
        o.close()


def test_each_output_alone_single_calls_repeats_and_the_sums_of_the_maps():
    from flowonthego_amd.erase import remove_objects
    frames, plates, index, flows, motions, pcode, mask = case(3, False, 9, (33, 129), (131, 30, 1, -2))
    rm_np = removal((33, 129))
    fr, pl, fl, mo, pc, mk, rm = (dev(v) for v in (frames, plates, flows, motions, pcode, mask, rm_np))
    kw = dict(index=list(index), origin=(1, -2), plate_code=pc, mask=mk, grow=3, feather=4)
    flags = ("dst", "code", "alpha", "stats")
    for src in (dict(flows=fl), dict(motions=mo)):
        full = remove_objects(fr, pl, rm, **src, **kw, dst=True, code=True, alpha=True, stats=True)
        again = remove_objects(fr, pl, rm, **src, **kw, dst=True, code=True, alpha=True, stats=True)
        torch.cuda.synchronize()
        for x, y, nm in zip(full, again, NAMES):
            assert same_bits(x, y), nm                                             # the same bytes every time, stats included
        for j, keep in enumerate(flags):
            one = remove_objects(fr, pl, rm, **src, **kw, **{f: f == keep for f in flags})
            assert isinstance(one, torch.Tensor) and same_bits(one, full[j]), keep
        # single calls against the batch
        for i in range(len(frames)):
            s = {k: v[i] for k, v in src.items()}
            one = remove_objects(fr[i], pl[int(index[i])], rm[i], **s, origin=(1, -2), plate_code=pc[int(index[i])], mask=mk[i], grow=3, feather=4,
                                 dst=True, code=True, alpha=True, stats=True)
            for x, y, nm in zip(one, full, NAMES):
                assert same_bits(x, y[i]), (i, nm)
        # stats are the sums of the returned maps
        _, code, alpha, stats = (host(t) for t in full)
        for i in range(len(frames)):
            holes = ((alpha[i] == 256) & ((code[i] == 2) | (code[i] == 3))).sum()
            assert stats[i].tolist() == np.bincount(code[i].ravel(), minlength=5).tolist() + [holes, (rm_np[i] != 0).sum(), alpha[i].astype(np.int64).sum()]
        assert not code[alpha == 0].any() and (code[alpha > 0] > 0).all()


@pytest.mark.parametrize("G", range(9))
def test_grow_mask_is_a_disc_dilation(G):
    import flowonthego_amd as F
    rng = np.random.default_rng(G)
    for shape in ((3, 37, 131), (5, 3), (2, 1, 1), (40, 200)):
        rm = (rng.random(shape) < 0.01).astype(np.uint8) * 200
        rm.reshape(-1)[0] = 1
        got = host(F.grow_mask(dev(rm), G))
        assert got.dtype == np.uint8 and np.array_equal(got, R.disc_dilation(rm, G)), shape
    assert not host(F.grow_mask(dev(np.zeros((7, 9), np.uint8)), G)).any()


# ---- OFClass.remove_objects --------------------------------------------------------------------------------------------------------
def test_ofclass_remove_objects_is_the_documented_composition_and_restores_the_scene(natural_images):
    """640 x 384 crops of the jittered-crops walk, the scene of OFClass.foreground's end-to-end test.  The three mean absolute
    differences from the underlying clean image are taken over the pixels of the patch's footprint whose true position in frame
    0 lies on the plate's grid, where the plate's own difference is defined (the plate is on the frame grid, not a mosaic); they
    are printed, with the figures over the whole footprint, before they are asserted."""
    import flowonthego_amd as F
    from flowonthego_amd.erase import ofc_remove_objects
    frames_np, motions, canvas, truth, foot = PR.crops_scene(natural_images["road_HD"], T=8, w=PR.BIG_W, h=PR.BIG_H)
    K, h, w = frames_np.shape
    frames = dev(frames_np)
    o = make_ctx(2, w, h, max_batch=K - 1)
    clean, code, mask, plate = o.remove_objects(frames)
    # the composition, call for call
    m, _, _, pl, _ = o.foreground(frames)
    _, pcode, _ = o.background(frames)
    params = F.upsample_crop_fit_motion(o, o.calc_sequence(frames), None, "affine", code=True)[0]
    back = F.frame_motions(F.plate_motions(params, 0))
    c2, cd2 = F.remove_objects(frames, pl, m, motions=back, plate_code=pcode, grow=2, feather=3, dst=True, code=True)
    torch.cuda.synchronize()
    for x, y, nm in zip((clean, code, mask, plate), (c2, cd2, m, pl), ("clean", "code", "mask", "plate")):
        assert same_bits(x, y), nm
    assert clean.shape == frames.shape and clean.dtype == torch.uint8 and mask.any() and (code == 1).any() and (code == 4).any()
    # other arguments, and a mask of one's own in place of the objects found
    own = dev(foot)
    got = ofc_remove_objects(o, frames, ref=2, model="similarity", grow=1, feather=0, mask=own)
    pl2, pc2, _ = o.background(frames, ref=2, model="similarity")
    back2 = F.frame_motions(F.plate_motions(F.upsample_crop_fit_motion(o, o.calc_sequence(frames), None, "similarity", code=True)[0], 2))
    want = F.remove_objects(frames, pl2, own, motions=back2, plate_code=pc2, grow=1, feather=0, dst=True, code=True)
    torch.cuda.synchronize()
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]) and got[2] is own and same_bits(got[3], pl2)
    with pytest.raises(F.FotgError):
        o.remove_objects(frames, grow=9)
    with pytest.raises(F.FotgError):
        o.remove_objects(frames[:1])

    # the quality: frame 0 is the reference, so the plate's grid is frame 0's and its underlying image is frame 0's clean crop
    back_true = np.zeros_like(motions)
    back_true[:, 2], back_true[:, 5] = -motions[:, 2], -motions[:, 5]
    crops, _ = _clean_crops(dict(frames=frames_np, back=back_true, canvas=canvas, truth=truth))
    plate_np, clean_np = host(plate).astype(np.float64), host(clean).astype(np.float64)
    before, after, own_err, n_pix = [], [], [], 0
    for k in range(K):
        ys, xs = np.nonzero(foot[k])
        X, Y = xs + int(back_true[k, 2]), ys + int(back_true[k, 5])                  # the pixel's true position in frame 0
        ok = (X >= 0) & (X < w) & (Y >= 0) & (Y < h)
        ys, xs, X, Y = ys[ok], xs[ok], X[ok], Y[ok]
        before.append(np.abs(frames_np[k, ys, xs].astype(np.float64) - crops[k, ys, xs]))
        after.append(np.abs(clean_np[k, ys, xs] - crops[k, ys, xs]))
        own_err.append(np.abs(plate_np[Y, X] - crops[0, Y, X]))
        n_pix += len(ys)
    before, after, own_err = (np.concatenate(v).mean() for v in (before, after, own_err))
    whole = lambda a: np.abs(a.astype(np.float64) - crops)[foot == 1].mean()
    holes = int((((host(code) == 2) | (host(code) == 3)) & (foot == 1)).sum())
    print("mean absolute difference from the clean image inside the footprint (%d pixels): before %.3f, after %.3f, the plate's own %.3f; "
          "over the whole footprint before %.3f, after %.3f; %d footprint pixels kept for want of a plate; the mask covers %.3f of the footprint"
          % (n_pix, before, after, own_err, whole(frames_np), whole(host(clean)), holes, host(mask)[foot == 1].mean()))
    assert n_pix > 0.9 * foot.sum()
    assert after < before
    assert after <= own_err + 0.5
    # what the removal itself costs: the footprint as the mask and the clean image of frame 0 as the plate, along the fitted motions
    ideal = host(F.remove_objects(frames, dev(crops[0]), own, motions=back, grow=2, feather=3))
    print("with the clean image as the plate and the footprint as the mask: after %.3f over the whole footprint" % whole(ideal))
    assert whole(ideal) < whole(frames_np)
    o.close()


# ---- the tool ----------------------------------------------------------------------------------------------------------------------
def test_cli_writes_what_the_call_returns(tmp_path, natural_images):
    import motion_ref as M
    from flowonthego_amd._cli import sequence_context
    frames, _ = M.jittered_crops(natural_images["road_HD"], T=4, patch=True)
    fr, out, cd, pl = (str(tmp_path / n) for n in ("f.npy", "out.npy", "code.npy", "plate.png"))
    np.save(fr, frames)
    run = run_cli("remove_objects", [fr, out, "--ref", "1", "--model", "similarity", "--low", "6", "--high", "30", "--window", "2", "--min-area", "32",
                                     "--grow", "3", "--feather", "2", "--code", cd, "--plate", pl])
    assert run.returncode == 0, run.stderr
    ofc = sequence_context(frames, 2, bidir=False, max_batch=4)
    clean, code, mask, plate = ofc.remove_objects(torch.from_numpy(frames).cuda(), ref=1, model="similarity", low=6.0, high=30.0, window=2,
                                                  min_area=32, grow=3, feather=2)
    clean, code, plate = clean.cpu().numpy(), code.cpu().numpy(), plate.cpu().numpy()
    got = np.load(out)
    assert got.dtype == np.uint8 and got.shape == frames.shape and np.array_equal(got, clean) and mask.any() and (got != frames).any()
    assert np.array_equal(np.load(cd), code)
    assert np.array_equal(read_png_rgb(pl), np.broadcast_to(plate[..., None], plate.shape + (3,)))
    lines = run.stdout.strip().splitlines()
    assert lines[0] == "objects removed from 5 frames of 320 x 192 with the plate on frame 1, grow 3, feather 2:" and len(lines) == 6
    for k in range(5):
        assert lines[1 + k] == "  frame %d: replaced %.4f, blended %.4f, %d pixels kept for want of a plate or a vector" \
            % (k, (code[k] == 1).mean(), (code[k] == 4).mean(), ((code[k] == 2) | (code[k] == 3)).sum())
    ofc.close()
