"""The background plate on the GPU: fotg_plate / fotg_plate_motion / fotg_upsample_crop_plate equal the numpy restatement
tests/plate_ref.py byte for byte in dst, count, code and stats, for every K at which the selection changes shape, both pixel types,
both modes and every launch shape; the three sources agree; the properties the definition promises hold; the documented refusals
launch nothing; OFClass.background is the documented composition, and on the jittered-crops scene its median plate is closer to
the underlying image than the mean and than the unaligned median."""
import ctypes as C

import numpy as np
import pytest
import torch

import motion_ref as M
import plate_ref as R
from test_gpu_warp import dev, make_ctx, np_same_bits, same_bits

pytestmark = pytest.mark.gpu

f32 = np.float32
FOTG_ERR_ARG = 1
FRAME = (23, 61)                      # h, w
CANVAS = (67, 19, 5, -3)              # W, H, ox, oy: tiles straddle the frame's edges, some pixels get no frame
T = 6


def host(t):
    return None if t is None else t.cpu().numpy()


def stack(rng, noc, u8, h=FRAME[0], w=FRAME[1], nframes=T):
    shape = (nframes, h, w) if noc == 1 else (nframes, h, w, noc)
    if u8:
        return rng.integers(0, 256, shape, dtype=np.uint8)
    a = rng.uniform(0, 255, shape).astype(f32)
    flat = a.reshape(-1)
    flat[rng.choice(flat.size, flat.size // 97, replace=False)] = np.nan
    return a


def case(K, noc, u8, seed, canvas=CANVAS, n=2):
    """frames, index, dense flows, motions, occ, exclude, ref of one comparison"""
    rng = np.random.default_rng(seed)
    W, H, ox, oy = canvas
    h, w = FRAME
    frames = stack(rng, noc, u8)
    index = rng.integers(0, T, (n, K))
    index[rng.random((n, K)) < 0.15] = -1
    index[0, 0] = 0                                                             # at least one sample
    flows = (rng.standard_normal((n, K, H, W, 2)) * 3.0).astype(f32)
    flows[..., 0] += ox                                                         # most samples land in the frame
    flows[..., 1] += oy
    flows[:, ::2] = np.round(flows[:, ::2] * 4) / 4                             # quarter pixels: ties among the samples
    flat = flows.reshape(-1)
    bad = rng.choice(flat.size, flat.size // 61, replace=False)
    flat[bad] = np.array([np.nan, np.inf, -np.inf, 3e38, -1e30], f32)[np.arange(bad.size) % 5]
    motions = rng.normal(0, 0.02, (n, K, 6))
    motions[..., [2, 5]] = rng.normal(0, 2.5, (n, K, 2))
    motions[0, 0] = 0
    occ = rng.choice(np.array([0] * 10 + [1, 2, 3, 200], np.uint8), (n, K, H, W))
    exclude = (rng.random((T, h, w)) < 0.08).astype(np.uint8)
    exclude[:, 4:9, 10:30] = 1                                                  # hidden in every frame
    ref = stack(rng, noc, u8, H, W, n)
    if not u8:
        ref = np.nan_to_num(ref)
    return frames, index, flows, motions, occ, exclude, ref


def gpu_plate(frames, index, canvas, **kw):
    from flowonthego_amd.plate import background_plate
    W, H, ox, oy = canvas
    a = {k: (dev(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    out = background_plate(dev(frames), index.tolist(), canvas=(W, H), origin=(ox, oy), count=True, code=True, stats=True, **a)
    torch.cuda.synchronize()
    return [host(o) for o in out]


def assert_equal_to_ref(got, want, what):
    for g, w_, nm in zip(got, want[:4], ("dst", "count", "code", "stats")):
        if nm == "stats":
            assert np.array_equal(g.view(np.uint64), w_.view(np.uint64)), (what, nm, g, w_)
        else:
            assert np_same_bits(g, w_), (what, nm)


@pytest.mark.parametrize("noc,u8", [(1, False), (1, True), (3, False), (3, True)])
@pytest.mark.parametrize("K", [1, 2, 3, 4, 5, 8, 9, 16, 31, 32])
def test_gpu_equals_the_restatement(K, noc, u8):
    frames, index, flows, motions, occ, exclude, ref = case(K, noc, u8, 100 * K + 10 * noc + u8)
    W, H, ox, oy = CANVAS
    seen = set()
    for mode in (0, 1):
        for min_count in sorted({1, K}):
            kw = dict(occ=occ, exclude=exclude, min_count=min_count, fill=7.25, ref=ref)
            for src in (dict(flows=flows), dict(motions=motions)):
                got = gpu_plate(frames, index, CANVAS, mode=("median", "mean")[mode], **kw, **src)
                sk = {("params" if k == "motions" else k): v for k, v in src.items()}
                want = R.plate(frames, index, W, H, ox, oy, mode=mode, **kw, **sk)
                assert_equal_to_ref(got, want, (mode, min_count, list(src)))
                seen |= set(np.unique(want[2]).tolist())
    assert seen == {0, 1, 2}
    # without masks and reference
    got = gpu_plate(frames, index, CANVAS, flows=flows)
    assert_equal_to_ref(got, R.plate(frames, index, W, H, ox, oy, flows=flows), "plain")
    assert got[3][0, 4] == 0 and got[3][0, 5] == 0


def test_every_launch_shape_gives_the_same_bits_one_past_the_tile():
    import flowonthego_amd as F
    L = F.lib()
    prev = L.fotg_plate_rows(0)
    assert prev in (1, 2, 4) and L.fotg_plate_rows(3) == prev and L.fotg_plate_rows(-1) == prev      # only a query
    try:
        for canvas, K, noc, u8 in (((65, 5, 2, 1), 9, 3, False), ((129, 9, -1, 0), 32, 3, False), (CANVAS, 5, 1, True)):
            frames, index, flows, motions, occ, exclude, ref = case(K, noc, u8, 7 + K, canvas)
            W, H, ox, oy = canvas
            want = R.plate(frames, index, W, H, ox, oy, flows=flows, occ=occ, exclude=exclude, ref=ref)
            for rows in (1, 2, 4):                                              # 4 rows, K = 32, three channels: 96 KB of LDS
                L.fotg_plate_rows(rows)
                assert L.fotg_plate_rows(0) == rows
                got = gpu_plate(frames, index, canvas, flows=flows, occ=occ, exclude=exclude, ref=ref)
                assert_equal_to_ref(got, want, (canvas, rows))
    finally:
        L.fotg_plate_rows(prev)


# ---- the routes agree -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,noc,u8", [(3, 1, True), (8, 3, False)])
def test_motion_source_equals_dense_on_motion_flow(K, noc, u8):
    from flowonthego_amd.motion import motion_flow
    from flowonthego_amd.plate import background_plate
    frames, index, _, motions, _, exclude, _ = case(K, noc, u8, 40 + K)
    h, w = FRAME
    mo, fr, ex = dev(motions), dev(frames), dev(exclude)
    flows = motion_flow(mo.view(-1, 6), w, h).view(2, K, h, w, 2)
    kw = dict(exclude=ex, min_count=min(2, K), count=True, code=True, stats=True)
    a = background_plate(fr, index.tolist(), motions=mo, **kw)
    b = background_plate(fr, index.tolist(), flows=flows, **kw)
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert same_bits(x, y)
    assert (a[2] == 0).any() and (a[2] == 2).any()


@pytest.mark.parametrize("K,noc,u8", [(1, 1, False), (4, 3, True), (9, 1, True)])
def test_fused_equals_dense_on_the_upsampled_flow(K, noc, u8):
    from flowonthego_amd.plate import background_plate
    n = 2
    for w, h in ((130, 40), (67, 37)):                        # 67 x 37: the pyramid pads to 68 x 40
        rng = np.random.default_rng(500 + K + w)
        o = make_ctx(2, w, h, max_batch=n * K, finest_scale=1, coarsest_scale=2, use_var_ref=False)
        wl, hl = o.out_size()
        cf = (rng.standard_normal((n * K, hl, wl, 2)) * 0.6).astype(f32)
        cf[0, 0, :3] = (np.nan, 0.0)
        cf[-1, hl // 2, :2] = (np.inf, 1.0)
        frames = dev(stack(rng, noc, u8, h, w))
        ref = dev(np.nan_to_num(stack(rng, noc, u8, h, w, n)))
        index = rng.integers(-1, T, (n, K)).tolist()
        occ = dev(rng.choice(np.array([0] * 12 + [1, 3], np.uint8), (n, K, h, w)))
        exclude = dev((rng.random((T, h, w)) < 0.1).astype(np.uint8))
        kw = dict(occ=occ, exclude=exclude, mode="median", min_count=1, fill=3, ref=ref, count=True, code=True, stats=True)
        got = o.upsample_crop_background_plate(dev(cf), frames, index, fused=True, **kw)
        unf = o.upsample_crop_background_plate(dev(cf), frames, index, fused=False, **kw)
        want = background_plate(frames, index, flows=o.upsample_crop(dev(cf)).view(n, K, h, w, 2), **kw)
        torch.cuda.synchronize()
        for g, u, w_, nm in zip(got, unf, want, ("dst", "count", "code", "stats")):
            assert same_bits(g, w_) and same_bits(u, w_), nm
        o.close()


# ---- properties -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 4, 32])
def test_copies_of_one_frame_with_zero_vectors_return_the_frame(K):
    from flowonthego_amd.plate import background_plate
    rng = np.random.default_rng(K)
    h, w = FRAME
    for noc, u8, mode in ((3, False, "median"), (1, True, "median"), (3, True, "mean")):
        frames = np.nan_to_num(stack(rng, noc, u8))
        z = torch.zeros((1, K, h, w, 2), device="cuda")
        dst, count = background_plate(dev(frames), [[2] * K], flows=z, mode=mode, count=True)
        assert np_same_bits(host(dst)[0], frames[2]) and (count == K).all()
        dst = background_plate(dev(frames), [[2] * K], motions=torch.zeros((K, 6), dtype=torch.float64, device="cuda"), mode=mode)
        assert np_same_bits(host(dst)[0], frames[2])


def test_one_sample_is_the_warp_at_its_valid_pixels():
    from flowonthego_amd.plate import background_plate
    from flowonthego_amd.warp import warp
    frames, _, flows, _, _, _, _ = case(1, 3, False, 3, (FRAME[1], FRAME[0], 0, 0))
    fl = dev(flows[0, 0])
    wd, wc, _ = warp(dev(frames[1]), fl, stats=True)
    dst, code = background_plate(dev(frames), [[1]], flows=fl[None, None], code=True)
    ok = wc == 0
    # what the warp calls valid and is no NaN is what the plate estimates
    sel = code[0] == 0
    assert torch.equal(sel, ok & ~torch.isnan(wd).any(-1)) and sel.sum() > 100 and (~ok).any() and (ok & ~sel).any()
    assert same_bits(dst[0][sel], wd[sel])


def test_permuting_the_samples_of_8_bit_frames_leaves_the_median_unchanged():
    K = 9
    frames, index, flows, motions, occ, exclude, ref = case(K, 3, True, 77)
    perm = np.random.default_rng(1).permutation(K)
    a = gpu_plate(frames, index, CANVAS, flows=flows, occ=occ, exclude=exclude, ref=ref)
    b = gpu_plate(frames, index[:, perm], CANVAS, flows=np.ascontiguousarray(flows[:, perm]), occ=np.ascontiguousarray(occ[:, perm]),
                  exclude=exclude, ref=ref)
    for x, y, nm in zip(a[:3], b[:3], ("dst", "count", "code")):
        assert np.array_equal(x, y), nm
    assert np.array_equal(a[3][:, :5], b[3][:, :5])                              # the first admitted sample is another


def _raw(K=3, n=2, noc=3):
    import flowonthego_amd as F
    h, w = 9, 11
    W, H = 13, 7
    s = dict(L=F.lib(), K=K, n=n, noc=noc, h=h, w=w, W=W, H=H)
    rng = np.random.default_rng(2)
    s["frames"] = dev(rng.uniform(0, 255, (T, h, w, noc)).astype(f32))
    s["flows"] = dev(rng.standard_normal((n, K, H, W, 2)).astype(f32))
    s["params"] = dev(rng.normal(0, 0.01, (n, K, 6)))
    s["occ"] = dev((rng.random((n, K, H, W)) < 0.2).astype(np.uint8))
    s["exclude"] = dev((rng.random((T, h, w)) < 0.2).astype(np.uint8))
    s["ref"] = dev(rng.uniform(0, 255, (n, H, W, noc)).astype(f32))
    s["index"] = [0, 1, -1, 5, 2, 3]
    s["dst"] = torch.full((n, H, W, noc), -7.0, device="cuda")
    s["count"] = torch.full((n, H, W), 99, dtype=torch.uint8, device="cuda")
    s["code"] = torch.full((n, H, W), 99, dtype=torch.uint8, device="cuda")
    s["stats"] = torch.full((n, 6), -7.0, dtype=torch.float64, device="cuda")
    return s


def _call(s, motion=False, **over):
    a = dict(s)
    a.update(over)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    ix = None if a["index"] is None else (C.c_int * len(a["index"]))(*a["index"])
    fn = s["L"].fotg_plate_motion if motion else s["L"].fotg_plate
    return fn(0, a["n"], a["K"], a.get("T", T), p(a["frames"]), a["w"], a["h"], a["noc"], ix, p(a["params"] if motion else a["flows"]),
              a["W"], a["H"], a.get("ox", 1), a.get("oy", -1), p(a["occ"]), p(a["exclude"]), a.get("mode", 0), a.get("min_count", 1),
              C.c_float(0.5), p(a["ref"]), p(a["dst"]), p(a["count"]), p(a["code"]), p(a["stats"]), None)


def test_each_output_alone():
    s = _raw()
    for motion in (False, True):
        assert _call(s, motion) == 0
        torch.cuda.synchronize()
        full = {k: s[k].clone() for k in ("dst", "count", "code", "stats")}
        assert (full["code"] < 3).all() and (full["stats"] >= 0).all()
        for keep in ("dst", "count", "code", "stats"):
            t = {k: torch.full_like(s[k], 99 if s[k].dtype == torch.uint8 else -7.0) for k in full}
            assert _call(s, motion, **{k: (t[k] if k == keep else None) for k in full}) == 0
            torch.cuda.synchronize()
            assert same_bits(t[keep], full[keep]), (motion, keep)


def test_arguments_are_refused_and_nothing_is_launched():
    import flowonthego_amd as F
    s = _raw()
    bad = [dict(n=0), dict(n=-1), dict(n=65536), dict(K=0), dict(K=33), dict(T=0), dict(w=0), dict(h=-1), dict(w=16385), dict(W=0), dict(H=0),
           dict(W=16385), dict(H=16385), dict(ox=(1 << 20) + 1), dict(oy=-(1 << 20) - 1), dict(noc=2), dict(noc=0), dict(mode=2), dict(mode=-1),
           dict(min_count=0), dict(min_count=4), dict(index=[0, 1, -2, 5, 2, 3]), dict(index=[0, 1, -1, 6, 2, 3]), dict(frames=None),
           dict(flows=None, params=None), dict(index=None), dict(dst=None, count=None, code=None, stats=None),
           dict(dst=s["frames"]), dict(dst=s["ref"]), dict(count=s["occ"]), dict(code=s["exclude"]), dict(code=s["count"]),
           dict(stats=s["ref"].view(-1).view(torch.float64))]
    for motion in (False, True):
        for b in bad:
            assert _call(s, motion, **b) == FOTG_ERR_ARG, (motion, b)
    assert _call(s, dst=s["flows"]) == FOTG_ERR_ARG and _call(s, True, dst=s["params"].view(torch.float32)) == FOTG_ERR_ARG
    torch.cuda.synchronize()
    assert (s["dst"] == -7.0).all() and (s["count"] == 99).all() and (s["code"] == 99).all() and (s["stats"] == -7.0).all()
    assert _call(s) == 0 and _call(s, True) == 0
    # the fused form
    L = s["L"]
    o = make_ctx(2, 64, 48, max_batch=4)
    wl, hl = o.out_size()
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    cf = torch.zeros((4, hl, wl, 2), device="cuda")
    fr = torch.zeros((3, 48, 64), device="cuda")
    out = torch.full((2, 48, 64), -7.0, device="cuda")
    ints = lambda v: None if v is None else (C.c_int * len(v))(*v)
    fused = lambda ctx=o._h, n=2, K=2, f=cf, s_=fr, ch=1, ix=(0, 2, 1, -1), d=out, mc=1: L.fotg_upsample_crop_plate(
        ctx, n, K, 3, p(f), p(s_), ch, ints(ix), None, None, 0, mc, C.c_float(0.0), None, p(d), None, None, None, None)
    for b in (dict(ctx=None), dict(n=3), dict(K=3), dict(n=0), dict(f=None), dict(s_=None), dict(ch=4), dict(ix=(0, 3, 1, 1)), dict(ix=None),
              dict(d=None), dict(d=fr), dict(mc=3)):
        assert fused(**b) == FOTG_ERR_ARG, b
    torch.cuda.synchronize()
    assert (out == -7.0).all()
    assert fused() == 0
    op = F.operating_point(2, 64, 1)
    op.depth_mode = True
    from flowonthego_amd.oflow import OFClass
    od = OFClass(op, F.img_params(width=64, height=48), max_batch=4)
    assert fused(ctx=od._h) == FOTG_ERR_ARG
    with pytest.raises(F.FotgError):
        od.background(fr)
    # the binding's own refusals
    from flowonthego_amd.plate import background_plate
    z = torch.zeros((1, 3, 48, 64, 2), device="cuda")
    for kw in (dict(), dict(flows=z, motions=torch.zeros((3, 6), dtype=torch.float64, device="cuda")), dict(flows=z, mode="mode"),
               dict(flows=z, min_count=4), dict(flows=z, index=[[0, 1, 3]]), dict(flows=z, canvas=(64, 47)), dict(flows=z.cpu()),
               dict(motions=torch.zeros((3, 6), device="cuda")), dict(flows=z, exclude=torch.zeros((3, 48, 64), device="cuda")),
               dict(flows=z, origin=5)):
        with pytest.raises(F.FotgError):
            background_plate(fr, **kw)
    torch.cuda.synchronize()


# ---- OFClass.background -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bidir", [False, True])
def test_ofclass_background_is_the_documented_composition(bidir, natural_images):
    import flowonthego_amd as F
    frames_np, _ = M.jittered_crops(natural_images["road_HD"], T=4, patch=True)
    frames = dev(frames_np)
    K, h, w = frames_np.shape
    o = make_ctx(2, w, h, max_batch=K - 1, bidir=bidir)
    for mosaic, ref, model in ((False, 0, "affine"), (True, 2, "similarity")):
        plate, code, count = o.background(frames, ref=ref, model=model, mosaic=mosaic, min_count=2)
        if bidir:
            fw, bw = o.calc_sequence_bidirectional(frames)
            mask = o.upsample_crop_fb_check(fw, bw)[0]
        else:
            fw, mask = o.calc_sequence(frames), None
        params, moving = F.upsample_crop_fit_motion(o, fw, mask, model, code=True)
        exclude = torch.zeros((K, h, w), dtype=torch.uint8, device="cuda")
        exclude[:K - 1] = (moving == 1).to(torch.uint8)
        motions = F.plate_motions(params, ref)
        W, H, ox, oy = F.mosaic_canvas(motions, w, h) if mosaic else (w, h, 0, 0)
        d, n, c = F.background_plate(frames, None, motions=motions, canvas=(W, H), origin=(ox, oy), exclude=exclude, min_count=2, count=True,
                                     code=True)
        torch.cuda.synchronize()
        assert same_bits(plate, d[0]) and same_bits(count, n[0]) and same_bits(code, c[0])
        assert plate.shape == (H, W) and (W >= w and H >= h) and (code == 0).float().mean().item() > 0.5
        if mosaic:
            assert (W, H) != (w, h)
        keep = o.background(frames, ref=ref, model=model, mosaic=mosaic, exclude_moving=False, mode="mean")
        d = F.background_plate(frames, None, motions=motions, canvas=(W, H), origin=(ox, oy), mode="mean", count=True, code=True)
        assert same_bits(keep[0], d[0][0]) and same_bits(keep[2], d[1][0])
    with pytest.raises(F.FotgError):
        o.background(frames[:1])
    with pytest.raises(F.FotgError):
        o.background(frames, ref=K)
    o.close()


def test_median_plate_beats_the_mean_and_the_unaligned_median(natural_images):
    """the scene and the selection of tests/test_plate.py's CPU form of this test: 640 x 384 crops of the jittered-crops walk
    (at 320 x 192 the flows of this scene are too poor to align it), the code-0 pixels the patch covers in fewer than half of the
    coverage"""
    import flowonthego_amd as F
    frames_np, motions, (_, _, ox, oy), truth, foot = R.crops_scene(natural_images["road_HD"], T=8, w=R.BIG_W, h=R.BIG_H)
    K, h, w = frames_np.shape
    frames = dev(frames_np)
    o = make_ctx(2, w, h, max_batch=K - 1)
    med = o.background(frames)
    mean = o.background(frames, mode="mean")
    ident = F.background_plate(frames, None, motions=torch.zeros((K, 6), dtype=torch.float64, device="cuda"), code=True)
    torch.cuda.synchronize()
    grid = (w, h, 0, 0)
    hit, cover = R.stamp(foot, motions, grid), R.stamp(np.ones_like(foot), motions, grid)
    sel = (host(med[1]) == 0) & (host(mean[1]) == 0) & (host(ident[1])[0] == 0) & (2 * hit < cover)
    T0 = truth[oy:oy + h, ox:ox + w].astype(np.float64)
    e = [float(np.abs(host(d).astype(np.float64) - T0)[sel].mean()) for d in (med[0], mean[0], ident[0][0])]
    mse = float(((host(med[0]).astype(np.float64) - T0)[sel] ** 2).mean())
    print("mean absolute error over %d pixels: median %.4f, mean %.4f, median with identity motions %.4f; PSNR of the median plate %.2f dB"
          % (sel.sum(), e[0], e[1], e[2], 10 * np.log10(255.0 ** 2 / mse)))
    assert sel.sum() > 0.8 * h * w
    assert e[0] < e[1] and e[0] < e[2]
    o.close()
