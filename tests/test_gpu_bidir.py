"""GPU tests of bidirectional flow (fotg_calc_bidir / fotg_calc_sequence_bidir, OFClass.calc_bidirectional) and the
forward-backward consistency check (fotg_fb_check / fotg_upsample_crop_fb_check, flowonthego_amd.consistency).

The bidirectional contract: the forward flow equals fotg_calc_batch(I0, I1, initflow) and the backward one
fotg_calc_batch(I1, I0, initflow_bw), bit for bit.  The dense check equals the numpy restatement (tests/fbcheck_ref.py) byte for
byte; the fused check equals the dense check of fotg_upsample_crop's outputs byte for byte."""
import ctypes as C

import numpy as np
import pytest
import torch

import fbcheck_ref as R

pytestmark = pytest.mark.gpu

FOTG_ERR_ARG, FOTG_ERR_BATCH, FOTG_ERR_UNSUPPORTED = 1, 3, 4


def _F():
    import flowonthego_amd as F
    from flowonthego_amd.oflow import OFClass
    return F, OFClass


def dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def make_ctx(op_point, w, h, channels=1, max_batch=1, bidir=True, **kw):
    F, OFClass = _F()
    op = F.operating_point(op_point, w, channels)
    op.bidir = bidir
    for k, v in kw.items():
        setattr(op, k, v)
    return OFClass(op, F.img_params(width=w, height=h), max_batch=max_batch)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def check_contract(o, I0, I1, u8=False, initflow=None, initflow_bw=None):
    """bidir == the two one-direction calls on the same context, bit for bit; returns (fw, bw)"""
    one = o.calc_batch_u8 if u8 else o.calc_batch
    both = o.calc_bidirectional_u8 if u8 else o.calc_bidirectional
    fw, bw = both(I0, I1, initflow, initflow_bw)
    want_fw, want_bw = one(I0, I1, initflow), one(I1, I0, initflow_bw)
    torch.cuda.synchronize()
    assert same_bits(fw, want_fw), (fw - want_fw).abs().max().item()
    assert same_bits(bw, want_bw), (bw - want_bw).abs().max().item()
    assert torch.isfinite(fw).all() and torch.isfinite(bw).all()
    return fw, bw


def batch(f0, f1, n, step=3):
    """n pairs: the frames shifted sideways by step px per pair (different content per pair)"""
    I0 = np.stack([np.roll(f0, step * k, axis=1) for k in range(n)])
    I1 = np.stack([np.roll(f1, step * k, axis=1) for k in range(n)])
    return I0, I1


def init_field(o, n, seed):
    sc = o.op.coarsest_scale + 1
    rng = np.random.default_rng(seed)
    return dev(rng.uniform(-1.5, 1.5, (n, o.height >> sc, o.width >> sc, 2)))


# ---- the bidirectional contract ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op_point", [1, 2, 3, 4])
def test_bidir_contract_operating_points(op_point, alley, natural_images):
    f0, f1 = alley["frame_0001"].astype(np.float32), alley["frame_0002"].astype(np.float32)
    o = make_ctx(op_point, f0.shape[1], f0.shape[0])
    check_contract(o, dev(f0[None]), dev(f1[None]))
    road = natural_images["road_HD"].astype(np.float32)
    o = make_ctx(op_point, road.shape[1], road.shape[0])
    check_contract(o, dev(road[None]), dev(np.roll(road, (2, -5), axis=(0, 1))[None]))


@pytest.mark.parametrize("variant", ["rgb", "u8", "u8_color", "fast_math", "sor1", "sor2", "no_refinement", "usefbcon"])
def test_bidir_contract_modes(variant, alley):
    f0, f1 = alley["frame_0001"], alley["frame_0002"]
    h, w = f0.shape
    if variant == "rgb":
        c0, c1 = alley["rgb_crop_0001"].astype(np.float32), alley["rgb_crop_0002"].astype(np.float32)
        o = make_ctx(2, c0.shape[1], c0.shape[0], channels=3)
        check_contract(o, dev(c0[None]), dev(c1[None]))
    elif variant == "u8":
        o = make_ctx(2, w, h)
        check_contract(o, dev(f0[None], np.uint8), dev(f1[None], np.uint8), u8=True)
    elif variant == "u8_color":
        c0, c1 = alley["rgb_crop_0001"], alley["rgb_crop_0002"]
        o = make_ctx(2, c0.shape[1], c0.shape[0], u8_color=1)
        check_contract(o, dev(c0[None], np.uint8), dev(c1[None], np.uint8), u8=True)
    else:
        kw = {"fast_math": {"fast_math": True}, "sor1": {"sor_mode": 1}, "sor2": {"sor_mode": 2},
              "no_refinement": {"use_var_ref": False}, "usefbcon": {"use_fbcon": True}}[variant]
        o = make_ctx(2, w, h, **kw)
        check_contract(o, dev(f0[None].astype(np.float32)), dev(f1[None].astype(np.float32)))


def test_bidir_contract_batches_odd_sizes_and_initflow(alley):
    f0, f1 = alley["frame_0001"].astype(np.float32), alley["frame_0002"].astype(np.float32)
    h, w = f0.shape
    o = make_ctx(2, w, h, max_batch=8)
    for n in (1, 7, 8):
        I0, I1 = batch(f0, f1, n)
        check_contract(o, dev(I0), dev(I1))
    I0, I1 = batch(f0, f1, 3)
    check_contract(o, dev(I0), dev(I1), initflow=init_field(o, 3, 1), initflow_bw=init_field(o, 3, 2))
    check_contract(o, dev(I0), dev(I1), initflow_bw=init_field(o, 3, 3))
    for hh, ww in ((17, 33), (479, 641)):
        a0 = np.ascontiguousarray(np.tile(f0, (2, 1))[:hh, :ww])
        a1 = np.ascontiguousarray(np.tile(f1, (2, 1))[:hh, :ww])
        o = make_ctx(2, ww, hh, max_batch=2)
        I0, I1 = batch(a0, a1, 2)
        check_contract(o, dev(I0), dev(I1), initflow=init_field(o, 2, 4), initflow_bw=init_field(o, 2, 5))


def test_bidir_sequence(alley):
    f0, f1 = alley["frame_0001"], alley["frame_0002"]
    h, w = f0.shape
    frames = np.stack([np.roll(f0 if k % 2 == 0 else f1, 2 * k, axis=1) for k in range(9)])
    o = make_ctx(2, w, h, max_batch=8)
    for dt in (np.float32, np.uint8):
        fr = dev(frames, dt)
        fw, bw = o.calc_sequence_bidirectional(fr)
        one = o.calc_batch_u8 if dt == np.uint8 else o.calc_batch
        want_fw, want_bw = one(fr[:-1].contiguous(), fr[1:].contiguous()), one(fr[1:].contiguous(), fr[:-1].contiguous())
        torch.cuda.synchronize()
        assert same_bits(fw, want_fw) and same_bits(bw, want_bw), dt
    ifw, ibw = init_field(o, 8, 6), init_field(o, 8, 7)
    fr = dev(frames)
    fw, bw = o.calc_sequence_bidirectional(fr, ifw, ibw)
    assert same_bits(fw, o.calc_batch(fr[:-1].contiguous(), fr[1:].contiguous(), ifw))
    assert same_bits(bw, o.calc_batch(fr[1:].contiguous(), fr[:-1].contiguous(), ibw))


def test_bidir_4k_operating_point_4_and_a_second_call(natural_images):
    y = natural_images["yosemite_4k"].astype(np.float32)
    o = make_ctx(4, y.shape[1], y.shape[0])
    I0, I1 = dev(y[None]), dev(np.roll(y, (3, -4), axis=(0, 1))[None])
    check_contract(o, I0, I1)
    # a second call on the same context, other content: nothing of the first call's state leaks into it
    check_contract(o, I1, dev(np.roll(y, (-2, 5), axis=(0, 1))[None]))


def test_bidir_refusals(alley):
    F, _ = _F()
    L = F.lib()
    f0 = alley["frame_0001"].astype(np.float32)
    h, w = f0.shape
    I = dev(f0[None])
    plain = make_ctx(2, w, h, bidir=False, max_batch=2)
    out, out_bw = plain.new_outflow(2), plain.new_outflow(2)
    p = lambda t: C.c_void_p(t.data_ptr())
    assert L.fotg_calc_bidir(plain._h, 1, p(I), p(I), None, None, p(out), p(out_bw), None) == FOTG_ERR_ARG
    assert L.fotg_calc_sequence_bidir(plain._h, 2, p(I), None, None, p(out), p(out_bw), None) == FOTG_ERR_ARG
    with pytest.raises(F.FotgError):
        plain.calc_bidirectional(I, I)
    # depth mode has no bidirectional form
    op = F.operating_point(2, w, 1)
    op.bidir, op.depth_mode = True, True
    h_ = C.c_void_p()
    assert L.fotg_create(op.to_c(), w, h, 0, 1, h_) == FOTG_ERR_UNSUPPORTED
    o = make_ctx(2, w, h, max_batch=2)
    args = lambda n, a, b, o1, o2, i1=None, i2=None: (o._h, n, a, b, i1, i2, o1, o2, None)
    assert L.fotg_calc_bidir(*args(1, None, p(I), p(out), p(out_bw))) == FOTG_ERR_ARG
    assert L.fotg_calc_bidir(*args(1, p(I), None, p(out), p(out_bw))) == FOTG_ERR_ARG
    assert L.fotg_calc_bidir(*args(1, p(I), p(I), None, p(out_bw))) == FOTG_ERR_ARG
    assert L.fotg_calc_bidir(*args(1, p(I), p(I), p(out), None)) == FOTG_ERR_ARG
    assert L.fotg_calc_bidir(None, 1, p(I), p(I), None, None, p(out), p(out_bw), None) == FOTG_ERR_ARG
    for n in (0, -1, 3):
        assert L.fotg_calc_bidir(*args(n, p(I), p(I), p(out), p(out_bw))) == FOTG_ERR_BATCH
        assert L.fotg_calc_bidir_u8(*args(n, p(I), p(I), p(out), p(out_bw))) == FOTG_ERR_BATCH
    assert L.fotg_calc_sequence_bidir(o._h, 1, p(I), None, None, p(out), p(out_bw), None) == FOTG_ERR_BATCH
    assert L.fotg_calc_sequence_bidir(o._h, 4, p(I), None, None, p(out), p(out_bw), None) == FOTG_ERR_BATCH
    assert L.fotg_calc_sequence_bidir_u8(o._h, 2, None, None, None, p(out), p(out_bw), None) == FOTG_ERR_ARG
    # usefbcon couples the directions: only without initflows
    fb = make_ctx(2, w, h, use_fbcon=True)
    init = init_field(fb, 1, 1)
    assert L.fotg_calc_bidir(fb._h, 1, p(I), p(I), p(init), None, p(out), p(out_bw), None) == FOTG_ERR_ARG
    assert L.fotg_calc_bidir(fb._h, 1, p(I), p(I), None, p(init), p(out), p(out_bw), None) == FOTG_ERR_ARG
    torch.cuda.synchronize()


# ---- the consistency check -----------------------------------------------------------------------------------------------------
def gpu_check(fw, bw, a1=0.01, a2=0.5):
    from flowonthego_amd.consistency import fb_check
    m, mb, cnt = fb_check(dev(fw), dev(bw), a1, a2, stats=True)
    return m.cpu().numpy(), mb.cpu().numpy(), cnt.cpu().numpy()


def assert_dense_matches(fw, bw, a1=0.01, a2=0.5):
    m, mb, cnt = gpu_check(fw, bw, a1, a2)
    want, want_bw = R.fb_check(fw, bw, a1, a2)
    assert np.array_equal(m, want), np.argwhere(m != want)[:5]
    assert np.array_equal(mb, want_bw), np.argwhere(mb != want_bw)[:5]
    assert np.array_equal(cnt.reshape(-1, 2, 4), R.counts(want, want_bw))


def engine_flows(o, f0, f1):
    fw, bw = o.calc_bidirectional(dev(f0[None]), dev(f1[None]))
    return o.upsample_crop(fw), o.upsample_crop(bw), fw, bw


def test_dense_check_on_engine_flows(alley, natural_images):
    f0, f1 = alley["frame_0001"].astype(np.float32), alley["frame_0002"].astype(np.float32)
    road = natural_images["road_HD"].astype(np.float32)
    yos = natural_images["yosemite_4k"].astype(np.float32)
    for op_point, a, b in ((2, f0, f1), (2, road, np.roll(road, (4, -6), axis=(0, 1))), (4, yos, np.roll(yos, (-3, 7), axis=(0, 1)))):
        o = make_ctx(op_point, a.shape[1], a.shape[0])
        ufw, ubw, _, _ = engine_flows(o, a, b)
        fw, bw = ufw.cpu().numpy()[0], ubw.cpu().numpy()[0]
        assert_dense_matches(fw, bw)
        m, _, _ = gpu_check(fw, bw)
        assert (m == 0).mean() > 0.5 and (m == 1).any() and (m == 2).any()      # a real mix of codes


def test_dense_check_synthetic_edge_values():
    rng = np.random.default_rng(11)
    for n, h, w in ((3, 37, 53), (2, 1, 1), (1, 2, 3), (1, 64, 64)):
        fw = (rng.standard_normal((n, h, w, 2)) * 4).astype(np.float32)
        bw = (-fw + rng.standard_normal((n, h, w, 2)).astype(np.float32) * 0.5).astype(np.float32)
        vals = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 3e38, 0.0, -0.0], np.float32)
        for f in (fw, bw):
            flat = f.reshape(-1)
            idx = rng.choice(flat.size, min(24, flat.size), replace=False)
            flat[idx] = vals[np.arange(idx.size) % vals.size]
        # targets exactly on the last column / row and on 0
        ys, xs = np.mgrid[0:h, 0:w]
        fw[0, ::3, :, 0] = (np.float32(w - 1) - xs[::3]).astype(np.float32)
        fw[0, 1::3, :, 1] = (np.float32(h - 1) - ys[1::3]).astype(np.float32)
        fw[-1, :, ::2, 0] = -xs[:, ::2].astype(np.float32)
        for a1, a2 in ((0.01, 0.5), (0.0, 1.0), (0.05, 0.0)):
            assert_dense_matches(fw, bw, a1, a2)


def test_dense_check_null_masks_and_arguments():
    F, _ = _F()
    L = F.lib()
    rng = np.random.default_rng(3)
    n, h, w = 2, 45, 31
    fw, bw = dev(rng.standard_normal((n, h, w, 2)) * 3), dev(rng.standard_normal((n, h, w, 2)) * 3)
    want, want_bw = R.fb_check(fw.cpu().numpy(), bw.cpu().numpy())
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for with_m, with_mb in ((True, False), (False, True), (False, False)):
        m = torch.full((n, h, w), 7, dtype=torch.uint8, device="cuda") if with_m else None
        mb = torch.full((n, h, w), 7, dtype=torch.uint8, device="cuda") if with_mb else None
        cnt = torch.full((n, 2, 4), -1, dtype=torch.int32, device="cuda")
        assert L.fotg_fb_check(0, n, p(fw), p(bw), w, h, C.c_float(0.01), C.c_float(0.5), p(m), p(mb), p(cnt), s) == 0
        torch.cuda.synchronize()
        if with_m:
            assert np.array_equal(m.cpu().numpy(), want)
        if with_mb:
            assert np.array_equal(mb.cpu().numpy(), want_bw)
        assert np.array_equal(cnt.cpu().numpy(), R.counts(want, want_bw))
    m = torch.empty((n, h, w), dtype=torch.uint8, device="cuda")
    assert L.fotg_fb_check(0, n, p(fw), p(bw), w, h, C.c_float(0.01), C.c_float(0.5), p(m), None, None, s) == 0
    torch.cuda.synchronize()
    assert np.array_equal(m.cpu().numpy(), want)
    a = (C.c_float(0.01), C.c_float(0.5), p(m), None, None, s)
    assert L.fotg_fb_check(0, 0, p(fw), p(bw), w, h, *a) == FOTG_ERR_ARG
    assert L.fotg_fb_check(0, n, None, p(bw), w, h, *a) == FOTG_ERR_ARG
    assert L.fotg_fb_check(0, n, p(fw), None, w, h, *a) == FOTG_ERR_ARG
    assert L.fotg_fb_check(0, n, p(fw), p(bw), 0, h, *a) == FOTG_ERR_ARG
    assert L.fotg_fb_check(0, n, p(fw), p(bw), w, -1, *a) == FOTG_ERR_ARG
    o = make_ctx(2, 64, 48)
    assert L.fotg_upsample_crop_fb_check(o._h, 2, p(fw), p(bw), *a) == FOTG_ERR_ARG          # n > max_batch
    assert L.fotg_upsample_crop_fb_check(o._h, 1, None, p(bw), *a) == FOTG_ERR_ARG
    assert L.fotg_upsample_crop_fb_check(None, 1, p(fw), p(bw), *a) == FOTG_ERR_ARG


def assert_fused_matches(o, fw, bw, a1=0.01, a2=0.5):
    from flowonthego_amd.consistency import upsample_crop_fb_check
    m, mb, cnt = upsample_crop_fb_check(o, fw, bw, a1, a2, stats=True, fused=True)
    um, umb, ucnt = upsample_crop_fb_check(o, fw, bw, a1, a2, stats=True, fused=False)
    torch.cuda.synchronize()
    assert torch.equal(m, um) and torch.equal(mb, umb) and torch.equal(cnt, ucnt)
    # the C-ABI's fused entry point directly, one mask at a time and no counts
    F, _ = _F()
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for want, first in ((um, True), (umb, False)):
        got = torch.full_like(want, 9)
        assert F.lib().fotg_upsample_crop_fb_check(o._h, fw.shape[0], p(fw), p(bw), C.c_float(a1), C.c_float(a2),
                                                   p(got) if first else None, None if first else p(got), None, s) == 0
        torch.cuda.synchronize()
        assert torch.equal(got, want), first
    return m, mb, cnt


@pytest.mark.parametrize("op_point", [1, 2, 3, 4])
def test_fused_check_operating_points_1080p(op_point, natural_images):
    road = natural_images["road_HD"].astype(np.float32)
    o = make_ctx(op_point, road.shape[1], road.shape[0])
    _, _, fw, bw = engine_flows(o, road, np.roll(road, (3, -5), axis=(0, 1)))
    m, mb, cnt = assert_fused_matches(o, fw, bw)
    assert int(cnt.sum()) == 2 * road.size and (m == 0).any() and (mb == 0).any()


@pytest.mark.parametrize("sc_l", [0, 1, 2, 3])
def test_fused_check_finest_scales_on_odd_sizes(sc_l):
    rng = np.random.default_rng(20 + sc_l)
    for w, h in ((641, 479), (97, 61)):
        o = make_ctx(2, w, h, max_batch=3, finest_scale=sc_l, coarsest_scale=max(sc_l, 4), use_var_ref=False)
        wl, hl = o.out_size()
        fw = rng.standard_normal((3, hl, wl, 2)).astype(np.float32) * (6.0 / (1 << sc_l))
        bw = (-fw + rng.standard_normal((3, hl, wl, 2)).astype(np.float32) * 0.2).astype(np.float32)
        fw[0, 0, :4] = (np.nan, 0.0)
        bw[1, hl // 2, :3] = (np.inf, 1.0)
        assert_fused_matches(o, dev(fw), dev(bw))
        assert_fused_matches(o, dev(fw), dev(bw), 0.0, 2.0)


def test_fused_check_batch_of_64_engine_flows(natural_images):
    road = natural_images["road_HD"]
    n = 64
    o = make_ctx(2, road.shape[1], road.shape[0], max_batch=n)
    I0 = np.stack([np.roll(road, 5 * k, axis=1) for k in range(n)])
    I1 = np.stack([np.roll(road, (k % 5 - 2, 5 * k + k % 7 - 3), axis=(0, 1)) for k in range(n)])
    fw, bw = o.calc_bidirectional_u8(dev(I0, np.uint8), dev(I1, np.uint8))
    _, _, cnt = assert_fused_matches(o, fw, bw)
    assert (cnt.sum(dim=2) == road.size).all()


def test_fused_check_mask_beyond_2_pow_31_bytes():
    """260 synthetic coarse flow pairs on a 4K context: each mask is 260 x 3840 x 2160 = 2.16e9 bytes, so the batch offsets of
    the last pairs pass 2^31; compared with the unfused check chunk by chunk"""
    from flowonthego_amd.consistency import fb_check, upsample_crop_fb_check
    n, W, H = 260, 3840, 2160
    o = make_ctx(4, W, H, max_batch=n, use_var_ref=False)
    wl, hl = o.out_size()
    g = torch.Generator(device="cuda").manual_seed(5)
    fw = torch.randn((n, hl, wl, 2), device="cuda", generator=g) * 2.0
    bw = -fw + torch.randn((n, hl, wl, 2), device="cuda", generator=g) * 0.3
    fw[n - 1, hl // 2, wl - 8:] = float("nan")           # (the last coarse rows only feed the cropped padding)
    m, mb, cnt = upsample_crop_fb_check(o, fw, bw, stats=True, fused=True)
    assert m.numel() > 2 ** 31
    k = 20
    for s in range(0, n, k):
        e = min(n, s + k)
        um, umb, ucnt = fb_check(o.upsample_crop(fw[s:e].contiguous()), o.upsample_crop(bw[s:e].contiguous()), stats=True)
        assert torch.equal(m[s:e], um) and torch.equal(mb[s:e], umb) and torch.equal(cnt[s:e], ucnt), s
    assert (cnt[n - 1, 0, 3] > 0).item()
    del m, mb
    torch.cuda.synchronize()
