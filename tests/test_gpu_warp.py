"""GPU tests of the frame warp (fotg_warp / fotg_upsample_crop_warp and their 8-bit forms, flowonthego_amd.warp).

The dense form equals the numpy restatement (tests/warp_ref.py, itself pinned to the reference's image_warp by tests/test_warp.py)
byte for byte in dst, code and the four counts; the fused form equals the dense form of fotg_upsample_crop's output bit for bit,
the two residual sums included.  The residual sums are bounded against math.fsum of the restatement's terms by N 2^-53 fsum: the
bound of ANY order of adding N non-negative doubles (each addition errs by at most 2^-53 of its result, which never exceeds the
exact total times (1 + 2^-53)^k), so it is derived, not measured."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import warp_ref as W

pytestmark = pytest.mark.gpu

FOTG_ERR_ARG = 1
f32 = np.float32


def _F():
    import flowonthego_amd as F
    from flowonthego_amd.oflow import OFClass
    return F, OFClass


def dev(a, dtype=None):
    a = np.asarray(a)
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype or a.dtype)).cuda()


def make_ctx(op_point, w, h, channels=1, max_batch=1, bidir=False, **kw):
    F, OFClass = _F()
    op = F.operating_point(op_point, w, channels)
    op.bidir = bidir
    for k, v in kw.items():
        setattr(op, k, v)
    return OFClass(op, F.img_params(width=w, height=h), max_batch=max_batch)


def bits(t):
    t = t.contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int64) if t.dtype == torch.float64 else t


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def np_same_bits(a, b):
    if a.dtype == np.float32:
        return a.shape == b.shape and b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


def check_sums(got, tw, tu):
    """|gpu - fsum(terms)| <= N 2^-53 fsum(terms), printed before asserted"""
    for g, t, nm in ((got[4], tw, "warped"), (got[5], tu, "unwarped")):
        want = math.fsum(t)
        bound = len(t) * 2.0 ** -53 * want
        print("residual sum %s: gpu %.17g fsum %.17g |d| %.3g bound %.3g (N = %d)" % (nm, g, want, abs(g - want), bound, len(t)))
        assert abs(g - want) <= bound, nm


def image(rng, shape, u8):
    a = rng.integers(0, 256, shape)
    return a.astype(np.uint8) if u8 else (a + rng.random(shape) * (a < 255)).astype(f32)


def odd_flow(rng, n, h, w, scale=4.0):
    """smooth-ish random vectors with non-finite and huge entries, and targets exactly on the borders"""
    fl = (rng.standard_normal((n, h, w, 2)) * scale).astype(f32)
    vals = np.array([np.nan, np.inf, -np.inf, 2e9, -2e9, 1e30, -1e30, 3e38, -0.0], f32)
    flat = fl.reshape(-1)
    idx = rng.choice(flat.size, min(36, flat.size // 3), replace=False)
    flat[idx] = vals[np.arange(idx.size) % vals.size]
    ys, xs = np.mgrid[0:h, 0:w]
    fl[0, ::3, :, 0] = (f32(w - 1) - xs[::3]).astype(f32)
    fl[-1, :, ::2, 1] = -ys[:, ::2].astype(f32)
    return fl


def assert_dense_matches(src, flow, ref=None, occ=None, fill=None, sums=True):
    """the batch through the GPU against the restatement image by image: dst, code, counts byte for byte, sums within the bound"""
    from flowonthego_amd.warp import warp
    t = lambda a: None if a is None else dev(a)
    dst, code, st = warp(t(src), t(flow), ref=t(ref), occ=t(occ), fill=fill, stats=True)
    only = warp(t(src), t(flow), occ=t(occ), fill=fill)
    torch.cuda.synchronize()
    assert same_bits(only, dst)
    dst, code, st = dst.cpu().numpy(), code.cpu().numpy(), st.cpu().numpy()
    for k in range(len(src)):
        wd, wc, ws, tw, tu = W.warp(src[k], flow[k], None if ref is None else ref[k], None if occ is None else occ[k],
                                    0 if fill is None else 1, 0.0 if fill is None else fill, terms=True)
        assert np_same_bits(dst[k], wd), (k, np.argwhere(dst[k] != wd)[:5])
        assert np.array_equal(code[k], wc), (k, np.argwhere(code[k] != wc)[:5])
        assert np.array_equal(st[k, :4], ws[:4]), (k, st[k], ws)
        if ref is None:
            assert st[k, 4] == 0 and st[k, 5] == 0
        elif sums:
            check_sums(st[k], tw, tu)
    return dst, code, st


# ---- 4. the dense form ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noc", [1, 3])
@pytest.mark.parametrize("u8", [False, True])
def test_dense_small_sizes_every_mode(noc, u8):
    rng = np.random.default_rng(31 + noc + 10 * u8)
    for n, h, w in ((3, 101, 157), (3, 23, 41), (3, 1, 7), (3, 7, 1), (2, 436, 1024)):
        shape = (n, h, w) if noc == 1 else (n, h, w, 3)
        src, ref = image(rng, shape, u8), image(rng, shape, u8)
        flow = odd_flow(rng, n, h, w)
        occ = rng.choice(np.array([0, 0, 0, 1, 3], np.uint8), (n, h, w))
        for fill in (None, 17.5, -3.0):
            for with_occ in (False, True):
                for with_ref in (False, True):
                    if (h, w) == (436, 1024) and (fill == -3.0 or with_occ != with_ref):
                        continue
                    dst, code, st = assert_dense_matches(src, flow, ref if with_ref else None, occ if with_occ else None, fill)
        # a batch equals its images alone (unaligned bases inside the batch: w h % 4 != 0)
        from flowonthego_amd.warp import warp
        db, cb, sb = warp(dev(src), dev(flow), ref=dev(ref), occ=dev(occ), fill=5.0, stats=True)
        for k in range(n):
            d1, c1, s1 = warp(dev(src[k]), dev(flow[k]), ref=dev(ref[k]), occ=dev(occ[k]), fill=5.0, stats=True)
            assert same_bits(d1, db[k]) and torch.equal(c1, cb[k]) and same_bits(s1, sb[k]), k


@pytest.mark.parametrize("noc,u8", [(1, False), (3, True), (1, True), (3, False)])
def test_dense_1080p(noc, u8, natural_images):
    road = natural_images["road_HD"]
    h, w = road.shape
    rng = np.random.default_rng(50 + noc)
    g0, g1 = road, np.roll(road, (2, -5), axis=(0, 1))
    if noc == 3:
        g0, g1 = (np.stack([g, np.roll(g, 1, 1), 255 - g], -1) for g in (g0, g1))
    src, ref = (g[None].astype(np.uint8 if u8 else f32) for g in (g1, g0))
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    flow = np.stack([-5 + 2 * np.sin(ys / 90), 2 + 3 * np.cos(xs / 120)], -1)[None].astype(f32)
    flow[0, 5, 7] = (np.nan, 1)
    flow[0, 500, 900] = (1e30, -2e9)
    occ = rng.choice(np.array([0, 0, 0, 1], np.uint8), (1, h, w))
    assert_dense_matches(src, flow, ref, None, None)
    assert_dense_matches(src, flow, ref, occ, 0.0)


def test_dense_reference_cases():
    """the flows of the reference comparison (tests/test_warp.py): in reference mode the GPU IS image_warp"""
    for name, noc, h, w, kind, seed in W.cases():
        img, flow = W.case_image(h, w, noc, seed), W.case_flow(kind, h, w, seed)
        assert_dense_matches(img[None], flow[None], img[None][:, ::-1].copy(), None, None)


def test_arguments_are_refused():
    F, _ = _F()
    L = F.lib()
    n, h, w = 2, 9, 11
    src = torch.zeros((n, h, w), device="cuda")
    flow = torch.zeros((n, h, w, 2), device="cuda")
    dst = torch.empty_like(src)
    code = torch.empty((n, h, w), dtype=torch.uint8, device="cuda")
    st = torch.empty((n, 6), dtype=torch.float64, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    call = lambda n_=n, s=src, f=flow, w_=w, h_=h, ch=1, fm=0, d=dst, c=code, t=st: L.fotg_warp(
        0, n_, p(s), p(f), w_, h_, ch, None, None, fm, C.c_float(0), p(d), p(c), p(t), None)
    assert call() == 0
    assert call(d=None, c=None) == 0 and call(d=None, t=None) == 0          # any one output is enough
    torch.cuda.synchronize()
    for bad in (dict(n_=0), dict(n_=-1), dict(s=None), dict(f=None), dict(w_=0), dict(h_=-2), dict(ch=2), dict(ch=0), dict(fm=2),
                dict(fm=-1), dict(d=None, c=None, t=None), dict(d=src)):
        assert call(**bad) == FOTG_ERR_ARG, bad
    assert L.fotg_warp_u8(0, n, None, p(flow), w, h, 1, None, None, 0, C.c_float(0), p(code), None, None, None) == FOTG_ERR_ARG
    o = make_ctx(2, 64, 48)
    wl, hl = o.out_size()
    cf = torch.zeros((1, hl, wl, 2), device="cuda")
    img = torch.zeros((1, 48, 64), device="cuda")
    out = torch.empty_like(img)
    fused = lambda ctx=o._h, n_=1, f=cf, s=img, ch=1, d=out: L.fotg_upsample_crop_warp(
        ctx, n_, p(f), p(s), ch, None, None, 0, C.c_float(0), p(d), None, None, None)
    assert fused() == 0
    for bad in (dict(ctx=None), dict(n_=2), dict(n_=0), dict(f=None), dict(s=None), dict(ch=4), dict(d=None), dict(d=img)):
        assert fused(**bad) == FOTG_ERR_ARG, bad
    op = F.operating_point(2, 64, 1)
    op.depth_mode = True
    from flowonthego_amd.oflow import OFClass
    od = OFClass(op, F.img_params(width=64, height=48))
    assert fused(ctx=od._h) == FOTG_ERR_ARG
    with pytest.raises(F.FotgError):
        od.upsample_crop_warp(cf, img)
    torch.cuda.synchronize()


# ---- 5. the fused form ------------------------------------------------------------------------------------------------------------
def assert_fused_matches(o, cf, src, ref=None, occ=None, fill=None):
    got = o.upsample_crop_warp(cf, src, ref=ref, occ=occ, fill=fill, stats=True, fused=True)
    want = o.upsample_crop_warp(cf, src, ref=ref, occ=occ, fill=fill, stats=True, fused=False)
    torch.cuda.synchronize()
    for g, w_, nm in zip(got, want, ("dst", "code", "stats")):
        assert same_bits(g, w_), nm
    return got


@pytest.mark.parametrize("op_point", [1, 2, 3, 4])
def test_fused_operating_points_1080p(op_point, natural_images):
    road = natural_images["road_HD"]
    o = make_ctx(op_point, road.shape[1], road.shape[0])
    I0, I1 = dev(road[None], f32), dev(np.roll(road, (3, -5), axis=(0, 1))[None], f32)
    cf = o.calc_batch(I0, I1)
    dst, code, st = assert_fused_matches(o, cf, I1, ref=I0)
    assert st[0, :4].sum().item() == road.size and (code == 0).any() and st[0, 4].item() > 0
    occ = (torch.rand(code.shape, device="cuda") < 0.1).to(torch.uint8)
    assert_fused_matches(o, cf, I1, ref=I0, occ=occ, fill=0.0)
    assert_fused_matches(o, cf, I1.to(torch.uint8), ref=I0.to(torch.uint8), occ=occ, fill=255.0)


@pytest.mark.parametrize("sc_l", [0, 1, 2, 3])
def test_fused_finest_scales_on_odd_sizes(sc_l):
    rng = np.random.default_rng(70 + sc_l)
    for w, h in ((641, 479), (97, 61)):
        o = make_ctx(2, w, h, max_batch=3, finest_scale=sc_l, coarsest_scale=max(sc_l, 4), use_var_ref=False)
        wl, hl = o.out_size()
        cf = rng.standard_normal((3, hl, wl, 2)).astype(f32) * (6.0 / (1 << sc_l))
        cf[0, 0, :4] = (np.nan, 0.0)
        cf[1, hl // 2, :3] = (np.inf, 1.0)
        for noc, u8 in ((1, False), (3, False), (1, True), (3, True)):
            shape = (3, h, w) if noc == 1 else (3, h, w, 3)
            src, ref = dev(image(rng, shape, u8)), dev(image(rng, shape, u8))
            occ = dev(rng.choice(np.array([0, 0, 1, 3], np.uint8), (3, h, w)))
            assert_fused_matches(o, dev(cf), src, ref=ref)
            assert_fused_matches(o, dev(cf), src, ref=ref, occ=occ, fill=1.0)


def test_fused_engine_flows_alley_and_batch_of_64(alley, natural_images):
    f0, f1 = alley["frame_0001"].astype(f32), alley["frame_0002"].astype(f32)
    o = make_ctx(2, f0.shape[1], f0.shape[0])
    I0, I1 = dev(f0[None]), dev(f1[None])
    assert_fused_matches(o, o.calc_batch(I0, I1), I1, ref=I0)
    road = natural_images["road_HD"]
    n = 64
    o = make_ctx(2, road.shape[1], road.shape[0], max_batch=n)
    I0 = dev(np.stack([np.roll(road, 5 * k, axis=1) for k in range(n)]))
    I1 = dev(np.stack([np.roll(road, (k % 5 - 2, 5 * k + k % 7 - 3), axis=(0, 1)) for k in range(n)]))
    cf = o.calc_batch_u8(I0, I1)
    dst, code, st = assert_fused_matches(o, cf, I1, ref=I0)
    assert (st[:, :4].sum(dim=1) == road.size).all()
    assert_fused_matches(o, cf, I1.to(torch.float32), ref=I0.to(torch.float32), fill=0.0)


def test_fused_dst_beyond_2_pow_31_bytes():
    """96 synthetic coarse flows on a 4K context: dst is 96 x 3840 x 2160 x 4 = 3.2e9 bytes, so the batch offsets of the later
    images pass 2^31 (and 2^32); compared with the unfused warp chunk by chunk"""
    from flowonthego_amd.warp import warp
    n, W_, H = 96, 3840, 2160
    o = make_ctx(4, W_, H, max_batch=n, use_var_ref=False)
    wl, hl = o.out_size()
    g = torch.Generator(device="cuda").manual_seed(6)
    cf = torch.randn((n, hl, wl, 2), device="cuda", generator=g) * 2.0
    cf[n - 1, hl // 2, :8] = float("nan")
    base = torch.rand((8, H, W_), device="cuda", generator=g) * 255
    src = base.repeat(n // 8, 1, 1)
    src[n - 1] += 1.0
    dst, code, st = o.upsample_crop_warp(cf, src, ref=src, stats=True, fused=True)
    assert dst.numel() * 4 > 2 ** 31
    k = 12
    for s in range(0, n, k):
        ud, uc, us = warp(src[s:s + k], o.upsample_crop(cf[s:s + k].contiguous()), ref=src[s:s + k], stats=True)
        assert same_bits(dst[s:s + k], ud) and torch.equal(code[s:s + k], uc) and same_bits(st[s:s + k], us), s
    assert (st[n - 1, 3] > 0).item()
    del dst, code, src
    torch.cuda.synchronize()


# ---- 6. the residual sums are the same bits every time ----------------------------------------------------------------------------
def test_sums_repeat_bit_for_bit_also_beside_a_running_flow_batch(natural_images):
    from flowonthego_amd.warp import warp
    road = natural_images["road_HD"]
    n = 8
    o = make_ctx(2, road.shape[1], road.shape[0], max_batch=n)
    I0 = dev(np.stack([np.roll(road, 5 * k, axis=1) for k in range(n)]), f32)
    I1 = dev(np.stack([np.roll(road, (k % 3 - 1, 5 * k + 2), axis=(0, 1)) for k in range(n)]), f32)
    flow = o.upsample_crop(o.calc_batch(I0, I1))
    a = warp(I1, flow, ref=I0, stats=True)
    b = warp(I1, flow, ref=I0, stats=True)
    torch.cuda.synchronize()
    assert same_bits(a[2], b[2]) and same_bits(a[0], b[0])
    side = torch.cuda.Stream()
    o.calc_batch(I0, I1, outflow=o.new_outflow(n))            # a flow batch in flight on the current stream
    with torch.cuda.stream(side):
        c = warp(I1, flow, ref=I0, stats=True)
    torch.cuda.synchronize()
    assert same_bits(a[2], c[2]) and same_bits(a[0], c[0]) and torch.equal(a[1], c[1])
    # and they are the sums: image 0 against the restatement's terms
    _, _, _, tw, tu = W.warp(I1[0].cpu().numpy(), flow[0].cpu().numpy(), I0[0].cpu().numpy(), terms=True)
    check_sums(a[2][0].cpu().numpy(), tw, tu)


# ---- 7. the consistency mask as occ -----------------------------------------------------------------------------------------------
def test_fb_check_masks_as_occ(alley):
    from flowonthego_amd.consistency import fb_check
    from flowonthego_amd.warp import warp
    f0, f1 = alley["frame_0001"].astype(f32), alley["frame_0002"].astype(f32)
    o = make_ctx(2, f0.shape[1], f0.shape[0], bidir=True)
    I0, I1 = dev(f0[None]), dev(f1[None])
    cfw, cbw = o.calc_bidirectional(I0, I1)
    fw, bw = o.upsample_crop(cfw), o.upsample_crop(cbw)
    mask, mask_bw, cnt = fb_check(fw, bw, stats=True)
    for src, ref, flow, m, d in ((I1, I0, fw, mask, 0), (I0, I1, bw, mask_bw, 1)):
        _, own, _ = warp(src, flow, stats=True)
        dst, code, st = warp(src, flow, ref=ref, occ=m, fill=0.0, stats=True)
        torch.cuda.synchronize()
        assert torch.equal(code[own == 0], m[own == 0]) and torch.equal(code, m)     # code 2 / 3 are the same expressions
        assert np.array_equal(st[0, :4].cpu().numpy(), cnt[0, d].cpu().numpy().astype(np.float64))
        assert (dst[code != 0] == 0).all()


# ---- 8. it does what it is for ----------------------------------------------------------------------------------------------------
def test_warping_along_the_engine_flow_halves_the_residual(alley):
    from conftest import synth_pair
    pairs = ((alley["frame_0001"].astype(f32), alley["frame_0002"].astype(f32)), synth_pair(272, 480, seed=5))
    for f0, f1 in pairs:
        h, w = f0.shape
        o = make_ctx(2, w, h)
        I0, I1 = dev(f0[None]), dev(f1[None])
        dst, code, st = o.upsample_crop_warp(o.calc_batch(I0, I1), I1, ref=I0, stats=True)
        st = st[0].cpu().numpy()
        print("%d x %d: valid %.4f, mean |I0 - warp(I1)| %.3f, mean |I0 - I1| %.3f, ratio %.3f"
              % (h, w, st[0] / (h * w), st[4] / st[0], st[5] / st[0], st[4] / st[5]))
        assert st[0] > 0.95 * h * w
        assert st[4] < 0.5 * st[5]
