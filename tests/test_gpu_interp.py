"""GPU tests of the frame interpolation (fotg_interp / fotg_upsample_crop_interp and their 8-bit forms, flowonthego_amd.interp).

The dense form equals the numpy restatement (tests/interp_ref.py, pinned by tests/test_interp.py) byte for byte in dst, code and
the four counts; the fused form equals the dense form of fotg_upsample_crop's outputs and fotg_fb_check's masks bit for bit, the
residual sums included.  The residual sums are bounded against math.fsum of the restatement's terms by N 2^-53 fsum: the bound of
ANY order of adding N non-negative doubles (tests/test_gpu_warp.py derives it), so it is derived, not measured.

test_heavy_collisions_* is the test that fails for a wrong collision rule: with the atomicMin of interp_candidate_kernel replaced
by a plain store (last writer wins) the random +- 2 w flows give other winners and the byte comparison fails."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import fbcheck_ref as FB
import interp_ref as I
import warp_ref as W
from test_gpu_warp import bits, dev, image, make_ctx, np_same_bits, odd_flow, same_bits

pytestmark = pytest.mark.gpu

FOTG_ERR_ARG, FOTG_ERR_UNSUPPORTED = 1, 4
f32 = np.float32
TIMES = (0.5, 0.25, 0.3, 0.9375)


def check_sums(got, tv, tb):
    """|gpu - fsum(terms)| <= N 2^-53 fsum(terms), printed before asserted"""
    for g, t, nm in ((got[4], tv, "interpolated"), (got[5], tb, "blend")):
        want = math.fsum(t)
        bound = len(t) * 2.0 ** -53 * want
        print("residual sum %s: gpu %.17g fsum %.17g |d| %.3g bound %.3g (N = %d)" % (nm, g, want, abs(g - want), bound, len(t)))
        assert abs(g - want) <= bound, nm


def masks(rng, shape):
    """masks in fb_check's alphabet with a byte above it: every code occurs"""
    return rng.choice(np.array([0, 0, 0, 0, 1, 1, 2, 3, 200], np.uint8), shape)


def assert_dense_matches(I0, I1, F, B, t, mF=None, mB=None, ref=None):
    """the batch through the GPU against the restatement image by image: dst, code, counts byte for byte, sums within the bound"""
    from flowonthego_amd.interp import interpolate
    d = lambda a: None if a is None else dev(a)
    dst, code, st = interpolate(d(I0), d(I1), d(F), d(B), t, mask_fw=d(mF), mask_bw=d(mB), ref=d(ref), stats=True)
    only = interpolate(d(I0), d(I1), d(F), d(B), t, mask_fw=d(mF), mask_bw=d(mB))
    torch.cuda.synchronize()
    assert same_bits(only, dst)
    dst, code, st = dst.cpu().numpy(), code.cpu().numpy(), st.cpu().numpy()
    for k in range(len(I0)):
        wd, wc, ws, tv, tb = I.interp(I0[k], I1[k], F[k], B[k], t, None if mF is None else mF[k], None if mB is None else mB[k],
                                      None if ref is None else ref[k], terms=True)
        assert np.array_equal(code[k], wc), (k, t, np.argwhere(code[k] != wc)[:5])
        assert np_same_bits(dst[k], wd), (k, t, np.argwhere(dst[k] != wd)[:5])
        assert np.array_equal(st[k, :4], ws[:4]), (k, st[k], ws)
        assert st[k, :3].sum() == code[k].size
        if ref is None:
            assert st[k, 4] == 0 and st[k, 5] == 0
        else:
            check_sums(st[k], tv, tb)
    return dst, code, st


# ---- the dense form against the restatement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("noc", [1, 3])
@pytest.mark.parametrize("u8", [False, True])
def test_dense_small_sizes_every_mode(noc, u8):
    rng = np.random.default_rng(131 + noc + 10 * u8)
    for n, h, w in ((3, 101, 157), (3, 23, 41), (2, 1, 7), (2, 7, 1), (2, 5, 3)):
        shape = (n, h, w) if noc == 1 else (n, h, w, 3)
        I0, I1, ref = image(rng, shape, u8), image(rng, shape, u8), image(rng, shape, u8)
        F, B = odd_flow(rng, n, h, w), odd_flow(rng, n, h, w, scale=2.0)
        mF, mB = masks(rng, (n, h, w)), masks(rng, (n, h, w))
        for t in TIMES:
            assert_dense_matches(I0, I1, F, B, t, mF, mB, ref)
        assert_dense_matches(I0, I1, F, B, 0.5)                       # the call's own consistency check
        assert_dense_matches(I0, I1, F, B, 0.3, ref=ref)


@pytest.mark.parametrize("kind", W.KINDS)
def test_heavy_collisions_and_the_reference_flows(kind):
    """warp_ref.case_flow's kinds, `random` (up to +- 2 w) with every vector allowed to project: thousands of candidates per
    target, most of the frame holes.  The winners are the minimum keys: any other rule fails here."""
    for si, (h, w) in enumerate(W.SIZES):
        for noc in (1, 3):
            seed = 500 + 10 * si + noc
            I0, I1 = W.case_image(h, w, noc, seed), W.case_image(h, w, noc, seed + 1)
            F, B = W.case_flow(kind, h, w, seed), W.case_flow(kind, h, w, seed + 1)
            if kind == "random":                      # keep the targets inside: many sources per target
                F, B = (F * f32(0.25)), (B * f32(0.25))
            rng = np.random.default_rng(seed)
            m = rng.integers(0, 2, (2, h, w)).astype(np.uint8)
            for t in (0.5, 0.75):
                dst, code, st = assert_dense_matches(I0[None], I1[None], F[None], B[None], t, m[:1], m[1:], I0[None])
            if kind in ("random", "integer") and h * w > 100:
                _, _, _, KF, KB = I.interp(I0, I1, F, B, 0.5, m[0], m[1], planes=True)
                print("%s %dx%d: holes %.3f" % (kind, h, w, st[0, 2] / (h * w)))
    # the collisions of one big case: every target of a constant-target flow gets w h / 4 candidates
    h, w = 64, 96
    ys, xs = np.mgrid[0:h, 0:w]
    F = np.stack([(xs % 2 + 10 - xs) * 2.0, (ys % 2 + 7 - ys) * 2.0], -1).astype(f32)     # t = 0.5: everything lands on 2 x 2 pixels
    B = -F[::-1, ::-1].copy()
    rng = np.random.default_rng(9)
    I0, I1 = rng.integers(0, 256, (h, w)).astype(f32), rng.integers(0, 256, (h, w)).astype(f32)
    m = rng.integers(0, 2, (2, h, w)).astype(np.uint8)
    dst, code, st = assert_dense_matches(I0[None], I1[None], F[None], B[None], 0.5, m[:1], m[1:])
    assert st[0, 0] == 4 and st[0, 2] > 0


def test_batch_of_64_equals_its_images_alone():
    from flowonthego_amd.interp import interpolate
    rng = np.random.default_rng(64)
    n, h, w = 64, 45, 67                               # w h % 4 != 0: unaligned image bases inside the batch
    I0, I1, ref = image(rng, (n, h, w), True), image(rng, (n, h, w), True), image(rng, (n, h, w), True)
    F, B = odd_flow(rng, n, h, w, scale=6.0), odd_flow(rng, n, h, w, scale=6.0)
    dst, code, st = assert_dense_matches(I0, I1, F, B, 0.5, ref=ref)
    for k in (0, 1, 37, 63):
        d1, c1, s1 = interpolate(dev(I0[k]), dev(I1[k]), dev(F[k]), dev(B[k]), 0.5, ref=dev(ref[k]), stats=True)
        assert np.array_equal(d1.cpu().numpy(), dst[k]) and np.array_equal(c1.cpu().numpy(), code[k])
        assert np.array_equal(s1.cpu().numpy().view(np.int64), st[k].view(np.int64))


def test_a_sequence_of_t_returns_a_stack():
    from flowonthego_amd.interp import interpolate
    rng = np.random.default_rng(5)
    h, w = 33, 47
    I0, I1 = dev(image(rng, (h, w, 3), True)), dev(image(rng, (h, w, 3), True))
    F, B = dev(odd_flow(rng, 1, h, w)[0]), dev(odd_flow(rng, 1, h, w)[0])
    stack = interpolate(I0, I1, F, B, [0.25, 0.5, 0.75])
    assert tuple(stack.shape) == (3, h, w, 3)
    for i, t in enumerate((0.25, 0.5, 0.75)):
        assert torch.equal(stack[i], interpolate(I0, I1, F, B, t))
    d, c, s = interpolate(I0[None], I1[None], F[None], B[None], (0.5, 0.9), stats=True)
    assert tuple(d.shape) == (2, 1, h, w, 3) and tuple(c.shape) == (2, 1, h, w) and tuple(s.shape) == (2, 1, 6)
    torch.cuda.synchronize()


def test_dense_1080p_and_chunks(natural_images):
    """ten 1080p images: more than the eight whose key planes one chunk holds"""
    from flowonthego_amd.interp import interpolate
    road = natural_images["road_HD"]
    h, w = road.shape
    n = 10
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    F1 = np.stack([-5 + 2 * np.sin(ys / 90), 2 + 3 * np.cos(xs / 120)], -1).astype(f32)
    F1[5, 7] = (np.nan, 1)
    F1[500, 900] = (1e30, -2e9)
    I0 = dev(np.stack([np.roll(road, 3 * k, axis=1) for k in range(n)]))
    I1 = dev(np.stack([np.roll(road, (2, 3 * k - 5), axis=(0, 1)) for k in range(n)]))
    F = dev(np.stack([F1 * f32(1 + 0.1 * k) for k in range(n)]))
    B = dev(np.stack([-F1 * f32(1 + 0.1 * k) for k in range(n)]))
    dst, code, st = interpolate(I0, I1, F, B, 0.5, ref=I0, stats=True)
    torch.cuda.synchronize()
    for k in (0, 7, 8, 9):
        wd, wc, ws, tv, tb = I.interp(I0[k].cpu().numpy(), I1[k].cpu().numpy(), F[k].cpu().numpy(), B[k].cpu().numpy(), 0.5,
                                      ref=I0[k].cpu().numpy(), terms=True)
        assert np.array_equal(code[k].cpu().numpy(), wc) and np.array_equal(dst[k].cpu().numpy(), wd), k
        assert np.array_equal(st[k, :4].cpu().numpy(), ws[:4])
        check_sums(st[k].cpu().numpy(), tv, tb)


# ---- the sums repeat ---------------------------------------------------------------------------------------------------------------
def test_sums_repeat_bit_for_bit_on_two_runs_and_two_streams(natural_images):
    from flowonthego_amd.interp import interpolate
    road = natural_images["road_HD"]
    n = 4
    rng = np.random.default_rng(77)
    I0 = dev(np.stack([np.roll(road, 5 * k, axis=1) for k in range(n)]), f32)
    I1 = dev(np.stack([np.roll(road, (k % 3 - 1, 5 * k + 2), axis=(0, 1)) for k in range(n)]), f32)
    F = dev((rng.standard_normal((n,) + road.shape + (2,)) * 3).astype(f32))
    B = dev((rng.standard_normal((n,) + road.shape + (2,)) * 3).astype(f32))
    a = interpolate(I0, I1, F, B, 0.5, ref=I1, stats=True)
    b = interpolate(I0, I1, F, B, 0.5, ref=I1, stats=True)
    torch.cuda.synchronize()
    assert same_bits(a[2], b[2]) and same_bits(a[0], b[0]) and torch.equal(a[1], b[1])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = interpolate(I0, I1, F, B, 0.5, ref=I1, stats=True)
    torch.cuda.synchronize()
    assert same_bits(a[2], c[2]) and same_bits(a[0], c[0]) and torch.equal(a[1], c[1])
    assert (a[2][:, 4] > 0).all()


# ---- the fused form ----------------------------------------------------------------------------------------------------------------
def assert_fused_matches(o, cfw, cbw, I0, I1, t, ref=None, own_masks=True):
    """fused == the dense form on fotg_upsample_crop's outputs and fotg_fb_check's masks, through separate calls"""
    from flowonthego_amd.consistency import fb_check
    from flowonthego_amd.interp import interpolate
    got = o.upsample_crop_interpolate(cfw, cbw, I0, I1, t, ref=ref, stats=True, fused=True)
    fw, bw = o.upsample_crop(cfw), o.upsample_crop(cbw)
    m, mb = fb_check(fw, bw)
    want = interpolate(I0, I1, fw, bw, t, mask_fw=m, mask_bw=mb, ref=ref, stats=True)
    unf = o.upsample_crop_interpolate(cfw, cbw, I0, I1, t, ref=ref, stats=True, fused=False)
    given = o.upsample_crop_interpolate(cfw, cbw, I0, I1, t, mask_fw=m, mask_bw=mb, ref=ref, stats=True, fused=True)
    torch.cuda.synchronize()
    for g, w_, u, gv, nm in zip(got, want, unf, given, ("dst", "code", "stats")):
        assert same_bits(g, w_) and same_bits(u, w_) and same_bits(gv, w_), nm
    return got


@pytest.mark.parametrize("op_point", [1, 2, 3, 4])
def test_fused_operating_points_1080p(op_point, natural_images):
    road = natural_images["road_HD"]
    o = make_ctx(op_point, road.shape[1], road.shape[0], bidir=True)
    I0, I1 = dev(road[None], f32), dev(np.roll(road, (3, -5), axis=(0, 1))[None], f32)
    cfw, cbw = o.calc_bidirectional(I0, I1)
    dst, code, st = assert_fused_matches(o, cfw, cbw, I0, I1, 0.5, ref=I0)
    assert st[0, :3].sum().item() == road.size and st[0, 0].item() > 0.9 * road.size
    assert_fused_matches(o, cfw, cbw, I0.to(torch.uint8), I1.to(torch.uint8), 0.25, ref=I1.to(torch.uint8))


@pytest.mark.parametrize("sc_l", [0, 1, 2, 3])
def test_fused_finest_scales_on_odd_sizes(sc_l):
    rng = np.random.default_rng(170 + sc_l)
    for w, h in ((641, 479), (97, 61)):
        o = make_ctx(2, w, h, max_batch=3, bidir=True, finest_scale=sc_l, coarsest_scale=max(sc_l, 4), use_var_ref=False)
        wl, hl = o.out_size()
        cfw = rng.standard_normal((3, hl, wl, 2)).astype(f32) * (6.0 / (1 << sc_l))
        cbw = -cfw + rng.standard_normal((3, hl, wl, 2)).astype(f32) * (0.3 / (1 << sc_l))
        cfw[0, 0, :4] = (np.nan, 0.0)
        cbw[1, hl // 2, :3] = (np.inf, 1.0)
        for noc, u8 in ((1, False), (3, False), (1, True), (3, True)):
            shape = (3, h, w) if noc == 1 else (3, h, w, 3)
            I0, I1, ref = dev(image(rng, shape, u8)), dev(image(rng, shape, u8)), dev(image(rng, shape, u8))
            assert_fused_matches(o, dev(cfw), dev(cbw), I0, I1, 0.5, ref=ref)
            assert_fused_matches(o, dev(cfw), dev(cbw), I0, I1, 0.3)


def test_unsupported_and_refused_arguments():
    import flowonthego_amd as F
    L = F.lib()
    n, h, w = 2, 9, 11
    I0, I1 = torch.zeros((n, h, w), device="cuda"), torch.ones((n, h, w), device="cuda")
    fw, bw = torch.zeros((n, h, w, 2), device="cuda"), torch.zeros((n, h, w, 2), device="cuda")
    m = torch.zeros((n, h, w), dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(I0)
    code = torch.empty((n, h, w), dtype=torch.uint8, device="cuda")
    st = torch.empty((n, 6), dtype=torch.float64, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    call = lambda n_=n, a=I0, b=I1, f=fw, g=bw, w_=w, h_=h, ch=1, t=0.5, mf=m, mb=m, d=dst, c=code, s=st: L.fotg_interp(
        0, n_, p(a), p(b), p(f), p(g), w_, h_, ch, C.c_float(t), p(mf), p(mb), C.c_float(0.01), C.c_float(0.5), None, p(d), p(c), p(s), None)
    assert call() == 0 and call(mf=None, mb=None) == 0
    assert call(d=None, c=None) == 0 and call(d=None, s=None) == 0
    torch.cuda.synchronize()
    for bad in (dict(n_=0), dict(n_=-1), dict(a=None), dict(b=None), dict(f=None), dict(g=None), dict(w_=0), dict(h_=-2), dict(ch=2),
                dict(t=0.0), dict(t=1.0), dict(t=-0.5), dict(t=1.5), dict(t=float("nan")), dict(mf=None), dict(mb=None),
                dict(d=None, c=None, s=None), dict(d=I0), dict(d=I1)):
        assert call(**bad) == FOTG_ERR_ARG, bad
    assert L.fotg_interp_u8(0, n, None, p(m), p(fw), p(bw), w, h, 1, C.c_float(0.5), None, None, C.c_float(0.01), C.c_float(0.5),
                            None, p(code), None, None, None) == FOTG_ERR_ARG
    img0, img1 = torch.zeros((1, 48, 64), device="cuda"), torch.zeros((1, 48, 64), device="cuda")
    out = torch.empty_like(img0)

    def fused(o, n_=1, t=0.5, d=out, f=True):
        wl, hl = o.out_size()
        cf = torch.zeros((1, hl, wl, 2), device="cuda")
        return L.fotg_upsample_crop_interp(o._h, n_, p(cf) if f else None, p(cf), p(img0), p(img1), 1, C.c_float(t), None, None,
                                           C.c_float(0.01), C.c_float(0.5), None, p(d), None, None, None)
    plain, bi = make_ctx(2, 64, 48), make_ctx(2, 64, 48, bidir=True)
    assert fused(plain) == FOTG_ERR_UNSUPPORTED
    assert fused(bi) == 0
    for bad in (dict(n_=2), dict(n_=0), dict(t=1.0), dict(d=None), dict(d=img0), dict(f=False)):
        assert fused(bi, **bad) == FOTG_ERR_ARG, bad
    assert L.fotg_upsample_crop_interp(None, 1, p(out), p(out), p(img0), p(img1), 1, C.c_float(0.5), None, None, C.c_float(0.01),
                                       C.c_float(0.5), None, p(out), None, None, None) == FOTG_ERR_ARG
    with pytest.raises(F.FotgError):
        plain.interpolate(img0, img1, 0.5)
    with pytest.raises(F.FotgError):
        bi.interpolate(img0, img1, 1.0)
    torch.cuda.synchronize()


# ---- it does what it is for --------------------------------------------------------------------------------------------------------
def test_interpolating_the_alley_triplets_beats_the_plain_blend(alley):
    """OFClass.interpolate on (1, 2, 3) and (20, 21, 22) at t = 0.5 meets tests/test_interp.py's conditions (the thresholds are
    imported from there), with the engine's own flows; and those flows are the oracle's, so the frame is the restatement's."""
    import os
    from conftest import GOLDEN
    from test_interp import HOLE_SHARE_MAX, QUALITY
    more = np.load(os.path.join(GOLDEN, "alley_1_more.npz"))
    fr = {1: alley["frame_0001"], 2: alley["frame_0002"], 3: more["frame_0003"], 20: more["frame_0020"], 21: more["frame_0021"],
          22: more["frame_0022"]}
    for (i, m, j), (blend_db, interp_db) in QUALITY.items():
        f0, fm, f1 = (fr[k].astype(f32) for k in (i, m, j))
        h, w = f0.shape
        o = make_ctx(2, w, h, bidir=True)
        dst, code, st = o.interpolate(dev(f0), dev(f1), 0.5, ref=dev(fm), stats=True)
        torch.cuda.synchronize()
        st = st.cpu().numpy()
        got, blend = I.psnr(dst.cpu().numpy(), fm), I.psnr(f32(0.5) * f0 + f32(0.5) * f1, fm)
        print("(%d, %d, %d): blend %.3f dB, interpolated %.3f dB, holes %.4f, mean |ref - dst| %.3f, mean |ref - blend| %.3f"
              % (i, m, j, blend, got, st[2] / (h * w), st[4] / (h * w), st[5] / (h * w)))
        assert abs(blend - blend_db) < 1e-3
        assert got >= blend + 0.5 * (interp_db - blend_db)
        assert st[2] <= HOLE_SHARE_MAX * h * w
        if (i, m, j) == (1, 2, 3):
            from oracle import oracle as O
            F, B = O.full_flow(f0, f1), O.full_flow(f1, f0)
            cfw, cbw = o.bidirectional_flows(dev(f0[None]), dev(f1[None]))
            assert np.array_equal(o.upsample_crop(cfw)[0].cpu().numpy(), F) and np.array_equal(o.upsample_crop(cbw)[0].cpu().numpy(), B)
            wd, wc, ws = I.interp(f0, f1, F, B, 0.5, ref=fm)
            assert np_same_bits(dst.cpu().numpy(), wd) and np.array_equal(code.cpu().numpy(), wc) and np.array_equal(st[:4], ws[:4])
        o.close()
