"""GPU tests of the motion-compensated temporal filter (fotg_temporal_filter / fotg_upsample_crop_temporal_filter and their 8-bit
forms, flowonthego_amd.temporal, OFClass.temporal_filter).

The dense form equals the numpy restatement (tests/temporal_ref.py, on top of warp_ref.warp) byte for byte in dst, used and the two
counts; the fused form equals the dense form of fotg_upsample_crop's output bit for bit, the two residual sums included.  The
residual sums are bounded against math.fsum of the restatement's terms by N 2^-53 fsum, the bound of any order of adding N
non-negative doubles (tests/test_gpu_warp.py derives it).

The sizes are the smallest at which the kernel's paths differ (its tile is 64 x 16, its store width four pixels): 1 x 1 (every window
position clamped), 3 x 5 (smaller than a tile, a halo clamped on all four sides), 19 x 67 and 40 x 130 (tile borders crossed in both
directions, a width that is no multiple of four)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import temporal_ref as R
from test_gpu_warp import dev, make_ctx, np_same_bits, odd_flow, same_bits

pytestmark = pytest.mark.gpu

FOTG_ERR_ARG = 1
f32 = np.float32
SIZES = ((1, 1), (3, 5), (19, 67), (40, 130))          # (h, w)
T, CENTER = 5, [0, 2, 4]
# per centre K slots: absent neighbours at the ends of the sequence, frames shared by several centres, every slot of the middle
# centre filled (so used can reach K), and centre 4 its own neighbour in slot 0
ROWS = ([-1, 1, -1, 2, -1, 3, -1, 4], [1, 3, 0, 4, 2, 1, 3, 0], [4, 3, -1, 2, -1, 1, -1, 0])
GAINS = [1.0, 0.5, 2.0, 0.75, 1.25, 3.0, 0.125, 1.5]


def neighbors(K):
    return [row[:K] for row in ROWS]


def stack(rng, h, w, noc, u8):
    """T frames of one smooth scene with independent noise (sigma 3): a small flow changes a frame little, so the window's mean
    difference lies between the two values of tau the tests use"""
    ys, xs = np.mgrid[0:h, 0:w]
    base = 128 + 60 * np.sin(ys / 9.0) + 50 * np.cos(xs / 7.0)
    if noc == 3:
        base = np.stack([base, 255 - base, base[::-1]], -1)
    fr = np.clip(base[None] + rng.normal(0, 3, (T,) + base.shape), 0, 255)
    return np.rint(fr).astype(np.uint8) if u8 else fr.astype(f32)


def case(h, w, K, noc, u8, seed):
    rng = np.random.default_rng(seed)
    n = len(CENTER)
    frames = stack(rng, h, w, noc, u8)
    ref = stack(rng, h, w, noc, u8)[:n]
    flows = odd_flow(rng, n * K, h, w, scale=0.4).reshape(n, K, h, w, 2)
    masks = rng.choice(np.array([0] * 12 + [1, 2, 3, 7], np.uint8), (n, K, h, w))
    return frames, ref, flows, masks


def check_sums(got, tv, tc):
    """|gpu - fsum(terms)| <= N 2^-53 fsum(terms), printed before asserted"""
    for g, t, nm in ((got[2], tv, "filtered"), (got[3], tc, "centre")):
        want = math.fsum(t)
        bound = len(t) * 2.0 ** -53 * want
        print("residual sum %s: gpu %.17g fsum %.17g |d| %.3g bound %.3g (N = %d)" % (nm, g, want, abs(g - want), bound, len(t)))
        assert abs(g - want) <= bound, nm


def assert_dense_matches(frames, K, flows, masks, tau, gains, ref):
    """the batch through the GPU against the restatement image by image; returns the restatement's used"""
    from flowonthego_amd.temporal import temporal_filter
    t = lambda a: None if a is None else dev(a)
    nbr = neighbors(K)
    args = (t(frames), CENTER, nbr, t(flows))
    kw = dict(masks=t(masks), tau=tau, gains=gains, ref=t(ref))
    dst, used, st = temporal_filter(*args, stats=True, **kw)
    again = temporal_filter(*args, stats=True, **kw)
    only = temporal_filter(*args, **kw)
    torch.cuda.synchronize()
    assert same_bits(only, dst)
    for a, b in zip((dst, used, st), again):                  # two identical calls give identical bits
        assert same_bits(a, b)
    dst, used, st = dst.cpu().numpy(), used.cpu().numpy(), st.cpu().numpy()
    want_used = []
    for i in range(len(CENTER)):
        wd, wu, ws, tv, tc = R.filter_one(frames, CENTER[i], nbr[i], flows[i], None if masks is None else masks[i], tau, gains,
                                          None if ref is None else ref[i], terms=True)
        assert np_same_bits(dst[i], wd), (i, np.argwhere(dst[i] != wd)[:5])
        assert np.array_equal(used[i], wu), (i, np.argwhere(used[i] != wu)[:5])
        assert np.array_equal(st[i, :2], ws[:2]), (i, st[i], ws)
        if ref is None:
            assert st[i, 2] == 0 and st[i, 3] == 0
        else:
            check_sums(st[i], tv, tc)
        want_used.append(wu)
    return np.stack(want_used)


# ---- the dense form ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("noc", [1, 3])
@pytest.mark.parametrize("K", [1, 2, 4, 8])
def test_dense_equals_the_restatement(K, noc, u8):
    seen = set()
    for si, (h, w) in enumerate(SIZES):
        frames, ref, flows, masks = case(h, w, K, noc, u8, 1000 * K + 100 * noc + 10 * u8 + si)
        for tau in (2.0, 40.0):
            wu = assert_dense_matches(frames, K, flows, masks, tau, GAINS[:K], ref)
            seen.update(np.unique(wu).tolist())
        wu = assert_dense_matches(frames, K, flows, None, 40.0, None, None)         # no masks, unit gains, no ref
        seen.update(np.unique(wu).tolist())
    # both branches are populated: pixels no neighbour entered, and pixels every neighbour did
    assert 0 in seen and K in seen, sorted(seen)


def test_absent_zero_gain_and_masked_neighbours_are_left_out_and_an_identical_one_returns_the_centre():
    from flowonthego_amd.temporal import temporal_filter
    h, w, K = 19, 67, 4
    frames, ref, flows, masks = case(h, w, K, 1, False, 77)
    fr, fl = dev(frames), dev(flows)
    nbr = neighbors(K)
    gains = GAINS[:K]
    want = temporal_filter(fr, CENTER, [r[:1] + r[2:] for r in nbr], dev(flows[:, [0, 2, 3]]), tau=40.0, gains=gains[:1] + gains[2:],
                           ref=dev(ref), stats=True)
    absent = temporal_filter(fr, CENTER, [r[:1] + [-1] + r[2:] for r in nbr], fl, tau=40.0, gains=gains, ref=dev(ref), stats=True)
    nogain = temporal_filter(fr, CENTER, nbr, fl, tau=40.0, gains=gains[:1] + [0.0] + gains[2:], ref=dev(ref), stats=True)
    m = np.zeros((len(CENTER), K, h, w), np.uint8)
    m[:, 1] = 1
    masked = temporal_filter(fr, CENTER, nbr, fl, masks=dev(m), tau=40.0, gains=gains, ref=dev(ref), stats=True)
    torch.cuda.synchronize()
    for got in (absent, nogain, masked):
        for a, b, nm in zip(got, want, ("dst", "used", "stats")):
            assert same_bits(a, b), nm
    # one neighbour identical to the centre, zero flow: (C + 1 C) / 2 == C
    dst, used, st = temporal_filter(fr, [3], [[3]], torch.zeros((1, 1, h, w, 2), device="cuda"), ref=fr[3:4], stats=True)
    assert same_bits(dst[0], fr[3]) and (used == 1).all() and st[0].tolist() == [h * w, 0.0, 0.0, 0.0]


# ---- the C-ABI: each output alone, and every refused argument ---------------------------------------------------------------------
def _raw(h=9, w=11, K=2, n=2, nframes=3):
    import flowonthego_amd as F
    L = F.lib()
    rng = np.random.default_rng(5)
    st = dict(L=L, n=n, K=K, T=nframes, w=w, h=h, ch=1, tau=30.0,
              frames=dev(rng.random((nframes, h, w)).astype(f32) * 255),
              flows=dev((rng.standard_normal((n, K, h, w, 2)) * 0.3).astype(f32)),
              center=[0, 2], nbr=[1, -1, 1, 0], gains=[1.0, 0.5],
              dst=torch.full((n, h, w), -7.0, device="cuda"), used=torch.full((n, h, w), 99, dtype=torch.uint8, device="cuda"),
              stats=torch.full((n, 4), -7.0, dtype=torch.float64, device="cuda"))
    return st


def _call(s, **over):
    a = dict(s, **over)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    ints = lambda v: None if v is None else (C.c_int * len(v))(*v)
    flt = lambda v: None if v is None else (C.c_float * len(v))(*v)
    return a["L"].fotg_temporal_filter(0, a["n"], a["K"], a["T"], p(a["frames"]), a["w"], a["h"], a["ch"], ints(a["center"]),
                                       ints(a["nbr"]), p(a["flows"]), None, C.c_float(a["tau"]), flt(a["gains"]), None, p(a["dst"]),
                                       p(a["used"]), p(a["stats"]), None)


def test_each_output_alone():
    s = _raw()
    assert _call(s) == 0
    torch.cuda.synchronize()
    full = [s[k].clone() for k in ("dst", "used", "stats")]
    assert (full[1] <= s["K"]).all() and (full[2][:, 0] == full[1].sum(dim=(1, 2))).all()
    for keep in ("dst", "used", "stats"):
        t = _raw()
        assert _call(t, **{k: None for k in ("dst", "used", "stats") if k != keep}) == 0
        torch.cuda.synchronize()
        for k, f in zip(("dst", "used", "stats"), full):
            if k == keep:
                assert same_bits(t[k], f), keep
            else:
                assert (t[k] == (99 if k == "used" else -7.0)).all(), (keep, k)       # untouched


def test_arguments_are_refused_and_nothing_is_launched():
    import flowonthego_amd as F
    s = _raw()
    inf, nan = float("inf"), float("nan")
    bad = [dict(n=0), dict(n=-1), dict(K=0), dict(K=9), dict(T=0), dict(w=0), dict(h=-1), dict(ch=2), dict(ch=0),
           dict(tau=0.0), dict(tau=-1.0), dict(tau=inf), dict(tau=nan), dict(gains=[1.0, -0.5]), dict(gains=[nan, 1.0]),
           dict(gains=[1.0, inf]), dict(center=[0, 3]), dict(center=[-1, 0]), dict(nbr=[1, -2, 1, 0]), dict(nbr=[1, -1, 3, 0]),
           dict(frames=None), dict(flows=None), dict(center=None), dict(nbr=None), dict(dst=None, used=None, stats=None),
           dict(dst=s["frames"]), dict(dst=s["frames"][1:])]
    for b in bad:
        assert _call(s, **b) == FOTG_ERR_ARG, b
    torch.cuda.synchronize()
    assert (s["dst"] == -7.0).all() and (s["used"] == 99).all() and (s["stats"] == -7.0).all()
    assert _call(s, gains=None) == 0                              # no gains: all 1
    # the fused form
    L = s["L"]
    o = make_ctx(2, 64, 48, max_batch=4)
    wl, hl = o.out_size()
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    cf = torch.zeros((4, hl, wl, 2), device="cuda")
    fr = torch.zeros((3, 48, 64), device="cuda")
    out = torch.full((2, 48, 64), -7.0, device="cuda")
    ints = lambda v: None if v is None else (C.c_int * len(v))(*v)
    fused = lambda ctx=o._h, n=2, K=2, f=cf, s_=fr, ch=1, cen=(0, 2), nb=(1, -1, 1, 0), d=out: L.fotg_upsample_crop_temporal_filter(
        ctx, n, K, 3, p(f), p(s_), ch, ints(cen), ints(nb), None, C.c_float(30.0), None, None, p(d), None, None, None)
    for b in (dict(ctx=None), dict(n=3), dict(K=3), dict(n=0), dict(f=None), dict(s_=None), dict(ch=4), dict(cen=(0, 3)),
              dict(nb=(1, -1, 5, 0)), dict(d=None), dict(d=fr)):
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
        od.temporal_filter(fr)
    torch.cuda.synchronize()


# ---- the fused form ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,noc,u8", [(1, 1, False), (2, 3, True), (4, 1, True), (8, 3, False)])
def test_fused_equals_dense_on_the_upsampled_flow(K, noc, u8):
    from flowonthego_amd.temporal import temporal_filter
    n = len(CENTER)
    for w, h in ((130, 40), (67, 37)):                        # 67 x 37: the pyramid pads to 68 x 40
        rng = np.random.default_rng(300 + K + w)
        o = make_ctx(2, w, h, max_batch=n * K, finest_scale=1, coarsest_scale=2, use_var_ref=False)
        assert (o.padw, o.padh) != (0, 0)
        wl, hl = o.out_size()
        cf = (rng.standard_normal((n * K, hl, wl, 2)) * 0.3).astype(f32)
        cf[0, 0, :3] = (np.nan, 0.0)
        cf[-1, hl // 2, :2] = (np.inf, 1.0)
        frames, ref = dev(stack(rng, h, w, noc, u8)), dev(stack(rng, h, w, noc, u8)[:n])
        masks = dev(rng.choice(np.array([0] * 12 + [1, 2, 3, 7], np.uint8), (n, K, h, w)))
        kw = dict(masks=masks, tau=40.0, gains=GAINS[:K], ref=ref, stats=True)
        got = o.upsample_crop_temporal_filter(dev(cf), frames, CENTER, neighbors(K), fused=True, **kw)
        unf = o.upsample_crop_temporal_filter(dev(cf), frames, CENTER, neighbors(K), fused=False, **kw)
        want = temporal_filter(frames, CENTER, neighbors(K), o.upsample_crop(dev(cf)).view(n, K, h, w, 2), **kw)
        torch.cuda.synchronize()
        for g, u, w_, nm in zip(got, unf, want, ("dst", "used", "stats")):
            assert same_bits(g, w_) and same_bits(u, w_), nm
        assert got[2][1, 0].item() > 0 and got[1].max().item() > 0
        plain = o.upsample_crop_temporal_filter(dev(cf), frames, CENTER, neighbors(K), tau=2.0)
        assert same_bits(plain, temporal_filter(frames, CENTER, neighbors(K), o.upsample_crop(dev(cf)).view(n, K, h, w, 2), tau=2.0))


# ---- the whole thing in one call --------------------------------------------------------------------------------------------------
def sequence(alley, count=5, h=64, w=96):
    """a 96 x 64 window sliding over an alley_1 frame by (2, 1) pixels per frame, with noise sigma 4: (clean, noisy) float32"""
    big = alley["frame_0001"].astype(np.float64)
    clean = np.stack([big[180 + k:180 + k + h, 400 + 2 * k:400 + 2 * k + w] for k in range(count)])
    noisy = np.clip(clean + np.random.default_rng(9).normal(0, 4, clean.shape), 0, 255)
    return clean.astype(f32), noisy.astype(f32)


@pytest.mark.parametrize("radius", [1, 2])
@pytest.mark.parametrize("bidir", [False, True])
def test_ofclass_temporal_filter_is_the_explicit_sequence(radius, bidir, alley):
    import flowonthego_amd as F
    from flowonthego_amd.temporal import neighbor_table
    clean, noisy = (dev(a) for a in sequence(alley))
    K, mb = 2 * radius, 8
    o = make_ctx(2, 96, 64, max_batch=mb, bidir=bidir)
    gains = GAINS[:K]
    got = o.temporal_filter(noisy, radius=radius, tau=25.0, gains=gains, occlusion=bidir, ref=clean, stats=True)
    cen, nbr = neighbor_table(5, radius)
    assert nbr[0][:2] == [-1, 1] and nbr[4][:2] == [3, -1] and len(nbr[2]) == K
    per = mb // K
    parts = []
    for s in range(0, 5, per):
        c, nb = cen[s:s + per], nbr[s:s + per]
        i0 = [ci for ci in c for _ in range(K)]
        i1 = [b if b >= 0 else ci for ci, row in zip(c, nb) for b in row]
        I0, I1 = noisy[i0].contiguous(), noisy[i1].contiguous()
        masks = None
        if bidir:
            fw, bw = o.calc_bidirectional(I0, I1)
            masks = o.upsample_crop_fb_check(fw, bw)[0].view(len(c), K, 64, 96)
        else:
            fw = o.calc_batch(I0, I1)
        parts.append(o.upsample_crop_temporal_filter(fw, noisy, c, nb, masks=masks, tau=25.0, gains=gains, ref=clean[s:s + len(c)],
                                                     stats=True))
    torch.cuda.synchronize()
    for j, nm in enumerate(("dst", "used", "stats")):
        assert same_bits(got[j], torch.cat([p[j] for p in parts])), nm
    assert got[0].shape == noisy.shape and got[1].shape == (5, 64, 96) and got[2].shape == (5, 4)
    assert (got[2][:, 0] > 0).all()
    if not bidir:
        with pytest.raises(F.FotgError):
            o.temporal_filter(noisy, radius=radius, occlusion=True)


# ---- it does what it is for -------------------------------------------------------------------------------------------------------
def test_filtering_along_the_engine_flows_denoises_alley():
    """the quality case of tests/test_temporal.py through OFClass.temporal_filter at operating point 2 (the engine's flows are the
    oracle's): CPU figures noisy 28.41 dB, along the flows 33.71 dB, with zero flows 31.27 dB"""
    from flowonthego_amd.temporal import temporal_filter
    clean, noisy = R.quality_frames()
    h, w = clean.shape[1:]
    o = make_ctx(2, w, h, max_batch=6)
    fr = dev(noisy)
    dst, used, st = o.temporal_filter(fr, radius=1, tau=R.QUALITY_TAU, ref=dev(clean), stats=True)
    still = temporal_filter(fr, [1], [[0, 2]], torch.zeros((1, 2, h, w, 2), device="cuda"), tau=R.QUALITY_TAU)
    torch.cuda.synchronize()
    p_noisy = R.psnr(noisy[1], clean[1])
    p_along, p_still = R.psnr(dst[1].cpu().numpy(), clean[1]), R.psnr(still[0].cpu().numpy(), clean[1])
    print("PSNR of frame 2: noisy %.2f dB, filtered along the flows %.2f dB, with zero flows %.2f dB; mean used %.3f"
          % (p_noisy, p_along, p_still, st[1, 0].item() / (h * w)))
    assert p_along >= p_noisy + 3.0
    assert p_along > p_still
