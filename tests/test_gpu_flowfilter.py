"""GPU tests of the edge- and occlusion-aware flow filter (fotg_flow_filter / fotg_upsample_crop_flow_filter and their 8-bit-guide
forms, flowonthego_amd.flowfilter, OFClass.calc_filtered).

The dense form equals the numpy restatement (tests/flowfilter_ref.py) byte for byte in out and code and exactly in the three counts;
the one exception is that any NaN equals any NaN (the default NaN of the GPU and of the host differ in sign), so NaN positions and
all other bytes are compared.  The change sum is bounded against math.fsum of the restatement's terms by N 2^-53 fsum, the bound of
any order of adding N non-negative doubles (tests/test_gpu_warp.py derives it).  The fused form equals the dense form of
fotg_upsample_crop's output bit for bit in all three outputs.

The sizes are the smallest at which the kernel's paths differ (its tile is 64 x 16, its halo up to 7): 1 x 1 (one pixel), 3 x 5
(smaller than any window), 19 x 67 and 40 x 130 (tile borders crossed in both directions, a halo that reaches into a neighbouring
tile, a width that is no multiple of four)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import flowfilter_ref as R
from test_gpu_warp import dev, make_ctx, same_bits

pytestmark = pytest.mark.gpu

FOTG_ERR_ARG = 1
f32 = np.float32
SIZES = ((1, 1), (3, 5), (19, 67), (40, 130))          # (h, w)
ODD = np.array([np.nan, np.inf, -np.inf, 2e9, -2e9, 3e38, -3e38, -0.0], f32)
# (iters, tau, Gaussian spatial table?) per size: both pass counts, both taus, the box and the Gaussian
COMBOS = ((1, 2.0, False), (2, 40.0, True), (1, 40.0, True), (2, 2.0, False))


def case(h, w, noc, u8, seed, n=3):
    """n images of different content: a piecewise-smooth flow with non-finite and huge entries, a guide with steps and noise (so
    that at tau 2 and at tau 40 some weights are positive and some are not), a mask with all four codes and bytes above 3"""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w]
    flow = (rng.standard_normal((n, h, w, 2)) * 2.0).astype(f32)
    flow[:, :, w // 2:] += f32(5.0)
    flat = flow.reshape(-1)
    idx = rng.choice(flat.size, max(1, min(40, flat.size // 4)), replace=False)
    flat[idx] = ODD[np.arange(idx.size) % ODD.size]
    base = 100.0 + 6.0 * np.sin(ys / 3.0) + 5.0 * np.cos(xs / 4.0) + 60.0 * (xs > 0.45 * w) - 40.0 * (ys > 0.6 * h)
    g = base[None] + rng.normal(0, 2.0, (n, h, w))
    if noc == 3:
        g = np.stack([g, 255 - g, g[:, ::-1]], -1) + rng.normal(0, 1.0, (n, h, w, 3))
    g = np.clip(g, 0, 255)
    guide = np.rint(g).astype(np.uint8) if u8 else g.astype(f32)
    mask = rng.choice(np.array([0] * 10 + [1, 2, 3, 7, 200], np.uint8), (n, h, w))
    return flow, guide, mask


def check_sum(got, terms):
    """|gpu - fsum(terms)| <= N 2^-53 fsum(terms), printed before asserted"""
    want = math.fsum(terms)
    bound = len(terms) * 2.0 ** -53 * want
    print("change sum: gpu %.17g fsum %.17g |d| %.3g bound %.3g (N = %d)" % (got, want, abs(got - want), bound, len(terms)))
    assert abs(got - want) <= bound


def assert_dense_matches(flow, guide, mask, radius, spatial, tau, iters):
    """the batch through the GPU against the restatement image by image; returns the restatement's codes"""
    from flowonthego_amd.flowfilter import filter_flow
    t = lambda a: None if a is None else dev(a)
    args = (t(flow), t(guide))
    kw = dict(mask=t(mask), radius=radius, spatial=None if spatial is None else [float(v) for v in spatial], tau=tau, iters=iters)
    out, code, st = filter_flow(*args, stats=True, **kw)
    again = filter_flow(*args, stats=True, **kw)
    only = filter_flow(*args, **kw)
    torch.cuda.synchronize()
    assert same_bits(only, out)
    for a, b in zip((out, code, st), again):                      # two identical calls give identical bits
        assert same_bits(a, b)
    out, code, st = out.cpu().numpy(), code.cpu().numpy(), st.cpu().numpy()
    codes = []
    for i in range(len(flow)):
        wo, wc, ws, terms = R.filter_one(flow[i], guide[i], None if mask is None else mask[i], radius, spatial, tau, iters, terms=True)
        assert np.array_equal(code[i], wc), (i, np.argwhere(code[i] != wc)[:5])
        assert R.same_but_nan(out[i], wo), (i, np.argwhere(out[i].view(np.uint32) != wo.view(np.uint32))[:5])
        assert np.array_equal(st[i, :3], ws[:3]), (i, st[i], ws)
        check_sum(st[i, 3], terms)
        codes.append(wc)
    return np.stack(codes)


# ---- the dense form ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("noc", [1, 3])
@pytest.mark.parametrize("radius", [1, 3, 7])
def test_dense_equals_the_restatement(radius, noc, u8):
    seen = set()
    gauss = R.spatial_table(radius, radius / 2.0)
    for si, (h, w) in enumerate(SIZES):
        flow, guide, mask = case(h, w, noc, u8, 1000 * radius + 100 * noc + 10 * u8 + si)
        for iters, tau, g in COMBOS:
            wc = assert_dense_matches(flow, guide, mask, radius, gauss if g else None, tau, iters)
            seen.update(np.unique(wc).tolist())
        assert_dense_matches(flow, guide, None, radius, gauss, 40.0, 2)               # no mask
    assert seen == {0, 1, 3}, sorted(seen)                                            # every branch is populated


def test_fully_masked_image_passes_through_and_the_table_of_the_module_is_the_restatements():
    from flowonthego_amd.flowfilter import filter_flow, spatial_table
    for r, s in ((1, 0.5), (3, 1.5), (7, 3.0), (7, 0.3)):
        assert np.array_equal(np.array(spatial_table(r, s), f32), R.spatial_table(r, s))
    flow, guide, _ = case(19, 67, 1, False, 5)
    mask = np.full((3, 19, 67), 1, np.uint8)
    mask[1] = 3
    mask[2] = 200
    for iters in (1, 3):
        out, code, st = filter_flow(dev(flow), dev(guide), mask=dev(mask), radius=3, iters=iters, stats=True)
        torch.cuda.synchronize()
        assert (code == 3).all() and same_bits(out, dev(flow))
        assert st.cpu().tolist() == [[0.0, 0.0, 19.0 * 67, 0.0]] * 3
    # a single image without the batch dimension
    o1, c1, s1 = filter_flow(dev(flow[1]), dev(guide[1]), radius=3, sigma=1.5, iters=2, stats=True)
    ob, cb, sb = filter_flow(dev(flow), dev(guide), radius=3, sigma=1.5, iters=2, stats=True)
    assert same_bits(o1, ob[1]) and same_bits(c1, cb[1]) and same_bits(s1, sb[1])
    import flowonthego_amd as F
    assert same_bits(F.filter_flow(dev(flow), dev(guide), radius=3, sigma=1.5, iters=2), ob)


def test_iters_equals_single_passes_composed_by_hand():
    from flowonthego_amd.flowfilter import filter_flow
    flow, guide, mask = case(40, 130, 3, True, 6)
    mask[0, 5:30, 20:60] = 1                                       # an island wider than 2 R + 1
    kw = dict(radius=2, sigma=1.0, tau=40.0)
    f, g = dev(flow), dev(guide)
    cur, m, first = f, dev(mask), None
    for k in range(1, 5):
        cur, cd = filter_flow(cur, g, mask=m, code=True, **kw)
        first = cd if first is None else first
        m = (cd == 3).to(torch.uint8)
        final = torch.where(cd == 3, torch.full_like(cd, 3), torch.where(first == 0, torch.zeros_like(cd), torch.ones_like(cd)))
        out, code = filter_flow(f, g, mask=dev(mask), iters=k, code=True, **kw)
        only_code_and_stats = filter_flow(f, g, mask=dev(mask), iters=k, stats=True, **kw)
        torch.cuda.synchronize()
        assert same_bits(out, cur) and same_bits(code, final), k
        assert same_bits(only_code_and_stats[1], final)
    assert (code[0] == 3).sum().item() < (first[0] == 3).sum().item()


# ---- the C-ABI: each output alone, and every refused argument ---------------------------------------------------------------------
def _raw(h=21, w=70, n=2):
    import flowonthego_amd as F
    rng = np.random.default_rng(5)
    return dict(L=F.lib(), n=n, w=w, h=h, ch=1, R=2, tau=20.0, iters=2, spatial=[1.0, 0.5, 0.25],
                flow=dev((rng.standard_normal((n, h, w, 2))).astype(f32)), guide=dev((rng.random((n, h, w)) * 60).astype(f32)),
                mask=dev(rng.choice(np.array([0, 0, 0, 1], np.uint8), (n, h, w))),
                out=torch.full((n, h, w, 2), -7.0, device="cuda"), code=torch.full((n, h, w), 99, dtype=torch.uint8, device="cuda"),
                stats=torch.full((n, 4), -7.0, dtype=torch.float64, device="cuda"))


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _call(s, **over):
    a = dict(s, **over)
    sp = None if a["spatial"] is None else (C.c_float * len(a["spatial"]))(*a["spatial"])
    return a["L"].fotg_flow_filter(0, a["n"], _p(a["flow"]), _p(a["guide"]), a["w"], a["h"], a["ch"], _p(a["mask"]), a["R"], sp,
                                   C.c_float(a["tau"]), a["iters"], _p(a["out"]), _p(a["code"]), _p(a["stats"]), None)


@pytest.mark.parametrize("iters", [1, 2, 3])
def test_each_output_alone(iters):
    s = _raw()
    assert _call(s, iters=iters) == 0
    torch.cuda.synchronize()
    full = [s[k].clone() for k in ("out", "code", "stats")]
    assert (full[2][:, :3].sum(dim=1) == s["h"] * s["w"]).all() and (full[1] != 99).all()
    for keep in ("out", "code", "stats"):
        t = _raw()
        assert _call(t, iters=iters, **{k: None for k in ("out", "code", "stats") if k != keep}) == 0
        torch.cuda.synchronize()
        for k, f in zip(("out", "code", "stats"), full):
            if k == keep:
                assert same_bits(t[k], f), keep
            else:
                assert (t[k] == (99 if k == "code" else -7.0)).all(), (keep, k)       # untouched


def test_arguments_are_refused_and_nothing_is_launched():
    import flowonthego_amd as F
    s = _raw()
    inf, nan = float("inf"), float("nan")
    bad = [dict(n=0), dict(n=-1), dict(n=65536), dict(w=0), dict(h=-1), dict(ch=2), dict(ch=0), dict(ch=4), dict(R=0), dict(R=8),
           dict(R=-1), dict(iters=0), dict(iters=5), dict(tau=0.0), dict(tau=-1.0), dict(tau=inf), dict(tau=nan),
           dict(spatial=[1.0, -0.5, 0.25]), dict(spatial=[1.0, 1.5, 0.25]), dict(spatial=[1.0, nan, 0.25]),
           dict(spatial=[1.0, 0.5, inf]), dict(spatial=[0.0, 0.5, 0.25]), dict(flow=None), dict(guide=None),
           dict(out=None, code=None, stats=None), dict(out=s["flow"]), dict(out=s["flow"][1:])]
    for b in bad:
        assert _call(s, **b) == FOTG_ERR_ARG, b
    torch.cuda.synchronize()
    assert (s["out"] == -7.0).all() and (s["code"] == 99).all() and (s["stats"] == -7.0).all()
    assert _call(s, spatial=None) == 0 and _call(s, spatial=[1.0, 0.0, 1.0]) == 0      # no table: all 1; zeros are allowed past s[0]
    # the fused form
    L = s["L"]
    o = make_ctx(2, 64, 48, max_batch=2)
    wl, hl = o.out_size()
    cf = torch.zeros((2, hl, wl, 2), device="cuda")
    gd = torch.zeros((2, 48, 64), device="cuda")
    out = torch.full((2, 48, 64, 2), -7.0, device="cuda")
    fused = lambda ctx=o._h, n=2, f=cf, g=gd, ch=1, R=3, tau=20.0, iters=1, d=out: L.fotg_upsample_crop_flow_filter(
        ctx, n, _p(f), _p(g), ch, None, R, None, C.c_float(tau), iters, _p(d), None, None, None)
    for b in (dict(ctx=None), dict(n=3), dict(n=0), dict(f=None), dict(g=None), dict(ch=2), dict(R=0), dict(R=8), dict(iters=0),
              dict(iters=5), dict(tau=0.0), dict(tau=nan), dict(d=None), dict(d=cf)):
        assert fused(**b) == FOTG_ERR_ARG, b
    torch.cuda.synchronize()
    assert (out == -7.0).all()
    assert fused() == 0
    op = F.operating_point(2, 64, 1)
    op.depth_mode = True
    from flowonthego_amd.oflow import OFClass
    od = OFClass(op, F.img_params(width=64, height=48), max_batch=2)
    assert fused(ctx=od._h) == FOTG_ERR_ARG
    with pytest.raises(F.FotgError):
        od.calc_filtered(gd, gd, occlusion=False)
    with pytest.raises(F.FotgError):
        o.calc_filtered(gd, gd)                                    # occlusion=True needs a bidir context
    for kw in (dict(radius=0), dict(radius=8), dict(sigma=0.0), dict(sigma=1.0, spatial=[1.0] * 4), dict(spatial=[1.0] * 3)):
        with pytest.raises(F.FotgError):
            o.upsample_crop_filter_flow(cf, gd, **kw)
    torch.cuda.synchronize()


# ---- the fused form ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noc,u8,radius,iters", [(1, False, 3, 1), (3, True, 7, 2), (1, True, 1, 3), (3, False, 2, 4)])
def test_fused_equals_dense_on_the_upsampled_flow(noc, u8, radius, iters):
    from flowonthego_amd.flowfilter import filter_flow
    n = 3
    for w, h in ((128, 40), (67, 37)):                        # 128 x 40 needs no padding; 67 x 37: the pyramid pads to 68 x 40
        rng = np.random.default_rng(300 + radius + w)
        o = make_ctx(2, w, h, max_batch=n, finest_scale=1, coarsest_scale=2, use_var_ref=False)
        assert ((o.padw, o.padh) != (0, 0)) == (w == 67)
        wl, hl = o.out_size()
        cf = (rng.standard_normal((n, hl, wl, 2)) * 1.5).astype(f32)
        cf[0, 0, :3] = (np.nan, 0.0)
        cf[-1, hl // 2, :2] = (np.inf, 1.0)
        cf[1, hl // 3, wl // 2] = (3e38, -3e38)
        _, guide, mask = case(h, w, noc, u8, 40 + w)
        guide, mask, cf = dev(guide), dev(mask), dev(cf)
        kw = dict(mask=mask, radius=radius, sigma=radius / 2.0, tau=40.0, iters=iters, stats=True)
        got = o.upsample_crop_filter_flow(cf, guide, fused=True, **kw)
        unf = o.upsample_crop_filter_flow(cf, guide, fused=False, **kw)
        want = filter_flow(o.upsample_crop(cf), guide, **kw)
        torch.cuda.synchronize()
        for g, u, w_, nm in zip(got, unf, want, ("out", "code", "stats")):
            assert same_bits(g, w_) and same_bits(u, w_), nm
        assert (got[2][:, 0] > 0).all() and (got[2][:, 1] > 0).all() and (got[2][:, 3] > 0).all()
        plain = o.upsample_crop_filter_flow(cf, guide, radius=radius, tau=2.0, iters=iters)
        assert same_bits(plain, filter_flow(o.upsample_crop(cf), guide, radius=radius, tau=2.0, iters=iters))


# ---- the whole thing in one call --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("occlusion", [False, True])
def test_ofclass_calc_filtered_is_the_explicit_sequence(occlusion, alley):
    from test_gpu_temporal import sequence
    _, frames = sequence(alley)
    frames = dev(frames)
    I0, I1 = frames[:4].contiguous(), frames[1:5].contiguous()
    mb = 3                                                         # two chunks: 3 pairs and 1
    o = make_ctx(2, 96, 64, max_batch=mb, bidir=occlusion)
    kw = dict(radius=3, sigma=1.5, tau=25.0, iters=2, stats=True)
    got = o.calc_filtered(I0, I1, occlusion=occlusion, both=occlusion, **kw)
    parts_fw, parts_bw = [], []
    for s in range(0, 4, mb):
        a, b = I0[s:s + mb], I1[s:s + mb]
        if occlusion:
            fw, bw = o.calc_bidirectional(a, b)
            m, m_bw = o.upsample_crop_fb_check(fw, bw)
            parts_bw.append(o.upsample_crop_filter_flow(bw, b, mask=m_bw, **kw))
        else:
            fw, m = o.calc_batch(a, b), None
        parts_fw.append(o.upsample_crop_filter_flow(fw, a, mask=m, **kw))
    torch.cuda.synchronize()
    for res, parts in ((got[0], parts_fw), (got[1], parts_bw)) if occlusion else ((got, parts_fw),):
        assert res[0].shape == (4, 64, 96, 2) and res[1].shape == (4, 64, 96) and res[2].shape == (4, 4)
        for j, nm in enumerate(("out", "code", "stats")):
            assert same_bits(res[j], torch.cat([p[j] for p in parts])), nm
        assert (res[2][:, 0] > 0).all()
    if occlusion:
        assert (got[0][2][:, 1] > 0).any()                         # some occluded pixels were filled
        only = o.calc_filtered(I0, I1, **dict(kw, stats=False))
        assert same_bits(only, got[0][0])


# ---- it does what it is for -------------------------------------------------------------------------------------------------------
def test_quality_case_gives_the_restatements_bytes():
    """the synthetic scene of tests/test_flowfilter.py: the GPU returns the restatement's bytes, hence its EPE figures (whole frame
    0.933 -> 0.149 px, boundary belt 1.683 -> 0.987 px, occluded band 28.66 -> 0.117 px)"""
    from flowonthego_amd.flowfilter import filter_flow
    true, bad, guide, mask, regions = R.quality_scene()
    q = R.QUALITY
    out, code, st = filter_flow(dev(bad), dev(guide), mask=dev(mask), radius=q["radius"], sigma=q["sigma"], tau=q["tau"],
                                iters=q["iters"], stats=True)
    wo, wc, ws = R.filter_one(bad, guide, mask, q["radius"], R.spatial_table(q["radius"], q["sigma"]), q["tau"], q["iters"])
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    for k, m in regions.items():
        print("EPE %s: before %.4f after %.4f (restatement %.4f)" % (k, R.epe(bad, true, m), R.epe(out, true, m), R.epe(wo, true, m)))
    assert R.same_but_nan(out, wo) and np.array_equal(code.cpu().numpy(), wc) and np.array_equal(st.cpu().numpy()[:3], ws[:3])
    assert R.epe(out, true, regions["band"]) < 1.0
