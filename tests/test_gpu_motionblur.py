"""GPU tests of the motion blur along a flow (fotg_motion_blur / fotg_upsample_crop_motion_blur, flowonthego_amd.motionblur,
OFClass.motion_blur).

The definition is integer arithmetic after one f32 multiply (and, for f32 frames, f32 sums in a defined order), so every output equals
the numpy restatement (tests/motionblur_ref.py) byte for byte, and the fused form equals the dense one on fotg_upsample_crop's output
bit for bit.  No tolerance appears anywhere; every call is made twice and the bytes compared.

The sizes (tests/test_motionblur.py SIZES, which also asserts that the scenes reach every branch): 1 x 1, 5 x 3 (narrower than a
thread's four pixels), 33 x 70 (partial tiles on both axes, rows at every alignment), 70 x 130 (3 x 5 tiles: one tile has all nine
neighbours and a streak of the cap's length crosses a whole tile)."""
import ctypes as C

import numpy as np
import pytest
import torch

import motionblur_ref as R
from test_gpu_warp import dev, make_ctx, same_bits
from test_motionblur import N, SIZES, scene, want

pytestmark = pytest.mark.gpu

FOTG_ERR_ARG = 1
KINDS = ("u8-1", "u8-3", "f32-1", "f32-3")
ALL = dict(code=True, vectors=True, stats=True)


def assert_equal(got, want_, what):
    got = [g.cpu().numpy() for g in got]
    assert len(got) == len(want_)
    for k, (g, w_) in enumerate(zip(got, want_)):
        assert g.dtype == w_.dtype and g.shape == w_.shape, (what, k, g.dtype, g.shape, w_.dtype, w_.shape)
        gb, wb = (g.view(np.uint32), w_.view(np.uint32)) if g.dtype == np.float32 else (g, w_)
        assert np.array_equal(gb, wb), (what, k, np.argwhere(gb != wb)[:5].tolist())


def twice(fn):
    """two identical calls give identical bytes"""
    a, b = fn(), fn()
    a, b = (a if isinstance(a, tuple) else (a,)), (b if isinstance(b, tuple) else (b,))
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert same_bits(x, y)
    return a


# ---- the dense form -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("masked", [False, True])
def test_dense_equals_the_restatement(kind, masked):
    from flowonthego_amd.motionblur import motion_blur
    for h, w in SIZES:
        flow, mask, frames = scene(h, w)
        f, m, fr = dev(flow), (dev(mask) if masked else None), dev(frames[kind])
        wd, wc, wv, ws = want(h, w, kind, masked)
        assert_equal(twice(lambda: motion_blur(fr, f, m, **ALL)), (wd, wc, wv, ws), (h, w, "all"))
        assert_equal(twice(lambda: motion_blur(fr, f, m)), (wd,), (h, w, "dst"))
        assert_equal(twice(lambda: motion_blur(fr, f, m, vectors=True)), (wd, wv), (h, w, "vectors"))
        assert_equal(twice(lambda: motion_blur(fr, f, m, stats=True)), (wd, ws), (h, w, "stats"))
        assert ws[:, :4].sum() == N * h * w and not ws[:, 7].any()


@pytest.mark.parametrize("shutter", [1 / 256, 0.5, 2])
@pytest.mark.parametrize("max_blur", [1, 7, 32])
def test_parameters_and_a_single_image(shutter, max_blur):
    from flowonthego_amd.motionblur import motion_blur
    h, w = 33, 70
    flow, mask, frames = scene(h, w)
    s256 = R.shutter256(shutter)
    for kind in ("u8-3", "f32-1"):
        got = twice(lambda: motion_blur(dev(frames[kind]), dev(flow), dev(mask), shutter, max_blur, **ALL))
        wnt = want(h, w, kind, True, s256, max_blur)
        assert_equal(got, wnt, (kind, shutter, max_blur))
        assert wnt[3][:, R.MAX_LEN].max() <= 16 * max_blur
        one = motion_blur(dev(frames[kind][1]), dev(flow[1]), dev(mask[1]), shutter, max_blur, **ALL)
        assert_equal(one, [t[1] for t in wnt], "single")


def test_unaligned_pointers_take_the_scalar_paths():
    """views that start 8 bytes (flow), 1 byte (frame) and 1 byte (mask) into an allocation"""
    from flowonthego_amd.motionblur import motion_blur
    h, w = 70, 130
    flow, mask, frames = scene(h, w)
    shift = lambda t, per: torch.cat([t.flatten()[:per], t.flatten()])[per:].view(t.shape)
    df, dm, dfr = shift(dev(flow), 2), shift(dev(mask), 1), shift(dev(frames["u8-3"]), 1)
    assert df.data_ptr() % 16 == 8 and dm.data_ptr() % 4 == 1 and dfr.data_ptr() % 16 == 1 and df.is_contiguous()
    for args in ((dev(frames["u8-3"]), df, dev(mask)), (dfr, dev(flow), dev(mask)), (dev(frames["u8-3"]), dev(flow), dm), (dfr, df, dm)):
        assert_equal(twice(lambda: motion_blur(*args, **ALL)), want(h, w, "u8-3", True), "unaligned")


# ---- nothing is written outside the outputs ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["u8-3", "f32-1"])
def test_guard_rows_and_refused_calls(kind):
    import flowonthego_amd as F
    L = F.lib()
    _p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    h, w = 33, 70
    flow, mask, frames = scene(h, w)
    fr = frames[kind]
    ch, ty = (fr.shape[3] if fr.ndim == 4 else 1), (1 if fr.dtype == np.float32 else 0)
    wd, wc, wv, ws = want(h, w, kind, True)
    sent = -7 if ty else 249
    dst = torch.full((N * h + 2, w * ch), sent, dtype=torch.float32 if ty else torch.uint8, device="cuda")
    code = torch.full((N * h + 2, w), 249, dtype=torch.uint8, device="cuda")
    vec = torch.full((N * h + 2, w * 2), -7, dtype=torch.int16, device="cuda")
    st = torch.full((N + 2, 8), -7, dtype=torch.int64, device="cuda")
    d = [dev(t) for t in (fr, flow, mask)]
    outs = (dst, code, vec, st)

    def call(n=N, s=d[0], ty_=ty, ch_=ch, f=d[1], w_=w, h_=h, m=d[2], sh=128, mb=32, o=dst[1:], c=code[1:], v=vec[1:], t=st[1:]):
        return L.fotg_motion_blur(0, n, _p(s), ty_, ch_, _p(f), w_, h_, _p(m), sh, mb, _p(o), _p(c), _p(v), _p(t), None)

    # a refused call writes nothing at all
    for bad in (dict(n=0), dict(n=65536), dict(w_=0), dict(h_=16385), dict(ty_=2), dict(ch_=2), dict(sh=0), dict(sh=513), dict(mb=0), dict(mb=33),
                dict(s=None), dict(f=None), dict(o=None), dict(o=d[0]), dict(c=d[2]), dict(v=d[1]), dict(t=d[1]), dict(c=dst[1:]), dict(v=code[1:]),
                dict(t=vec[1:]), dict(m=code[1:])):
        assert call(**bad) == FOTG_ERR_ARG, list(bad)
    torch.cuda.synchronize()
    for t, s in zip(outs, (sent, 249, -7, -7)):
        assert bool((t == s).all())
    # a good call writes between the guard rows only
    for _ in range(2):
        assert call() == 0
        torch.cuda.synchronize()
        for t, s, w_ in zip(outs, (sent, 249, -7, -7), (wd, wc, wv, ws)):
            assert bool((t[0] == s).all()) and bool((t[-1] == s).all())
            got = t[1:-1].cpu().numpy().reshape(w_.shape)
            assert np.array_equal(got.view(np.uint32) if ty and t is dst else got, w_.view(np.uint32) if ty and t is dst else w_)
    assert call(c=None, v=None, t=None) == 0 and call(m=None) == 0


# ---- the fused form ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sc_l", [1, 2])
def test_fused_equals_dense_on_upsample_crop(sc_l):
    from flowonthego_amd.motionblur import motion_blur
    rng = np.random.default_rng(50 + sc_l)
    n = N
    for w, h in ((97, 61), (64, 48)):
        o = make_ctx(2, w, h, max_batch=n, finest_scale=sc_l, coarsest_scale=max(sc_l, 4), use_var_ref=False)
        wl, hl = o.out_size()
        assert wl < w and hl < h
        cf = (rng.standard_normal((n, hl, wl, 2)) * 6.0 / (1 << sc_l)).astype(np.float32)
        cf[2] *= np.float32(0.01)                                 # a still image: every tile on the copy path
        cf[0, hl // 2, wl // 2:wl // 2 + 3] = (np.nan, 0.0)
        cf[1, hl // 3, wl // 3:wl // 3 + 2] = (np.inf, 1.0)
        cf[2, hl // 2, wl // 4] = (0.0, -np.inf)                  # (every output pixel it reaches is unknown: the image stays still)
        cf = dev(cf)
        mask = dev(rng.choice(np.array([0, 0, 0, 0, 0, 1, 2, 3], np.uint8), (n, h, w)))
        dense = o.upsample_crop(cf)
        for kind, fr in (("u8", dev(rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8))), ("f32", dev(rng.standard_normal((n, h, w)).astype(np.float32)))):
            for m, shutter, max_blur in ((None, 0.5, 32), (mask, 1.0, 5)):
                got = twice(lambda: o.upsample_crop_motion_blur(cf, fr, m, shutter, max_blur, **ALL))
                unf = o.upsample_crop_motion_blur(cf, fr, m, shutter, max_blur, fused=False, **ALL)
                ref = motion_blur(fr, dense, m, shutter, max_blur, **ALL)
                torch.cuda.synchronize()
                assert len(got) == len(unf) == len(ref) == 4
                for a, b, c in zip(got, unf, ref):
                    assert same_bits(a, b) and same_bits(a, c), (w, h, kind)
                st = got[3].cpu().numpy()
                assert (st[:, R.C3] > 0).all() and st[:, R.C1].sum() > 0 and st[2, R.COPY_TILES] > 0
                assert_equal(got, R.blur(fr.cpu().numpy(), dense.cpu().numpy(), None if m is None else m.cpu().numpy(), R.shutter256(shutter), max_blur),
                             "restatement")
        o.close()


# ---- the whole thing in one call --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bidir", [False, True])
def test_ofclass_motion_blur_is_the_documented_composition(bidir, natural_images):
    import flowonthego_amd as F
    import motion_ref as M
    frames, _ = M.jittered_crops(natural_images["road_HD"], T=3, patch=True)
    T, (h, w) = len(frames) - 1, frames.shape[1:]
    dfr = dev(frames)
    o = make_ctx(2, w, h, max_batch=2, bidir=bidir)                 # three flows in chunks of two and one
    got = o.motion_blur(dfr, shutter=1.0, max_blur=16, occlusion=bidir)
    parts = []
    for k in range(T):
        pair = dfr[k:k + 2].contiguous()
        if bidir:
            fw, bw = o.calc_sequence_bidirectional(pair)
            mask = o.upsample_crop_fb_check(fw, bw)[0]
        else:
            fw, mask = o.calc_sequence(pair), None
        parts.append(F.motion_blur(dfr[k:k + 1], o.upsample_crop(fw), mask, 1.0, 16))
    torch.cuda.synchronize()
    assert got.shape == (T, h, w) and got.dtype == torch.uint8 and same_bits(got, torch.cat(parts))
    assert bool((got != dfr[:T]).any())
    if bidir:
        assert not same_bits(got, o.motion_blur(dfr, shutter=1.0, max_blur=16))          # the mask matters
    else:
        with pytest.raises(F.FotgError):
            o.motion_blur(dfr, occlusion=True)
    for bad in (dict(shutter=0), dict(max_blur=33)):
        with pytest.raises(F.FotgError):
            o.motion_blur(dfr, **bad)
    with pytest.raises(F.FotgError):
        o.motion_blur(dfr[:1])
    o.close()


# ---- errors and streams -----------------------------------------------------------------------------------------------------------
def test_python_layer_refusals():
    import flowonthego_amd as F
    from flowonthego_amd.motionblur import motion_blur
    n, h, w = 2, 16, 24
    flow = torch.zeros((n, h, w, 2), device="cuda")
    frame = torch.zeros((n, h, w, 3), dtype=torch.uint8, device="cuda")
    mask = torch.zeros((n, h, w), dtype=torch.uint8, device="cuda")
    assert same_bits(motion_blur(frame, flow, mask), frame)
    for kw in (dict(shutter=0), dict(shutter=-0.5), dict(shutter=2.01), dict(shutter=0.001), dict(shutter=True), dict(shutter="1"), dict(max_blur=0),
               dict(max_blur=33), dict(max_blur=4.0), dict(mask=mask[:1]), dict(mask=mask.to(torch.int32)), dict(mask=mask[:, :, :-1].contiguous())):
        with pytest.raises(F.FotgError):
            motion_blur(frame, flow, **kw)
    for fr in (frame.to(torch.float64), frame.to(torch.int16), frame[..., :2].contiguous(), frame[:, :-1].contiguous(), frame[:1], frame.cpu(),
               frame.permute(0, 2, 1, 3), None):
        with pytest.raises(F.FotgError):
            motion_blur(fr, flow)
    for fl in (flow.to(torch.float64), flow[..., :1].contiguous(), flow.cpu(), None):
        with pytest.raises(F.FotgError):
            motion_blur(frame, fl)
    o = make_ctx(2, 64, 48, max_batch=2)
    wl, hl = o.out_size()
    cf = torch.zeros((2, hl, wl, 2), device="cuda")
    fr = torch.zeros((2, 48, 64), dtype=torch.float32, device="cuda")
    assert same_bits(o.upsample_crop_motion_blur(cf, fr), fr)
    for args, kw in (((cf[:, :-1].contiguous(), fr), {}), ((torch.zeros((3, hl, wl, 2), device="cuda"), fr), {}), ((cf, fr[:1]), {}),
                     ((cf, fr), dict(shutter=3)), ((cf, fr), dict(max_blur=0)), ((cf, fr.to(torch.float64)), {})):
        with pytest.raises(F.FotgError):
            o.upsample_crop_motion_blur(*args, **kw)
    o.close()


def test_a_call_on_another_stream():
    from flowonthego_amd.motionblur import motion_blur
    h, w = 70, 130
    flow, mask, frames = scene(h, w)
    f, m, fr = dev(flow), dev(mask), dev(frames["f32-3"])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got = motion_blur(fr, f, m, **ALL)
    s.synchronize()
    assert_equal(got, want(h, w, "f32-3", True), "stream")
