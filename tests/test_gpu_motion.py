"""GPU tests of the global-motion fit (fotg_fit_motion / fotg_upsample_crop_fit_motion / fotg_motion_flow, flowonthego_amd.motion)
and of stabilize.

Every output -- the parameters as f64 bits, code, residual, the counts and the twelve sums -- equals the numpy restatement
(tests/motion_ref.py) byte for byte, for every model, with and without a mask, after round 0 and after three more rounds, with
either ending of the reduction; the fused form equals the dense form over fotg_upsample_crop's output; stabilize on integer camera
steps returns the crops at the smoothed offsets byte for byte."""
import ctypes as C

import numpy as np
import pytest
import torch

import motion_ref as R

pytestmark = pytest.mark.gpu

FOTG_ERR_ARG = 1
f32 = np.float32
KEYS = ("params", "code", "residual", "stats", "sums")


def _F():
    import flowonthego_amd as F
    from flowonthego_amd.oflow import OFClass
    return F, OFClass


def dev(a, dtype=None):
    a = np.asarray(a)
    return torch.from_numpy(np.array(a, dtype=dtype or a.dtype, order="C")).cuda()       # (a copy: the shared references stay read-only)


def make_ctx(op_point, w, h, max_batch=1, bidir=False, **kw):
    F, OFClass = _F()
    op = F.operating_point(op_point, w, 1)
    op.bidir = bidir
    for k, v in kw.items():
        setattr(op, k, v)
    return OFClass(op, F.img_params(width=w, height=h), max_batch=max_batch)


def bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else (a.view(np.uint64) if a.dtype == np.float64 else a)


def same(a, b):
    """byte for byte; where the restatement b holds a NaN (the residual of a NaN vector) a NaN, whatever its payload"""
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == np.float32:
        nan = np.isnan(b)
        return np.array_equal(np.isnan(a), nan) and np.array_equal(bits(a)[~nan], bits(b)[~nan])
    return np.array_equal(bits(a), bits(b))


def p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


# ---- the cases and their restatement, computed once ------------------------------------------------------------------------------
SHAPES = {"67x45x3": (67, 45, 3),          # a partial last workgroup, no row a multiple of four, a batch
          "640x420": (640, 420, 1),        # 263 workgroups: more than one round of a 256-thread fold
          "1x1": (1, 1, 2), "33x1": (33, 1, 1), "3x2": (3, 2, 1)}
_IN, _REF = {}, {}


def inputs(name):
    """(flow (n, h, w, 2), mask (n, h, w)) of a shape, seeded"""
    if name not in _IN:
        w, h, n = SHAPES[name]
        sc = [R.make_scene(w, h, seed=40 + i) for i in range(n)]
        flow, mask = np.stack([s[0] for s in sc]), np.stack([s[1] for s in sc])
        if name == "67x45x3":
            mask[2] = 1                                     # one image of the batch with everything masked: the others are unaffected
        if name == "1x1":
            mask[1] = 3
        for a in (flow, mask):
            a.setflags(write=False)
        _IN[name] = (flow, mask)
    return _IN[name]


def reference(name, model, masked, iters):
    key = (name, model, masked, iters)
    if key not in _REF:
        flow, mask = inputs(name)
        res = [R.fit(flow[i], mask[i] if masked else None, model, iters) for i in range(len(flow))]
        out = {k: np.stack([r[k] for r in res]) for k in KEYS}
        for a in out.values():
            a.setflags(write=False)
        _REF[key] = out
    return _REF[key]


def gpu_fit(flow, mask, model, iters, **kw):
    from flowonthego_amd.motion import fit_motion
    return dict(zip(KEYS, fit_motion(flow, mask, R.MODELS[model], iters, 1.0, code=True, residual=True, stats=True, sums=True, **kw)))


def raw_fit(flow, mask, model, iters, off=1):
    """fotg_fit_motion into slices that start `off` elements into larger tensors (off = 1: code and residual are neither dword nor
    16-byte aligned), each tensor pre-filled: -> (outputs, guards untouched)"""
    L = _F()[0].lib()
    n, h, w = flow.shape[:3]
    sizes = dict(params=(n * 6, torch.float64, -7.0), code=(n * h * w, torch.uint8, 9), residual=(n * h * w * 2, torch.float32, -7.0),
                 stats=(n * 6, torch.int64, -1), sums=(n * 12, torch.int64, -1))
    big = {k: torch.full((sz + 8,), fillv, dtype=dt, device="cuda") for k, (sz, dt, fillv) in sizes.items()}
    out = {k: big[k][off:off + sizes[k][0]] for k in KEYS}
    assert L.fotg_fit_motion(0, n, p(flow), p(mask), w, h, model, iters, C.c_float(1.0), *(p(out[k]) for k in KEYS), None) == 0
    torch.cuda.synchronize()
    clean = all(bool((big[k][:off] == sizes[k][2]).all()) and bool((big[k][off + sizes[k][0]:] == sizes[k][2]).all()) for k in KEYS)
    shapes = dict(params=(n, 6), code=(n, h, w), residual=(n, h, w, 2), stats=(n, 6), sums=(n, 12))
    return {k: out[k].view(shapes[k]) for k in KEYS}, clean


# ---- byte for byte against the restatement -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_fit_equals_the_restatement(name):
    L = _F()[0].lib()
    flow, mask = inputs(name)
    dF, dM = dev(flow), dev(mask)
    fitted = set()
    for model in (0, 1, 2):
        for masked in (False, True):
            for iters in (0, 3):
                want = reference(name, model, masked, iters)
                got = gpu_fit(dF, dM if masked else None, model, iters)
                unal, clean = raw_fit(dF, dM if masked else None, model, iters)
                prev = L.fotg_motion_ending(-1)                    # the other ending of the reduction (atomics / partials and a fold)
                L.fotg_motion_ending(1 - prev)
                try:
                    fold = gpu_fit(dF, dM if masked else None, model, iters)
                    torch.cuda.synchronize()
                finally:
                    L.fotg_motion_ending(prev)
                for which, g in (("fit_motion", got), ("unaligned", unal), ("other ending", fold)):
                    for k in ("sums", "params", "stats", "code", "residual"):
                        assert same(g[k], want[k]), (which, model, masked, iters, k, g[k].cpu().numpy().ravel()[:12], want[k].ravel()[:12])
                assert clean, (model, masked, iters)
                fitted.update(int(v) for v in want["stats"][:, 5])
    if name == "67x45x3":
        assert fitted == {0, 1}                                    # the image with everything masked, and the others
    if name in ("1x1", "33x1"):
        assert 0 in fitted


def test_outputs_are_optional_and_one_image_equals_itself_in_a_batch():
    from flowonthego_amd.motion import fit_motion
    flow, mask = inputs("67x45x3")
    dF, dM = dev(flow), dev(mask)
    want = reference("67x45x3", 1, True, 3)
    only = fit_motion(dF, dM, "similarity")
    assert isinstance(only, torch.Tensor) and same(only, want["params"])
    pr, sm = fit_motion(dF, dM, "similarity", sums=True)                       # no final pass
    pr2, cd = fit_motion(dF, dM, 1, code=True)
    assert same(pr, want["params"]) and same(sm, want["sums"]) and same(pr2, want["params"]) and same(cd, want["code"])
    one = fit_motion(dF[1], dM[1], "similarity", code=True, residual=True, stats=True, sums=True)
    for a, k in zip(one, KEYS):
        assert same(a, want[k][1]), k


def test_residual_is_flow_minus_motion_flow_and_runs_repeat():
    from flowonthego_amd.motion import motion_flow
    for name in ("67x45x3", "640x420"):
        flow, mask = inputs(name)
        w, h, n = SHAPES[name]
        dF, dM = dev(flow), dev(mask)
        for model in (0, 1, 2):
            a = gpu_fit(dF, dM, model, 3)
            b = gpu_fit(dF, dM, model, 3)
            mf = motion_flow(a["params"], w, h)
            torch.cuda.synchronize()
            for k in KEYS:
                assert same(b[k], a[k].cpu().numpy()), (name, model, k)
            assert same(dF - mf, a["residual"].cpu().numpy())
            assert same(mf, np.stack([R.motion_flow(P, w, h) for P in a["params"].cpu().numpy()]))
            assert same(motion_flow(a["params"][0], w, h), mf[0].cpu().numpy())
    # into a slice one float into a larger tensor, the guards untouched
    L = _F()[0].lib()
    P = dev(np.array([[0.01, -0.02, 3.5, 0.03, 0.005, -1.25]]))
    big = torch.full((45 * 67 * 2 + 8,), -7.0, device="cuda")
    assert L.fotg_motion_flow(0, 1, p(P), 67, 45, p(big[1:]), None) == 0
    torch.cuda.synchronize()
    assert same(big[1:1 + 45 * 67 * 2].view(45, 67, 2), R.motion_flow(P[0].cpu().numpy(), 67, 45))
    assert bool((big[:1] == -7.0).all()) and bool((big[1 + 45 * 67 * 2:] == -7.0).all())


# ---- the fused form ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sc_l", [0, 1, 2, 3])
def test_fused_equals_unfused(sc_l):
    rng = np.random.default_rng(270 + sc_l)
    n = 3
    for w, h in ((97, 61), (64, 48)):
        o = make_ctx(2, w, h, max_batch=n, finest_scale=sc_l, coarsest_scale=max(sc_l, 4), use_var_ref=False)
        wl, hl = o.out_size()
        ys, xs = np.mgrid[0:hl, 0:wl].astype(np.float64) * (1 << sc_l)
        cf = np.stack([np.stack([2.5 * np.cos(k + 1.0) + 0.01 * xs - 0.02 * ys, 2.5 * np.sin(k + 1.0) + 0.015 * xs + 0.01 * ys], -1)
                       for k in range(n)])
        cf = ((cf + 0.1 * rng.standard_normal(cf.shape)) / (1 << sc_l)).astype(f32)
        cf[:, hl // 4:hl // 2, wl // 4:wl // 2] += f32(5.0 / (1 << sc_l))                  # a block moving on its own
        cf[0, hl // 2, wl // 2:wl // 2 + 4] = (np.nan, 0.0)                                # (in the middle: the crop drops the coarse border)
        cf[1, hl // 3, wl // 3:wl // 3 + 3] = (np.inf, 1.0)
        cf[2, hl // 2, wl // 4] = (5000.0 / (1 << sc_l), 0.0)
        mask = dev((rng.random((n, h, w)) < 0.2).astype(np.uint8) * rng.integers(1, 4, (n, h, w), dtype=np.uint8))
        for model in (0, 1, 2):
            for m in (None, mask):
                kw = dict(model=R.MODELS[model], code=True, residual=True, stats=True, sums=True)
                got = o.upsample_crop_fit_motion(dev(cf), m, fused=True, **kw)
                want = o.upsample_crop_fit_motion(dev(cf), m, fused=False, **kw)
                dflt = o.upsample_crop_fit_motion(dev(cf), m, **kw)
                torch.cuda.synchronize()
                for a, b, c, k in zip(got, want, dflt, KEYS):
                    assert same(a, b.cpu().numpy()) and same(c, b.cpu().numpy()), (w, h, model, m is not None, k)
                code = got[1].cpu().numpy()
                # (image 2 may end unfitted: the taps around its 5000 px vector are known, and far off any motion)
                assert all((code == c).any() for c in ((0, 1, 3) if m is None else (0, 1, 2, 3))) and bool((got[3][:2, 5] == 1).all())
        o.close()


# ---- stabilize --------------------------------------------------------------------------------------------------------------------
def test_stabilize_integer_steps_gives_the_crops_at_the_smoothed_offsets(natural_images):
    F, _ = _F()
    road = natural_images["road_HD"]
    frames, off = R.jittered_crops(road)
    T, (h, w) = len(frames) - 1, frames.shape[1:]
    flows = np.empty((T, h, w, 2), f32)
    flows[:] = (off[:-1] - off[1:])[:, None, None, :]
    smooth = np.array([off[max(k - 1, 0):k + 2].mean(0) for k in range(T + 1)])
    assert np.array_equal(smooth, np.rint(smooth)) and (smooth != off).any()
    for fr in (frames, frames.astype(f32)):
        out, code, st = F.stabilize(dev(fr), dev(flows), model="translation", radius=1, stats=True)
        out2, code2 = F.stabilize(dev(fr), dev(flows), model="translation", radius=1, fill=0)
        torch.cuda.synchronize()
        out, code, out2 = out.cpu().numpy(), code.cpu().numpy(), out2.cpu().numpy()
        assert out.dtype == fr.dtype and same(code2, code) and same(st[:, :4].sum(1), np.full(T + 1, float(h * w)))
        for k in range(T + 1):
            x, y = R.CROP_X + int(smooth[k, 0]), R.CROP_Y + int(smooth[k, 1])
            want = road[y:y + h, x:x + w].astype(fr.dtype)
            ok = code[k] == 0
            assert ok.mean() > 0.9 and np.array_equal(out[k][ok], want[ok]), k
            assert np.array_equal(out2[k][ok], want[ok]) and not out2[k][~ok].any()
            assert ok.all() == bool((smooth[k] == off[k]).all())


def test_path_algebra_equals_the_restatement():
    from flowonthego_amd.motion import smoothing_motions
    rng = np.random.default_rng(12)
    for model, T, radius in ((1, 9, 2), (2, 9, 2), (2, 5, 15), (2, 1, 0)):
        prm = rng.standard_normal((T, 6)) * np.array([0.01, 0.01, 3.0, 0.01, 0.01, 3.0])
        if model == 1:
            prm[:, 4], prm[:, 3] = prm[:, 0], -prm[:, 1]
        got = smoothing_motions(dev(prm), radius).cpu().numpy()
        want = R.smoothing_motions(prm, radius)
        assert got.shape == (T + 1, 6) and np.allclose(got, want, rtol=1e-12, atol=1e-12 * np.abs(want).max()), (model, T, radius)


# ---- OFClass ------------------------------------------------------------------------------------------------------------------------
def test_ofclass_stabilize_and_camera_motion(natural_images):
    F, _ = _F()
    frames, off = R.jittered_crops(natural_images["road_HD"])
    T, (h, w) = len(frames) - 1, frames.shape[1:]
    dfr = dev(frames)
    o = make_ctx(2, w, h, max_batch=T)
    got = o.stabilize(dfr, radius=2, stats=True)
    want = F.stabilize(dfr, o.upsample_crop(o.calc_sequence(dfr)), radius=2, stats=True)
    torch.cuda.synchronize()
    for a, b in zip(got, want):
        assert same(a, b.cpu().numpy())
    prm = o.camera_motion(dfr, model="translation").cpu().numpy()
    o.close()
    ob = make_ctx(2, w, h, max_batch=T, bidir=True)
    prm_b = ob.camera_motion(dfr, model="translation").cpu().numpy()
    aff = ob.camera_motion(dfr).cpu().numpy()
    out, code = ob.stabilize(dfr.float(), model="affine", radius=3)
    torch.cuda.synchronize()
    ob.close()
    true = (off[:-1] - off[1:]).astype(np.float64)
    for q in (prm, prm_b):
        print("worst translation error %.4f px" % np.abs(q[:, [2, 5]] - true).max())
        assert q.shape == (T, 6) and np.array_equal(np.rint(q[:, [2, 5]]), true) and not q[:, [0, 1, 3, 4]].any()
    print("worst corner error of the affine fits %.4f px" % max(R.corner_error(aff[k], [0, 0, true[k, 0], 0, 0, true[k, 1]], w, h) for k in range(T)))
    assert aff.shape == (T, 6) and np.isfinite(aff).all()
    assert out.shape == dfr.shape and out.dtype == torch.float32 and (code == 0).float().mean().item() > 0.8


# ---- arguments --------------------------------------------------------------------------------------------------------------------
def test_arguments_are_refused():
    F, OFClass = _F()
    L = F.lib()
    n, h, w = 2, 9, 11
    fl = torch.zeros((n, h, w, 2), device="cuda")
    mk = torch.zeros((n, h, w), dtype=torch.uint8, device="cuda")
    pr = torch.full((n, 6), -7.0, dtype=torch.float64, device="cuda")
    cd = torch.empty((n, h, w), dtype=torch.uint8, device="cuda")
    rs = torch.empty((n, h, w, 2), device="cuda")
    st = torch.empty((n, 6), dtype=torch.int64, device="cuda")
    sm = torch.empty((n, 12), dtype=torch.int64, device="cuda")
    fit = lambda n_=n, f=fl, m=mk, w_=w, h_=h, model=2, iters=3, th=1.0, a=pr, c=cd, r=rs, s=st, q=sm: L.fotg_fit_motion(
        0, n_, p(f), p(m), w_, h_, model, iters, C.c_float(th), p(a), p(c), p(r), p(s), p(q), None)
    assert fit() == 0 and fit(m=None, c=None, r=None, s=None, q=None) == 0 and fit(iters=0, th=0.0) == 0
    pr.fill_(-7.0)
    for bad in (dict(n_=0), dict(n_=-1), dict(n_=65536), dict(w_=0), dict(h_=-2), dict(w_=16385), dict(h_=16385), dict(f=None),
                dict(a=None), dict(model=3), dict(model=-1), dict(iters=-1), dict(iters=65), dict(th=-1.0), dict(th=float("nan")),
                dict(r=fl), dict(c=mk), dict(q=st)):
        assert fit(**bad) == FOTG_ERR_ARG, bad
    torch.cuda.synchronize()
    assert bool((pr == -7.0).all())                                                # nothing was launched: not even the clearing
    mflow = lambda n_=1, a=pr, w_=w, h_=h, f=rs: L.fotg_motion_flow(0, n_, p(a), w_, h_, p(f), None)
    assert mflow() == 0
    for bad in (dict(n_=0), dict(n_=65536), dict(a=None), dict(f=None), dict(w_=0), dict(h_=0), dict(f=pr)):
        assert mflow(**bad) == FOTG_ERR_ARG, bad
    o = make_ctx(2, 64, 48, max_batch=2)
    wl, hl = o.out_size()
    cf = torch.zeros((2, hl, wl, 2), device="cuda")
    fused = lambda ctx=o._h, n_=2, f=cf, model=1, a=pr: L.fotg_upsample_crop_fit_motion(ctx, n_, p(f), None, model, 3, C.c_float(1.0), p(a),
                                                                                         None, None, None, None, None)
    assert fused() == 0 and fused(n_=1) == 0
    for bad in (dict(ctx=None), dict(n_=3), dict(n_=0), dict(f=None), dict(a=None), dict(model=5)):
        assert fused(**bad) == FOTG_ERR_ARG, bad
    op = F.operating_point(2, 64, 1)
    op.depth_mode = True
    od = OFClass(op, F.img_params(width=64, height=48), max_batch=2)
    assert fused(ctx=od._h) == FOTG_ERR_ARG
    with pytest.raises(F.FotgError):
        od.upsample_crop_fit_motion(cf)
    for call in (lambda: F.fit_motion(fl, model="projective"), lambda: F.fit_motion(fl, iters=-1), lambda: F.fit_motion(fl, thresh=-1.0),
                 lambda: F.fit_motion(fl, mk[:1]), lambda: F.fit_motion(fl.cpu()), lambda: F.motion_flow(pr.float(), w, h),
                 lambda: F.stabilize(fl[..., 0], fl), lambda: F.smoothing_motions(pr, -1)):
        with pytest.raises(F.FotgError):
            call()
    assert fit() == 0 and fused() == 0                                             # a valid call afterwards succeeds
    torch.cuda.synchronize()
    o.close()
    od.close()
