"""GPU tests of the motion layers (fotg_motion_layers / fotg_upsample_crop_motion_layers, flowonthego_amd.layers) against the numpy
restatement tests/layers_ref.py, byte for byte: params (as uint64), labels, residual, records, stats and sums, over batches whose
images differ (the three-motion scene, a scene with NaNs, infinities, +-4096 and a mask of every code, an all-masked image), every
layer count, model, seeding and refinement depth, threshold, with and without init; the seed-tile tie, a uniform flow and a
checkerboard; the fused form, single against batched calls, repeated runs, the refusals, OFClass.motion_layers and the
compositions with the existing functions.  (A NaN of the residual -- the residual of a NaN vector -- is compared as a NaN,
whatever its payload, as in test_gpu_motion.)"""
import ctypes as C

import numpy as np
import pytest
import torch

import layers_ref as LR
import motion_ref as R
from host_checks import read_png_rgb, run_cli
from test_gpu_warp import dev, make_ctx, np_same_bits, same_bits

pytestmark = pytest.mark.gpu

FOTG_ERR_ARG = 1
f32 = np.float32
KEYS = ("params", "labels", "residual", "records", "stats", "sums")
ALL = dict(labels=True, residual=True, records=True, stats=True, sums=True)


def _F():
    import flowonthego_amd as F
    from flowonthego_amd.oflow import OFClass
    return F, OFClass


def p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def same(got, want, key):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    if key == "params":
        return got.shape == want.shape and got.dtype == np.float64 and np.array_equal(got.view(np.uint64), want.view(np.uint64))
    if key == "residual":
        nan = np.isnan(want)
        return np.array_equal(np.isnan(got), nan) and np_same_bits(np.where(nan, f32(0), got), np.where(nan, f32(0), want))
    return np_same_bits(got, want)


def check(got, want, what):
    for g, k in zip(got, KEYS):
        assert same(g, want[k], k), (what, k)


def batch(w, h):
    """three images of different content: the three-motion scene, make_scene's specials under a mask of every code, an all-masked image"""
    a = LR.three_motions(w, h, seed=3)[0]
    b, mb, _ = R.make_scene(w, h, seed=4, specials=True)
    c = R.make_scene(w, h, seed=5, specials=False)[0]
    return np.stack([a, b, c]), np.stack([np.zeros((h, w), np.uint8), mb, np.full((h, w), 2, np.uint8)])


SHAPES = [(1, 1), (5, 3), (61, 23), (157, 93)]
ROUNDS = [(0, 0), (0, 3), (3, 0), (3, 3)]
THRESH = [0.0, 1.0, 2.5]


@pytest.mark.parametrize("w,h", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_gpu_equals_the_restatement(w, h):
    F, _ = _F()
    flow, mask = batch(w, h)
    dflow, dmask = dev(flow), dev(mask)
    i = 0
    for K in (1, 2, 3, 5, 8):
        for model in (0, 1, 2):
            for iters, rounds in ROUNDS:                          # every K with every model and every depth; the thresholds in turn
                thresh = THRESH[i % 3]
                i += 1
                kw = dict(layers=K, model=model, iters=iters, rounds=rounds, thresh=thresh)
                got = F.motion_layers(dflow, dmask, **dict(kw, model=R.MODELS[model]), **ALL)
                check(got, LR.layers_batch(flow, mask, **kw), (w, h, kw))
    # without a mask, the defaults: the scene's three layers
    got = F.motion_layers(dflow[0], **ALL)
    want = LR.layers(flow[0])
    check(got, want, (w, h, "defaults"))
    if w * h >= 61 * 23:
        assert want["stats"][3] == 3 and (want["records"][:, 0] > 0).all()


@pytest.mark.parametrize("w,h", [(61, 23), (157, 93)], ids=["61x23", "157x93"])
def test_init_layers(w, h):
    F, _ = _F()
    flow, mask = batch(w, h)
    Ps = np.array([LR.P_BACKGROUND, LR.P_A, LR.P_B])
    bad = np.array([np.nan, 0.0, 1.0, 0.0, np.inf, -1.0])
    for K, pick in ((2, [0, 0]), (3, [2, 0, 1]), (5, [0, 1, 1, -1, 2]), (8, [1, -1, 0, 0, 2, 2, 1, 0])):
        init = np.stack([np.stack([bad if j < 0 else Ps[j] * (1.0 + 0.01 * i) for j in pick]) for i in range(3)])
        for model, iters, rounds, thresh in ((2, 3, 0, 1.0), (2, 0, 3, 1.0), (1, 1, 2, 2.5), (0, 0, 1, 0.0)):
            kw = dict(layers=K, model=model, iters=iters, rounds=rounds, thresh=thresh)
            got = F.motion_layers(dev(flow), dev(mask), init=dev(init), **dict(kw, model=R.MODELS[model]), **ALL)
            want = LR.layers_batch(flow, mask, init=init, **kw)
            check(got, want, (w, h, kw))
            assert (want["records"][:, :, 4] == -2).all()
            if rounds == 0:
                assert same(got[0], init, "params")
    # one image, init (K, 6): the twin of layer 0 holds no pixel
    init = np.stack([Ps[0], Ps[0], Ps[1]])
    prm, lab, rec = F.motion_layers(dev(flow[0]), init=dev(init), rounds=0, labels=True, records=True)
    assert prm.shape == (3, 6) and same(prm, init, "params") and int(rec[1, 0]) == 0 and not bool((lab == 1).any()) and int(rec[0, 0]) > 0


def test_seed_tile_tie_uniform_flow_and_checkerboard():
    F, _ = _F()
    # two tiles, each fully covered by a translation of its own: the mean motion of layer 0 holds no pixel and dies, both tiles
    # hold 1024 candidates, the lower index wins
    two = np.empty((32, 64, 2), f32)
    two[:, :32], two[:, 32:] = (3.0, 1.0), (-2.0, 4.0)
    got = F.motion_layers(dev(two), layers=3, model="translation", **ALL)
    want = LR.layers(two, layers=3, model=0)
    check(got, want, "two tiles")
    assert want["records"][:, 2].tolist() == [0, 1, 1] and want["records"][:, 4].tolist() == [-1, 0, 1]
    assert want["params"][1, [2, 5]].tolist() == [3.0, 1.0] and want["params"][2, [2, 5]].tolist() == [-2.0, 4.0]
    assert want["records"][1:, 0].tolist() == [1024, 1024]
    # a uniform flow: one layer takes everything, every lane of every wave adds to it
    uni = np.empty((2, 45, 77, 2), f32)
    uni[0], uni[1] = (1.25, -0.5), (-3.0, 2.0)
    for K in (1, 4):
        want = LR.layers_batch(uni, layers=K)
        check(F.motion_layers(dev(uni), layers=K, **ALL), want, ("uniform", K))
        assert (want["records"][:, 0, 0] == 45 * 77).all() and (want["stats"][:, 3] == 1).all()
    # a checkerboard of 4 x 4 squares of two translations: every wave holds both layers
    ys, xs = np.mgrid[0:48, 0:64]
    sq = ((ys // 4 + xs // 4) % 2).astype(bool)
    board = np.where(sq[..., None], np.array([2.0, 0.0], f32), np.array([-1.0, 3.0], f32)).astype(f32)
    init = np.array([[0, 0, 2.0, 0, 0, 0.0], [0, 0, -1.0, 0, 0, 3.0]])
    for kw in (dict(init=init, model=0), dict(init=init, model=2), dict(model=0)):
        want = LR.layers(board, layers=2, **kw)
        check(F.motion_layers(dev(board), layers=2, **dict(kw, model=R.MODELS[kw["model"]], init=None if "init" not in kw else dev(init)), **ALL),
              want, ("checkerboard", sorted(kw)))
    want = LR.layers(board, layers=2, init=init, model=0)
    assert np.array_equal(want["labels"], (~sq).astype(np.uint8)) and want["records"][:, 0].tolist() == [sq.sum(), (~sq).sum()]


def test_single_against_batched_and_repeated_runs():
    F, _ = _F()
    flow, mask = batch(61, 23)
    dflow, dmask = dev(flow), dev(mask)
    kw = dict(layers=3, model="similarity", iters=2, rounds=2, thresh=1.5, **ALL)
    a = F.motion_layers(dflow, dmask, **kw)
    b = F.motion_layers(dflow, dmask, **kw)
    for x, y in zip(a, b):
        assert same_bits(x, y)
    for i in range(3):
        one = F.motion_layers(dflow[i], dmask[i], **kw)
        for x, y in zip(a, one):
            assert same_bits(x[i], y), i
    # the outputs that are not asked for change nothing, and params alone comes back as a tensor
    prm = F.motion_layers(dflow, dmask, layers=3, model="similarity", iters=2, rounds=2, thresh=1.5)
    assert isinstance(prm, torch.Tensor) and same_bits(prm, a[0])
    prm, st = F.motion_layers(dflow, dmask, layers=3, model="similarity", iters=2, rounds=2, thresh=1.5, stats=True)
    assert same_bits(prm, a[0]) and same_bits(st, a[4])
    # layer 0 is the global-motion fit
    assert same_bits(F.motion_layers(dflow, dmask, layers=2, rounds=0)[:, 0].contiguous(), F.fit_motion(dflow, dmask))


def test_fused_equals_dense():
    for sc_l, (w, h) in ((1, (97, 61)), (2, (64, 48))):
        rng = np.random.default_rng(40 + sc_l)
        n = 2
        o = make_ctx(2, w, h, max_batch=n, finest_scale=sc_l, coarsest_scale=max(sc_l, 4), use_var_ref=False)
        wl, hl = o.out_size()
        ys, xs = np.mgrid[0:hl, 0:wl].astype(np.float64) * (1 << sc_l)
        cf = np.stack([np.stack([2.5 * np.cos(k + 1.0) + 0.01 * xs - 0.02 * ys, 2.5 * np.sin(k + 1.0) + 0.015 * xs + 0.01 * ys], -1) for k in range(n)])
        cf = ((cf + 0.1 * rng.standard_normal(cf.shape)) / (1 << sc_l)).astype(f32)
        cf[:, hl // 4:hl // 2, wl // 4:wl // 2] += f32(5.0 / (1 << sc_l))                  # a block moving on its own
        cf[0, hl // 2, wl // 2:wl // 2 + 4] = (np.nan, 0.0)
        cf[1, hl // 3, wl // 3:wl // 3 + 3] = (np.inf, 1.0)
        mask = dev((rng.random((n, h, w)) < 0.2).astype(np.uint8) * rng.integers(1, 4, (n, h, w), dtype=np.uint8))
        dcf = dev(cf)
        full = o.upsample_crop(dcf)
        for m in (None, mask):
            for K, model in ((2, "affine"), (4, "translation")):
                want = _F()[0].motion_layers(full, m, layers=K, model=model, **ALL)
                ref = LR.layers_batch(full.cpu().numpy(), None if m is None else m.cpu().numpy(), layers=K, model=R.MODELS.index(model))
                check(want, ref, (sc_l, K, model))
                for kw in (dict(fused=True), dict(fused=False), dict()):
                    got = o.upsample_crop_motion_layers(dcf, m, layers=K, model=model, **ALL, **kw)
                    for a, b, k in zip(got, want, KEYS):
                        assert same(a, b.cpu().numpy(), k), (sc_l, K, model, kw, k)
                assert int(want[4][:, 3].min()) >= 2                                       # the block is a layer of its own
        o.close()


def test_refusals_launch_nothing():
    F, OFClass = _F()
    L = F.lib()
    n, h, w, K = 2, 9, 11, 3
    fl = torch.zeros((n, h, w, 2), device="cuda")
    mk = torch.zeros((n, h, w), dtype=torch.uint8, device="cuda")
    ini = torch.zeros((n, K, 6), dtype=torch.float64, device="cuda")
    pr = torch.full((n, K, 6), -7.0, dtype=torch.float64, device="cuda")
    lb = torch.full((n, h, w), 77, dtype=torch.uint8, device="cuda")
    rs = torch.full((n, h, w, 2), -7.0, device="cuda")
    rc = torch.full((n, K, 8), -7, dtype=torch.int64, device="cuda")
    st = torch.full((n, 4), -7, dtype=torch.int64, device="cuda")
    sm = torch.full((n, K, 12), -7, dtype=torch.int64, device="cuda")
    call = lambda n_=n, f=fl, m=mk, w_=w, h_=h, K_=K, model=2, iters=3, rounds=3, th=1.0, i=None, a=pr, l=lb, r=rs, c=rc, s=st, q=sm: \
        L.fotg_motion_layers(0, n_, p(f), p(m), w_, h_, K_, model, iters, rounds, C.c_float(th), p(i), p(a), p(l), p(r), p(c), p(s), p(q), None)
    for bad in (dict(n_=0), dict(w_=0), dict(h_=16385), dict(K_=0), dict(K_=9), dict(model=3), dict(iters=65), dict(rounds=-1), dict(th=-1.0),
                dict(th=float("nan")), dict(f=None), dict(a=None),
                dict(r=fl), dict(l=mk), dict(a=ini, i=ini), dict(c=ini, i=ini), dict(q=pr), dict(s=rc), dict(c=sm), dict(l=rs)):
        assert call(**bad) == FOTG_ERR_ARG, bad
    torch.cuda.synchronize()
    for t, v in ((pr, -7.0), (lb, 77), (rs, -7.0), (rc, -7), (st, -7), (sm, -7)):
        assert bool((t == v).all())                                                  # nothing was launched: not even the clearing
    assert call() == 0 and call(m=None, l=None, r=None, c=None, s=None, q=None) == 0 and call(i=ini, iters=0, rounds=0, th=0.0) == 0
    o = make_ctx(2, 64, 48, max_batch=2)
    wl, hl = o.out_size()
    cf = torch.zeros((2, hl, wl, 2), device="cuda")
    big = torch.empty((2, 8, 6), dtype=torch.float64, device="cuda")
    fused = lambda ctx=o._h, n_=2, f=cf, K_=3, a=big: L.fotg_upsample_crop_motion_layers(ctx, n_, p(f), None, K_, 1, 3, 3, C.c_float(1.0), None, p(a),
                                                                                      None, None, None, None, None, None)
    assert fused() == 0 and fused(n_=1) == 0
    for bad in (dict(ctx=None), dict(n_=3), dict(n_=0), dict(f=None), dict(a=None), dict(K_=9)):
        assert fused(**bad) == FOTG_ERR_ARG, bad
    for bad in (lambda: F.motion_layers(fl, layers=9), lambda: F.motion_layers(fl, rounds=-1), lambda: F.motion_layers(fl, mk[:1]),
                lambda: F.motion_layers(fl, init=ini[:, :2]), lambda: F.motion_layers(fl, init=ini.float()), lambda: F.motion_layers(fl.cpu()),
                lambda: o.upsample_crop_motion_layers(cf[:, 1:], fused=True), lambda: o.upsample_crop_motion_layers(cf, layers=0, fused=True)):
        with pytest.raises(F.FotgError):
            bad()
    torch.cuda.synchronize()
    o.close()


def test_ofclass_motion_layers_is_its_composition(natural_images):
    F, _ = _F()
    frames, off = R.jittered_crops(natural_images["road_HD"], T=3, patch=True)
    T, (h, w) = len(frames) - 1, frames.shape[1:]
    dfr = dev(frames)
    for bidir in (False, True):
        o = make_ctx(2, w, h, max_batch=T, bidir=bidir)
        got = o.motion_layers(dfr, layers=2, model="translation", **ALL)
        if bidir:
            fw, bw = o.calc_sequence_bidirectional(dfr)
            m = o.upsample_crop_fb_check(fw, bw)[0]
        else:
            fw, m = o.calc_sequence(dfr), None
        want = F.motion_layers(o.upsample_crop(fw), m, layers=2, model="translation", **ALL)
        torch.cuda.synchronize()
        for a, b in zip(got, want):
            assert same_bits(a, b)
        seeded = o.motion_layers(dfr, layers=2, model="translation", rounds=0)
        assert got[0].shape == (T, 2, 6) and same_bits(seeded[:, 0].contiguous(), o.camera_motion(dfr, model="translation"))   # layer 0 starts as the camera
        o.close()


def test_outputs_go_into_the_existing_functions():
    F, _ = _F()
    w, h = 157, 93
    flow = LR.three_motions(w, h, seed=3)[0]
    dflow = dev(np.stack([flow, flow]))
    params, labels, records = F.motion_layers(dflow, layers=3, labels=True, records=True)
    objects = F.label_components(labels, fg=(1,))
    assert objects.shape == (2, 256, 11) and int(objects[0, :, 1].sum()) == int(records[0, 1, 0]) > 0     # the pieces of layer 1 are layer 1
    cells = F.motion_histograms(dflow, motion=params[:, 1].contiguous(), cell=16)
    assert cells.shape == (2, (h + 15) // 16, (w + 15) // 16, 32)
    frames = dev((np.arange(2 * h * w, dtype=np.float32) % 251).reshape(2, h, w))
    motions = torch.stack([torch.zeros(6, dtype=torch.float64, device="cuda"), params[0, 0]])   # frame 0 -> frame 0, frame 0 -> frame 1: the camera layer
    exclude = torch.stack([(labels[0] != 0).to(torch.uint8), torch.zeros_like(labels[0])])
    plate = F.background_plate(frames, motions=motions, exclude=exclude)
    assert plate.shape == (1, h, w)
    s = F.layer_summary(records, w, h).cpu().numpy()
    assert s.shape == (2, 3, 3) and np.isfinite(s).all() and abs(s[0, 2, 2] - 6.5) < 0.1      # layer 2 is the object moving by (6.5, -4)
    mf = F.motion_flow(params[0], w, h)
    assert mf.shape == (3, h, w, 2)


def test_cli_writes_what_the_call_returns(tmp_path):
    F, _ = _F()
    from flowonthego_amd.flo import write_flo
    from flowonthego_amd.motion_layers import palette
    from host_checks import gray_png_bytes
    w, h = 157, 93
    flow = LR.three_motions(w, h, seed=8)[0]
    flow[3, 7] = (np.nan, 0)
    mask = (np.random.default_rng(2).random((h, w)) < 0.05).astype(np.uint8) * 3
    fl, mk, out, prm = (str(tmp_path / n) for n in ("f.flo", "m.png", "out.png", "p.npy"))
    write_flo(fl, flow)
    open(mk, "wb").write(gray_png_bytes(mask))
    run = run_cli("motion_layers", [fl, out, "--layers", "4", "--model", "affine", "--mask", mk, "--params", prm])
    assert run.returncode == 0, run.stderr
    params, labels, records, st = F.motion_layers(dev(flow), dev(mask), 4, "affine", labels=True, records=True, stats=True)
    want = LR.layers(flow, mask, layers=4)
    assert same(params, want["params"], "params") and same(labels, want["labels"], "labels")
    assert np.array_equal(np.load(prm).view(np.uint64), want["params"].view(np.uint64))
    assert np.array_equal(read_png_rgb(out), np.asarray(palette(), np.uint8)[want["labels"]])
    lines = run.stdout.splitlines()
    assert len(lines) == 5 and lines[3].endswith("dead") and lines[0].startswith("layer 0: " + " ".join("%.9g" % v for v in want["params"][0]))
    assert lines[4] == "  ".join("%s %.4f" % (nm, c / (h * w)) for nm, c in zip(F.LAYER_STATS[:3], want["stats"][:3]))
    assert set(np.unique(want["labels"]).tolist()) >= {0, 1, 2, 254, 255}
