"""GPU tests of the motion histograms (fotg_motion_histograms / fotg_upsample_crop_motion_histograms, flowonthego_amd.histograms,
OFClass.motion_histograms).

The definition is integer arithmetic after the residual, so every output equals the numpy restatement (tests/histograms_ref.py) byte
for byte, and the fused form equals the dense one on fotg_upsample_crop's output bit for bit.  No tolerance appears anywhere; every
call is made twice and the bytes compared.

The sizes are the smallest at which the kernel's paths differ (a workgroup owns a tile of 64 x 32 pixels, a thread stages eight
adjacent pixels of a row, a lane then owns eight pixels of a column): 1 x 1, 5 x 3 (narrower than a thread's pixels), 19 x 67 (a width
that is no multiple of four: every row starts at another alignment; partial edge cells; two tiles across), 40 x 130 (two cell rows at
cell 32, two tiles down, more than two across)."""
import ctypes as C

import numpy as np
import pytest
import torch

import histograms_ref as R
from test_gpu_warp import dev, make_ctx, same_bits

pytestmark = pytest.mark.gpu

FOTG_ERR_ARG = 1
SIZES = ((1, 1), (5, 3), (19, 67), (40, 130))          # (h, w)
K, N = 16, 3
_SCENES, _WANT = {}, {}


def scene(h, w, n=N):
    """flow (n, h, w, 2), mask (n, h, w), params (n, 6), ids (n, h, w) of a case, computed once (nobody writes to them): random vectors
    in multiples of 1/512 pixel (so 256 u has fractions exactly at .5); vectors exactly on the axes and the diagonals; magnitudes
    exactly at and one below the threshold; NaN, infinities, +-5000 and exactly +-4096; image 1's parameters push a residual past
    4096; image 2's parameters hold a NaN; a mask with every code; ids from -3 to K + 3"""
    key = (h, w, n)
    if key in _SCENES:
        return _SCENES[key]
    rng = np.random.default_rng(1000 * h + w)
    flow = (rng.integers(-2048, 2049, (n, h, w, 2)) / 512.0).astype(np.float32)
    flow[:, h // 2:, :, :] *= np.float32(0.0625)          # a quieter half: many vectors below the threshold
    special = [(3, 0), (0, 3), (-3, 0), (0, -3), (2, 2), (-2, 2), (-2, -2), (2, -2), (102 / 256, 0), (101 / 256, 0), (0, -102 / 256),
               (0, 101 / 256), (0, 0), (np.nan, 0), (0, np.nan), (np.inf, 1), (1, -np.inf), (5000, 0), (0, -5000), (-5000, 5000), (4096, 0),
               (0, -4096), (4096, 4096), (-4096, 4096), (3e38, 0)]
    px = rng.permutation(h * w)
    for i in range(n):
        for s, p in zip(special, np.roll(px, 7 * i)[:len(special)]):
            flow[i, p // w, p % w] = s
    mask = rng.choice(np.array([0, 0, 0, 0, 0, 0, 0, 1, 2, 3, 200], np.uint8), (n, h, w))
    params = np.array([[0.004, -0.011, 1.75, 0.009, 0.006, -2.5], [0.0, 0.0, -1.0, 0.0, 0.0, 1.0], [0.001, 0.0, np.nan, 0.0, 0.0, 0.5]])[:n]
    ids = np.full((n, h, w), -1, np.int32)
    for i in range(n):
        for _ in range(2 + (h * w) // 120):
            bh, bw = rng.integers(1, max(2, h // 2 + 1)), rng.integers(1, max(2, w // 3 + 1))
            y, x = rng.integers(0, h), rng.integers(0, w)
            ids[i, y:y + bh, x:x + bw] = rng.integers(-3, K + 4)
        if h * w > 4:
            ids[i, 0, 0], ids[i, h - 1, w - 1] = -3, K + 2
    _SCENES[key] = (flow, mask, params, ids)
    return _SCENES[key]


def want(h, w, cell, masked, moved, thresh256=R.THRESH256, rows=K):
    key = (h, w, cell, masked, moved, thresh256, rows)
    if key not in _WANT:
        flow, mask, params, ids = scene(h, w)
        _WANT[key] = R.histograms(flow, mask if masked else None, params if moved else None, cell, thresh256, ids, rows)
    return _WANT[key]


def assert_equal(got, want_, what):
    got = [g.cpu().numpy() for g in got]
    assert len(got) == len(want_)
    for k, (g, w_) in enumerate(zip(got, want_)):
        assert g.dtype == w_.dtype and g.shape == w_.shape, (what, k, g.dtype, g.shape, w_.dtype, w_.shape)
        assert np.array_equal(g, w_), (what, k, np.argwhere(g != w_)[:5].tolist())


def twice(fn):
    """two identical calls give identical bytes"""
    a, b = fn(), fn()
    a, b = (a if isinstance(a, tuple) else (a,)), (b if isinstance(b, tuple) else (b,))
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert same_bits(x, y)
    return a


# ---- the dense form -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", R.CELLS)
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("moved", [False, True])
def test_dense_equals_the_restatement(cell, masked, moved):
    from flowonthego_amd.histograms import motion_histograms
    for h, w in SIZES:
        flow, mask, params, ids = (dev(t) for t in scene(h, w))
        m, p = (mask if masked else None), (params if moved else None)
        wc, wo = want(h, w, cell, masked, moved)
        assert_equal(twice(lambda: motion_histograms(flow, m, p, cell, ids=ids, rows=K)), (wc, wo), (h, w, "both"))
        assert_equal(twice(lambda: motion_histograms(flow, m, p, cell)), (wc,), (h, w, "cells"))
        assert_equal(twice(lambda: motion_histograms(flow, m, p, cell, ids=ids, rows=K, cells=False)), (wo,), (h, w, "objects"))
        assert (wc[..., R.N] + wc[..., R.NBAD]).sum() == N * h * w and not wc[..., 31].any() and not wo[..., 31].any()


def test_every_branch_is_populated():
    for h, w in SIZES[2:]:
        flow, mask, params, ids = scene(h, w)
        for masked in (False, True):
            c, o = want(h, w, 16, masked, False)
            tot = c.sum((0, 1, 2))
            assert (tot[0:8] > 0).all() and tot[R.ZERO] > 0 and (tot[9:25] > 0).all(), tot
            assert tot[R.NBAD] >= 3 * 8 and 0 < tot[R.NMBH] < tot[R.N] and tot[R.SU] != 0 and tot[R.SV] != 0
            assert (o.sum((0, 2)) > 0).sum() >= 4 and o[..., R.NBAD].sum() > 0       # several objects, some with inadmissible pixels
        plain, moved = [R.fixed(flow[1], None, P)[0] for P in (None, params[1])]
        assert (plain & ~moved).any()                       # known vectors whose residual is not
        cm, _ = want(h, w, 16, False, True)
        assert cm[2, ..., R.N].sum() == 0 and cm[2, ..., R.NBAD].sum() == h * w and cm[0, ..., R.N].sum() > 0     # the NaN parameter row
        adm0, U, V = R.fixed(flow[0])
        m = R.mag(U, V)
        assert (adm0 & (m == R.THRESH256)).any() and (adm0 & (m == R.THRESH256 - 1)).any() and (adm0 & (m == 0)).any()
        assert (adm0 & (np.abs(U) == 1 << 20)).any()        # exactly 4096 is admissible
        assert sorted(set(np.unique(mask))) == [0, 1, 2, 3, 200] and ids.min() < -1 and ids.max() >= K


def test_thresholds_and_a_single_image():
    from flowonthego_amd.histograms import motion_histograms
    h, w = 19, 67
    flow, mask, params, ids = scene(h, w)
    for t256 in (0, 1, 512):
        got = twice(lambda: motion_histograms(dev(flow), dev(mask), dev(params), 8, t256 / 256.0, dev(ids), K))
        assert_equal(got, want(h, w, 8, True, True, t256), t256)
    assert want(h, w, 8, True, True, 0)[0][..., R.ZERO].sum() == 0
    one = motion_histograms(dev(flow[1]), dev(mask[1]), dev(params[1]), 16, ids=dev(ids[1]), rows=K)
    assert_equal(one, [t[1] for t in want(h, w, 16, True, True)], "single")


def test_unaligned_pointers_take_the_scalar_path():
    """views that start 8 bytes (flow), 1 byte (mask) and 4 bytes (ids) into an allocation"""
    from flowonthego_amd.histograms import motion_histograms
    h, w = 40, 130
    flow, mask, params, ids = scene(h, w)
    shift = lambda t, per: torch.cat([t.flatten()[:per], t.flatten()])[per:].view(t.shape)
    df, dm, di = shift(dev(flow), 2), shift(dev(mask), 1), shift(dev(ids), 1)
    assert df.data_ptr() % 16 == 8 and dm.data_ptr() % 4 == 1 and di.data_ptr() % 16 == 4 and df.is_contiguous()
    for args in ((df, dev(mask), dev(ids)), (dev(flow), dm, dev(ids)), (dev(flow), dev(mask), di)):
        got = twice(lambda: motion_histograms(args[0], args[1], dev(params), 16, ids=args[2], rows=K))
        assert_equal(got, want(h, w, 16, True, True), "unaligned")


# ---- the worst cases for the counters ---------------------------------------------------------------------------------------------
def test_largest_sums():
    """a uniform flow puts every lane on the same two bins; (4096, 4096) everywhere is the largest HOF, signs that flip every two
    columns and every two rows the largest MBH; one object over 40 x 130 passes 2^32"""
    from flowonthego_amd.histograms import motion_histograms
    h, w = 40, 130
    ys, xs = np.mgrid[0:h, 0:w]
    uniform = np.full((h, w, 2), 4096.0, np.float32)
    sx, sy = 1 - 2 * ((xs // 2) % 2), 1 - 2 * ((ys // 2) % 2)
    pairs = np.stack([4096.0 * sx * sy, -4096.0 * sx * sy], -1).astype(np.float32)
    columns = np.stack([4096.0 * (1 - 2 * (xs % 2)), 4096.0 * (1 - 2 * (xs % 2))], -1).astype(np.float32)
    flow = np.stack([uniform, pairs, columns])
    ids = np.zeros((3, h, w), np.int32)
    for cell in R.CELLS:
        wc, wo = R.histograms(flow, None, None, cell, ids=ids, rows=2)
        got = twice(lambda: motion_histograms(dev(flow), None, None, cell, ids=dev(ids), rows=2))
        assert_equal(got, (wc, wo), cell)
    big = R.mag1(1 << 21, 1 << 21)
    assert wc[0, 0, 0, 1] == 1024 * R.mag1(1 << 20, 1 << 20) and wc[0, 0, 0, :8].sum() == wc[0, 0, 0, 1]       # 45 degrees: bin 1 alone
    # a cell of 32 x 32 at the top border: 31 rows of the largest gradient, and the border row, where the difference down the column is 0
    assert wc[1, 0, 1, 9:17].sum() == 992 * big + 32 * (1 << 21) > 1 << 31 and wc[1, 0, 1, 17:25].sum() == wc[1, 0, 1, 9:17].sum()
    assert wo[0, 0, R.SM] == h * w * R.mag1(1 << 20, 1 << 20) > 1 << 32 and wo[1, 0, 9:17].sum() > 1 << 32
    assert wo[0, 0, R.SU] == h * w << 20 and wo[2, 0, R.SU] == 0 and not wo[:, 1].any()
    neg = -flow[:1]
    got = twice(lambda: motion_histograms(dev(neg), None, None, 32, ids=dev(ids[:1]), rows=1))
    assert_equal(got, R.histograms(neg, None, None, 32, ids=ids[:1], rows=1), "negative")
    assert int(got[1][0, 0, R.SU]) == -(h * w << 20) and int(got[0][0, 0, 0, R.SV]) == -(1024 << 20)


# ---- object rows ------------------------------------------------------------------------------------------------------------------
def test_object_rows_and_guard_rows():
    from flowonthego_amd.histograms import motion_histograms
    import flowonthego_amd as F
    L = F.lib()
    h, w = 19, 67
    flow, mask, params, ids = scene(h, w)
    assert ids.max() >= 3
    for rows in (1, 2, 5, 1024):
        got = twice(lambda: motion_histograms(dev(flow), dev(mask), dev(params), 16, ids=dev(ids), rows=rows, cells=False))
        assert_equal(got, (want(h, w, 16, True, True, rows=rows)[1],), rows)
    wild = ids.copy()
    wild[ids == 1] = 1 << 30
    wild[ids == 2] = -(1 << 31)
    wild[ids == 3] = -2
    wc, wo = R.histograms(flow, mask, params, 8, ids=wild, rows=K)
    assert not wo[:, 1:4].any() and wo[:, 0].any()
    # the outputs sit between guard rows of a sentinel: nothing is written outside them
    _p = lambda t: C.c_void_p(t.data_ptr())
    gh, gw = -(-h // 8), -(-w // 8)
    cells = torch.full((N * gh * gw + 2, 32), -7, dtype=torch.int64, device="cuda")
    objs = torch.full((N * K + 2, 32), -7, dtype=torch.int64, device="cuda")
    d = [dev(t) for t in (flow, mask, params, wild)]
    for _ in range(2):
        assert L.fotg_motion_histograms(0, N, _p(d[0]), w, h, _p(d[1]), _p(d[2]), 8, R.THRESH256, _p(cells[1:]), _p(d[3]), K, _p(objs[1:]), None) == 0
        torch.cuda.synchronize()
        assert np.array_equal(cells[1:-1].cpu().numpy().reshape(wc.shape), wc) and np.array_equal(objs[1:-1].cpu().numpy().reshape(wo.shape), wo)
        for t in (cells, objs):
            assert bool((t[0] == -7).all()) and bool((t[-1] == -7).all())


# ---- the fused form ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sc_l", [1, 2])
def test_fused_equals_dense_on_upsample_crop(sc_l):
    from flowonthego_amd.histograms import motion_histograms
    rng = np.random.default_rng(40 + sc_l)
    n = N
    for w, h in ((97, 61), (64, 48)):
        o = make_ctx(2, w, h, max_batch=n, finest_scale=sc_l, coarsest_scale=max(sc_l, 4), use_var_ref=False)
        wl, hl = o.out_size()
        assert wl < w and hl < h
        cf = (rng.standard_normal((n, hl, wl, 2)) * 2.5 / (1 << sc_l)).astype(np.float32)
        cf[0, hl // 2, wl // 2:wl // 2 + 3] = (np.nan, 0.0)
        cf[1, hl // 3, wl // 3:wl // 3 + 2] = (np.inf, 1.0)
        cf[2, hl // 2, wl // 4] = (5000.0 / (1 << sc_l), 0.0)
        cf = dev(cf)
        mask = dev(rng.choice(np.array([0, 0, 0, 0, 1, 2, 3], np.uint8), (n, h, w)))
        ids = dev(rng.integers(-1, 4, (n, h // 8 + 1, w // 8 + 1)).astype(np.int32).repeat(8, 1).repeat(8, 2)[:, :h, :w])
        params = dev(np.array([[0.004, -0.011, 1.75, 0.009, 0.006, -2.5]] * n))
        dense = o.upsample_crop(cf)
        for m, p, i in ((None, None, None), (mask, params, ids), (mask, None, ids)):
            for cell in (8, 32):
                got = twice(lambda: o.upsample_crop_motion_histograms(cf, m, p, cell, ids=i, rows=4))
                unf = o.upsample_crop_motion_histograms(cf, m, p, cell, ids=i, rows=4, fused=False)
                ref = motion_histograms(dense, m, p, cell, ids=i, rows=4)
                torch.cuda.synchronize()
                for a, b, c in zip(got, unf if isinstance(unf, tuple) else (unf,), ref if isinstance(ref, tuple) else (ref,)):
                    assert same_bits(a, b) and same_bits(a, c), (w, h, cell)
                assert bool((got[0][..., R.NBAD].sum() > 0)) and bool((got[0][..., R.N].sum() > 0))
        o.close()


# ---- the whole thing in one call --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bidir", [False, True])
def test_ofclass_motion_histograms_is_the_documented_composition(bidir, natural_images):
    import flowonthego_amd as F
    import motion_ref as M
    from flowonthego_amd.motion import _sequence_flows
    frames, _ = M.jittered_crops(natural_images["road_HD"], T=3, patch=True)
    T, (h, w) = len(frames) - 1, frames.shape[1:]
    dfr = dev(frames)
    o = make_ctx(2, w, h, max_batch=T, bidir=bidir)
    got = o.motion_histograms(dfr, cell=16, model="affine", occlusion=bidir, objects=True, min_area=16, max_objects=32)
    fw, mask = _sequence_flows(o, dfr)
    params, code, res = o.upsample_crop_fit_motion(fw, mask, code=True, residual=True)
    objects, ids = F.label_components(code, (1,), 8, res, 16, 32, ids=True)
    cells, rows = F.motion_histograms(o.upsample_crop(fw), mask, params, 16, 0.4, ids, 32)
    torch.cuda.synchronize()
    assert len(got) == 5 and got[1].shape == (T, -(-h // 16), -(-w // 16), 32) and got[2].shape == (T, 32, 32)
    for g, w_ in zip(got, (params, cells, rows, objects, ids)):
        assert same_bits(g, w_)
    assert bool(got[1][..., R.N].sum() > 0) and bool(got[2][..., R.N].sum() > 0)
    # without a model nothing is subtracted; without objects only the cells come back
    plain = o.motion_histograms(dfr, cell=32, model=None)
    assert plain[0] is None and len(plain) == 2 and same_bits(plain[1], F.motion_histograms(o.upsample_crop(fw), None, None, 32))
    with pytest.raises(F.FotgError):
        o.motion_histograms(dfr, model=None, objects=True)
    if not bidir:
        with pytest.raises(F.FotgError):
            o.motion_histograms(dfr, occlusion=True)
    o.close()


# ---- errors and streams -----------------------------------------------------------------------------------------------------------
def test_argument_errors_and_aliasing():
    import flowonthego_amd as F
    from flowonthego_amd.histograms import motion_histograms
    L = F.lib()
    _p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    h, w, n = 16, 24, 2
    flow = torch.zeros((n, h, w, 2), device="cuda")
    mask = torch.zeros((n, h, w), dtype=torch.uint8, device="cuda")
    params = torch.zeros((n, 6), dtype=torch.float64, device="cuda")
    ids = torch.zeros((n, h, w), dtype=torch.int32, device="cuda")
    cells = torch.full((n, 2, 3, 32), -7, dtype=torch.int64, device="cuda")
    objs = torch.full((n, 4, 32), -7, dtype=torch.int64, device="cuda")
    big = torch.full((n * h * w * 2,), -7, dtype=torch.int64, device="cuda")           # room for an output laid over an input

    def call(n_=n, f=flow, w_=w, h_=h, m=mask, p=params, cell=8, t=102, c=cells, i=ids, rows=4, ob=objs):
        return L.fotg_motion_histograms(0, n_, _p(f), w_, h_, _p(m), _p(p), cell, t, _p(c), _p(i), rows, _p(ob), None)

    alias_f = big.view(torch.float32)[:n * h * w * 2].view(n, h, w, 2)
    for bad in (dict(n_=0), dict(n_=-1), dict(n_=65536), dict(w_=0), dict(h_=0), dict(w_=16385), dict(h_=16385), dict(f=None), dict(cell=0),
                dict(cell=12), dict(cell=64), dict(cell=-8), dict(t=-1), dict(c=None, ob=None), dict(i=None), dict(rows=0), dict(rows=1025),
                dict(c=big, f=alias_f), dict(ob=big, f=alias_f), dict(c=big, m=big.view(torch.uint8)), dict(c=big, p=big.view(torch.float64)),
                dict(ob=big, i=big.view(torch.int32)), dict(c=big, ob=big), dict(c=big, ob=big[32:])):
        assert call(**bad) == FOTG_ERR_ARG, {k: (v if isinstance(v, int) else "...") for k, v in bad.items()}
    torch.cuda.synchronize()
    assert bool((cells == -7).all()) and bool((objs == -7).all()) and bool((big == -7).all())
    assert call() == 0 and call(c=None) == 0 and call(ob=None, i=None) == 0 and call(ob=None, rows=0) == 0 and call(m=None, p=None) == 0
    # the fused form
    o = make_ctx(2, 64, 48, max_batch=2)
    wl, hl = o.out_size()
    cf = torch.zeros((2, hl, wl, 2), device="cuda")
    fc = torch.full((2, 6, 8, 32), -7, dtype=torch.int64, device="cuda")
    fused = lambda ctx=o._h, n_=2, f=cf, cell=8, t=0, c=fc: L.fotg_upsample_crop_motion_histograms(ctx, n_, _p(f), None, None, cell, t, _p(c), None, 4,
                                                                                                  None, None)
    for bad in (dict(ctx=None), dict(n_=3), dict(n_=0), dict(f=None), dict(c=None), dict(cell=7), dict(t=-2)):
        assert fused(**bad) == FOTG_ERR_ARG, bad
    torch.cuda.synchronize()
    assert bool((fc == -7).all())
    assert fused() == 0
    torch.cuda.synchronize()
    assert bool((fc[..., :25] == 0).all()) and bool((fc[..., R.N] == 64).all())            # a zero flow with thresh256 = 0: nothing in any bin
    o.close()
    # the Python layer refuses what it can see
    for kw in (dict(cell=12), dict(thresh=-1.0), dict(rows=0), dict(cells=False), dict(mask=mask[:1]), dict(motion=params[:, :5]), dict(ids=ids.to(torch.int64))):
        with pytest.raises(F.FotgError):
            motion_histograms(flow, **kw)


def test_a_call_on_another_stream():
    from flowonthego_amd.histograms import motion_histograms
    h, w = 40, 130
    flow, mask, params, ids = (dev(t) for t in scene(h, w))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got = motion_histograms(flow, mask, params, 16, ids=ids, rows=K)
    s.synchronize()
    assert_equal(got, want(h, w, 16, True, True), "stream")
