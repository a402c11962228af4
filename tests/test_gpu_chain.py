"""GPU tests of flow chaining (fotg_flow_chain / fotg_track_points and their fused forms, flowonthego_amd.chain).

The dense and the point form equal the numpy restatement (tests/chain_ref.py) byte for byte in total, code, steps, traj and the
five counters, on the seeded inputs that tests/test_chain.py shows to reach every code and step count; one step from integer
starts equals the flow itself and fb_check's forward mask (an existing kernel, not the restatement); the fused forms equal the
dense forms of fotg_upsample_crop's outputs byte for byte."""
import ctypes as C

import numpy as np
import pytest
import torch

import chain_ref as R

pytestmark = pytest.mark.gpu

FOTG_ERR_ARG = 1
f32 = np.float32


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
    return np.ascontiguousarray(a).view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


def same_traj(got, want):
    """byte for byte wherever the restatement is a number; a NaN (a non-finite start, repeated) must be a NaN"""
    got, want = got.cpu().numpy(), np.asarray(want)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(want)[~nan])


_REF = {}


def reference(w, h, n_seq, T, bw):
    """the restatement of one seeded case, computed once and shared: (F, B, total, code, steps, stats)"""
    key = (w, h, n_seq, T, bw)
    if key not in _REF:
        F, B = R.make_flows(w, h, n_seq, T)
        res = [R.chain(F[s], B[s] if bw else None) for s in range(n_seq)]
        total, code, steps = (np.stack([r[i] for r in res]) for i in range(3))
        st = np.stack([R.stats(code[s], steps[s]) for s in range(n_seq)]).astype(np.int64)
        for a in (F, B, total, code, steps, st):
            a.setflags(write=False)
        _REF[key] = (F, B, total, code, steps, st)
    return _REF[key]


def p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def raw_dense(F, B, off):
    """fotg_flow_chain into slices that start `off` elements into larger tensors (off = 1: no output is 16-byte or dword aligned)"""
    L = _F()[0].lib()
    n, T, h, w = F.shape[:4]
    total = torch.full((n * h * w * 2 + 8,), -7.0, device="cuda")[off:off + n * h * w * 2]
    code = torch.full((n * h * w + 8,), 9, dtype=torch.uint8, device="cuda")[off:off + n * h * w]
    steps = torch.full((n * h * w + 8,), -1, dtype=torch.int32, device="cuda")[off:off + n * h * w]
    st = torch.full((n * 5 + 1,), -1, dtype=torch.int64, device="cuda")[off:off + n * 5]
    assert L.fotg_flow_chain(0, n, T, p(F), p(B), w, h, C.c_float(0.01), C.c_float(0.5), p(total), p(code), p(steps), p(st), None) == 0
    return total.view(n, h, w, 2), code.view(n, h, w), steps.view(n, h, w), st.view(n, 5)


# ---- the dense and the point form against the restatement ----------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", R.SIZES)
def test_dense_equals_the_restatement(w, h):
    from flowonthego_amd.chain import chain
    for n_seq in (1, 2):
        for T in (1, 2, 5):
            for bw in (False, True):
                F, B, total, code, steps, st = reference(w, h, n_seq, T, bw)
                dF, dB = dev(F), dev(B) if bw else None
                got = chain(dF, dB, stats=True)
                again = chain(dF, dB, stats=True)
                unal = raw_dense(dF, dB, 1)
                one = chain(dF[0], None if dB is None else dB[0], stats=True)
                torch.cuda.synchronize()
                for g in (got, unal):
                    for a, b, nm in zip(g, (total, code, steps, st), ("total", "code", "steps", "stats")):
                        assert same(a, b), (n_seq, T, bw, nm, np.argwhere(bits(a) != bits(b))[:5])
                assert same(again[3], got[3])                                      # the counters repeat
                for a, b in zip(one, (total, code, steps, st)):                   # a sequence alone equals itself in a batch
                    assert same(a, b[0])


@pytest.mark.parametrize("w,h", R.SIZES)
def test_points_equal_the_restatement(w, h):
    from flowonthego_amd.chain import chain, track_points
    L = _F()[0].lib()
    ys, xs = np.mgrid[0:h, 0:w]
    grid = np.stack([xs.ravel(), ys.ravel()], -1).astype(f32)
    for n_seq in (1, 2):
        for T in (1, 2, 5):
            for bw in (False, True):
                F, B, total, code, steps, st = reference(w, h, n_seq, T, bw)
                dF, dB = dev(F), dev(B) if bw else None
                # a point on every pixel centre: the dense chain
                traj, pc, ps, pst = track_points(dev(grid), dF, dB, stats=True)
                torch.cuda.synchronize()
                assert same(traj[:, T], grid[None] + total.reshape(n_seq, -1, 2)), (n_seq, T, bw)
                assert same(traj[:, 0], np.broadcast_to(grid, (n_seq,) + grid.shape))
                assert same(pc, code.reshape(n_seq, -1)) and same(ps, steps.reshape(n_seq, -1)) and same(pst, st)
                # points off the grid, on the border, outside the frame and non-finite (300: more than one workgroup)
                pts = R.make_points(w, h, n_seq, 300)
                want = [R.track(pts[s], F[s], B[s] if bw else None) for s in range(n_seq)]
                traj, pc, ps, pst = track_points(dev(pts), dF, dB, stats=True)
                # the same into slices of larger tensors: traj 4 bytes off an 8-byte boundary
                t2 = torch.full((n_seq * (T + 1) * 300 * 2 + 2,), -7.0, device="cuda")[1:-1]
                c2 = torch.full((n_seq * 300 + 2,), 9, dtype=torch.uint8, device="cuda")[1:-1]
                assert L.fotg_track_points(0, n_seq, T, p(dF), p(dB), w, h, C.c_float(0.01), C.c_float(0.5), 300, p(dev(pts)), p(t2), p(c2),
                                           None, None, None) == 0
                torch.cuda.synchronize()
                assert same_traj(traj, np.stack([r[0] for r in want])), (n_seq, T, bw)
                assert same_traj(t2.view(n_seq, T + 1, 300, 2), np.stack([r[0] for r in want]))
                assert same(pc, np.stack([r[1] for r in want])) and same(c2.view(n_seq, 300), np.stack([r[1] for r in want]))
                assert same(ps, np.stack([r[2] for r in want]))
                assert same(pst, np.stack([R.stats(r[1], r[2]) for r in want]).astype(np.int64))


# ---- one step from integer starts: the flow itself and fb_check's mask ----------------------------------------------------------------
@pytest.mark.parametrize("w,h", R.SIZES[:2])
def test_one_step_is_the_flow_and_the_mask_of_fb_check(w, h):
    from flowonthego_amd.chain import chain
    from flowonthego_amd.consistency import fb_check
    F, B = R.make_flows(w, h, 2, 1)
    F, B = F[:, 0].copy(), B[:, 0].copy()
    total, code, steps = chain(dev(F[:, None]), dev(B[:, None]))
    mask, _ = fb_check(dev(F), dev(B))
    torch.cuda.synchronize()
    total, code, steps, mask = total.cpu().numpy(), code.cpu().numpy(), steps.cpu().numpy(), mask.cpu().numpy()
    ok = code == 0
    assert ok.mean() > 0.2 and (total[ok] == F[ok]).all() and np.array_equal(steps, ok.astype(np.int32))
    # byte for byte wherever the three weight-0 taps of the pixel (right, below, diagonal) are finite: a non-finite one makes the
    # lerp, and so the chain, unknown (csrc/chain.hip.h), where fb_check reads the pixel's own vector alone
    fin = np.isfinite(F).all(-1)
    pad = np.pad(fin, ((0, 0), (0, 1), (0, 1)), mode="edge")
    clean = pad[:, :-1, 1:] & pad[:, 1:, :-1] & pad[:, 1:, 1:]
    assert np.array_equal(code[clean], mask[clean]) and (code[~clean] == 3).all()
    assert clean.mean() > 0.8 and all((mask[clean] == c).any() for c in range(4))
    # and everywhere, byte for byte, on a flow without non-finite vectors (huge ones and a NaN row in B stay)
    F2 = np.where(np.isfinite(F), F, f32(2.5))
    c2 = chain(dev(F2[:, None]), dev(B[:, None]))[1]
    m2, _ = fb_check(dev(F2), dev(B))
    torch.cuda.synchronize()
    assert torch.equal(c2, m2) and all((m2 == c).any().item() for c in range(3))


# ---- the fused forms ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sc_l", [0, 1, 2, 3])
def test_fused_equals_unfused(sc_l):
    rng = np.random.default_rng(170 + sc_l)
    T = 3
    for w, h in ((97, 61), (64, 48)):
        o = make_ctx(2, w, h, max_batch=T, finest_scale=sc_l, coarsest_scale=max(sc_l, 4), use_var_ref=False)
        wl, hl = o.out_size()
        ys, xs = np.mgrid[0:hl, 0:wl].astype(np.float64) * (1 << sc_l)
        cf = np.stack([np.stack([2.5 * np.cos(k + 1.0) + 0.5 * np.sin(ys / 17.0), 2.5 * np.sin(k + 1.0) + 0.5 * np.cos(xs / 13.0)], -1)
                       for k in range(T)])
        cf = ((cf + 0.03 * rng.standard_normal(cf.shape)) / (1 << sc_l)).astype(f32)       # smooth: consistent with its negative
        cb = -cf
        cb[:, :, 2 * wl // 3:] = rng.standard_normal((T, hl, wl - 2 * wl // 3, 2)).astype(f32) * (3.0 / (1 << sc_l))
        cf[0, hl // 2, wl // 2:wl // 2 + 4] = (np.nan, 0.0)               # (in the middle: the crop drops the coarse border)
        cf[1, hl // 3, wl // 3:wl // 3 + 3] = (np.inf, 1.0)
        cb[2, hl // 2, wl // 4:wl // 4 + 3] = (0.0, -np.inf)
        pts = dev(R.make_points(w, h, 1, 300)[0])
        for b in (None, dev(cb)):
            got = o.upsample_crop_chain(dev(cf), b, stats=True, fused=True)
            want = o.upsample_crop_chain(dev(cf), b, stats=True, fused=False)
            gp = o.upsample_crop_track_points(pts, dev(cf), b, stats=True, fused=True)
            wp = o.upsample_crop_track_points(pts, dev(cf), b, stats=True, fused=False)
            torch.cuda.synchronize()
            for a, c, nm in zip(got, want, ("total", "code", "steps", "stats")):
                assert same(a, c), (w, h, b is not None, nm)
            assert same_traj(gp[0], wp[0].cpu().numpy())
            for a, c, nm in zip(gp[1:], wp[1:], ("code", "steps", "stats")):
                assert same(a, c), (w, h, b is not None, nm)
            code = got[1].cpu().numpy()
            assert (code == 0).any() and (code == 3).any() and (b is None or (code == 1).any())
        o.close()


# ---- arguments ------------------------------------------------------------------------------------------------------------------
def test_arguments_are_refused():
    F, OFClass = _F()
    L = F.lib()
    n, T, h, w, P = 2, 3, 9, 11, 7
    fl = torch.zeros((n, T, h, w, 2), device="cuda")
    fb = torch.zeros((n, T, h, w, 2), device="cuda")
    pts = torch.ones((n, P, 2), device="cuda")
    total = torch.empty((n, h, w, 2), device="cuda")
    traj = torch.empty((n, T + 1, P, 2), device="cuda")
    code = torch.empty((n, h, w), dtype=torch.uint8, device="cuda")
    steps = torch.empty((n, h, w), dtype=torch.int32, device="cuda")
    st = torch.empty((n, 5), dtype=torch.int64, device="cuda")
    a1, a2 = C.c_float(0.01), C.c_float(0.5)
    dense = lambda n_=n, T_=T, f=fl, b=fb, w_=w, h_=h, t=total, c=code, s=steps, q=st: L.fotg_flow_chain(
        0, n_, T_, p(f), p(b), w_, h_, a1, a2, p(t), p(c), p(s), p(q), None)
    points = lambda n_=n, T_=T, f=fl, b=fb, w_=w, h_=h, P_=P, x=pts, t=traj, c=code, s=steps, q=st: L.fotg_track_points(
        0, n_, T_, p(f), p(b), w_, h_, a1, a2, P_, p(x), p(t), p(c), p(s), p(q), None)
    assert dense() == 0 and dense(b=None) == 0 and dense(c=None, s=None, q=None) == 0 and dense(t=None, c=None, s=None) == 0
    assert points() == 0 and points(b=None, c=None, s=None, q=None) == 0
    bad_common = (dict(n_=0), dict(n_=-1), dict(n_=65536), dict(T_=0), dict(T_=-3), dict(w_=0), dict(h_=-2), dict(f=None),
                  dict(w_=1 << 21, h_=1 << 21),                                     # 2^32 workgroups: more than a grid's x dimension holds
                  dict(t=None, c=None, s=None, q=None), dict(t=fl), dict(t=fb), dict(q=fl))
    for bad in bad_common:
        assert dense(**bad) == FOTG_ERR_ARG, bad
        assert points(**bad) == FOTG_ERR_ARG, bad
    for bad in (dict(P_=0), dict(P_=-1), dict(x=None), dict(t=pts)):
        assert points(**bad) == FOTG_ERR_ARG, bad
    assert dense() == 0 and points() == 0                                          # a valid call afterwards succeeds
    o = make_ctx(2, 64, 48, max_batch=2)
    wl, hl = o.out_size()
    cf = torch.zeros((2, hl, wl, 2), device="cuda")
    tot = torch.empty((48, 64, 2), device="cuda")
    tr = torch.empty((3, P, 2), device="cuda")
    fd = lambda ctx=o._h, T_=2, f=cf, b=None, t=tot: L.fotg_upsample_crop_flow_chain(ctx, T_, p(f), p(b), a1, a2, p(t), None, None, None, None)
    fp = lambda ctx=o._h, T_=2, f=cf, P_=P, x=pts, t=tr: L.fotg_upsample_crop_track_points(ctx, T_, p(f), None, a1, a2, P_, p(x), p(t), None, None, None, None)
    assert fd() == 0 and fp() == 0 and fd(T_=1) == 0
    for bad in (dict(ctx=None), dict(T_=3), dict(T_=0), dict(f=None), dict(t=None), dict(t=cf)):
        assert fd(**bad) == FOTG_ERR_ARG, bad
        assert fp(**bad) == FOTG_ERR_ARG, bad
    assert fp(P_=0) == FOTG_ERR_ARG and fp(x=None) == FOTG_ERR_ARG
    op = F.operating_point(2, 64, 1)
    op.depth_mode = True
    od = OFClass(op, F.img_params(width=64, height=48), max_batch=2)
    assert fd(ctx=od._h) == FOTG_ERR_ARG and fp(ctx=od._h) == FOTG_ERR_ARG
    with pytest.raises(F.FotgError):
        od.upsample_crop_chain(cf)
    assert fd() == 0 and fp() == 0
    torch.cuda.synchronize()


# ---- it does what it is for -----------------------------------------------------------------------------------------------------
def test_track_follows_the_alley_over_two_frames(alley):
    """frames 1, 2, 3 of alley_1: frame 3 pulled back along the chained flow 1 -> 2 -> 3 is closer to frame 1 than frame 3 itself,
    over the pixels whose chain is valid to the end.  The figures are printed before the assertion."""
    import os
    from conftest import GOLDEN
    from flowonthego_amd.warp import warp
    more = np.load(os.path.join(GOLDEN, "alley_1_more.npz"))
    fr = np.stack([alley["frame_0001"], alley["frame_0002"], more["frame_0003"]]).astype(f32)
    h, w = fr.shape[1:]
    o = make_ctx(2, w, h, max_batch=2, bidir=True)
    frames = dev(fr)
    total, code, steps, st = o.track(frames, stats=True)
    _, _, ws = warp(frames[2], total, ref=frames[0], occ=code, stats=True)
    # the direct flow 1 -> 3 for comparison, with its own consistency mask
    fw, bw = o.calc_bidirectional(frames[0:1], frames[2:3])
    mask, _ = o.upsample_crop_fb_check(fw, bw)
    _, _, ds = o.upsample_crop_warp(fw, frames[2:3], ref=frames[0:1], occ=mask, stats=True)
    pts = dev(np.array([[100.5, 200.25], [1023, 435], [-1, 5]], f32))
    traj, pc, ps = o.track(frames, points=pts)
    torch.cuda.synchronize()
    st, ws, ds = st.cpu().numpy(), ws.cpu().numpy(), ds[0].cpu().numpy()
    print("chained 1->2->3: valid %.4f occluded %.4f outside %.4f unknown %.4f mean steps %.3f; mean |I1 - warp(I3)| %.3f, mean |I1 - I3| %.3f"
          % (tuple(st[:4] / (h * w)) + (st[4] / (h * w), ws[4] / ws[0], ws[5] / ws[0])))
    print("direct 1->3: valid %.4f; mean |I1 - warp(I3)| %.3f, mean |I1 - I3| %.3f" % (ds[0] / (h * w), ds[4] / ds[0], ds[5] / ds[0]))
    assert st[:4].sum() == h * w and ws[0] == st[0] > 0
    assert ws[4] < ws[5]
    assert same(ps[2:], np.zeros(1, np.int32)) and pc[2].item() == 2 and same_traj(traj[0], pts.cpu().numpy())
    o.close()
