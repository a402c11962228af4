"""GPU tests of the block motion vectors (fotg_block_motion / fotg_upsample_crop_block_motion, flowonthego_amd.blockmotion,
OFClass.block_motion).

The definition is integer arithmetic, so the dense form equals the numpy restatement (tests/blockmotion_ref.py) byte for byte in mv,
cost, kind, pred and stats, and the fused form equals the dense form of fotg_upsample_crop's output bit for bit.  No tolerance
appears anywhere.

The sizes are the smallest at which the kernel's paths differ (a wave per block of 8, 16 or 32 pixels, a lane owning 1, 4 or 4 x 4 of
them): 1 x 1, 5 x 3 (smaller than any block), 19 x 67 (partial blocks both ways, a width that is no multiple of four) and 40 x 130
(several block rows, a partial second row at block 32, more than one workgroup)."""
import ctypes as C

import numpy as np
import pytest
import torch

import blockmotion_ref as R
from test_gpu_warp import dev, make_ctx, same_bits as _same_bits

pytestmark = pytest.mark.gpu

FOTG_ERR_ARG = 1
SIZES = ((1, 1), (5, 3), (19, 67), (40, 130))          # (h, w)
NAMES = ("mv", "cost", "kind", "pred", "stats")
_SCENES, _WANT = {}, {}


def same_bits(a, b):
    """test_gpu_warp.same_bits; a uint32 tensor is compared through its int32 view"""
    if a.dtype == torch.uint32 and b.dtype == torch.uint32:
        a, b = a.view(torch.int32), b.view(torch.int32)
    return _same_bits(a, b)


def scene(h, w, noc, seed=0):
    """the frames, the flow and the mask of a case, computed once (nobody writes to them)"""
    key = (h, w, noc, seed)
    if key not in _SCENES:
        _SCENES[key] = R.scene(h, w, noc, 1000 * h + 10 * noc + seed)
    return _SCENES[key]


def restatement(h, w, noc, block, refine, masked=True):
    key = (h, w, noc, block, refine, masked)
    if key not in _WANT:
        cur, ref, flow, mask = scene(h, w, noc)
        _WANT[key] = R.block_motion(cur, ref, flow, mask if masked else None, block, refine)
    return _WANT[key]


def assert_equals_restatement(got, want, what):
    for g, w_, nm in zip(got, want, NAMES):
        g = g.cpu().numpy()
        assert g.dtype == w_.dtype and g.shape == w_.shape, (what, nm, g.dtype, g.shape, w_.shape)
        assert np.array_equal(g, w_), (what, nm, np.argwhere(g != w_)[:5].tolist())


# ---- the dense form ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("refine", [0, 3])
@pytest.mark.parametrize("noc", [1, 3])
@pytest.mark.parametrize("block", [8, 16, 32])
def test_dense_equals_the_restatement(block, noc, refine):
    from flowonthego_amd.blockmotion import block_motion
    for h, w in SIZES:
        cur, ref, flow, mask = (dev(a) for a in scene(h, w, noc))
        got = block_motion(cur, ref, flow, mask=mask, block=block, refine=refine, pred=True, stats=True)
        again = block_motion(cur, ref, flow, mask=mask, block=block, refine=refine, pred=True, stats=True)
        torch.cuda.synchronize()
        for a, b in zip(got, again):                              # two identical calls give identical bytes
            assert same_bits(a, b)
        want = restatement(h, w, noc, block, refine)
        assert_equals_restatement(got, want, (h, w))


def test_every_kind_and_the_moved_bit_occur():
    """over the union of the cases above (the restatement's kinds, which the GPU's equal): every branch is populated"""
    SEEN = set()
    for block in (8, 16, 32):
        for noc in (1, 3):
            for refine in (0, 3):
                for h, w in SIZES[2:]:
                    SEEN.update(np.unique(restatement(h, w, noc, block, refine)[2]).tolist())
    assert {k & 7 for k in SEEN} == set(range(7)) and any(k & 8 for k in SEEN), sorted(SEEN)


def test_calling_forms():
    import flowonthego_amd as F
    from flowonthego_amd.blockmotion import block_motion
    h, w, noc = 19, 67, 3
    cur, ref, flow, mask = (dev(a) for a in scene(h, w, noc))
    # no mask
    got = block_motion(cur, ref, flow, block=8, refine=2, pred=True, stats=True)
    assert_equals_restatement(got, restatement(h, w, noc, 8, 2, masked=False), "no mask")
    # the outputs that are not asked for are left out, the others do not change
    full = block_motion(cur, ref, flow, mask=mask, block=16, refine=1, pred=True, stats=True)
    for kw, idx in ((dict(), (0, 1, 2)), (dict(pred=True), (0, 1, 2, 3)), (dict(stats=True), (0, 1, 2, 4))):
        part = block_motion(cur, ref, flow, mask=mask, block=16, refine=1, **kw)
        assert len(part) == len(idx)
        for p, j in zip(part, idx):
            assert same_bits(p, full[j]), (kw, NAMES[j])
    # a single image without the batch dimension is its slice of the batch; the package attribute is the same function
    one = F.block_motion(cur[1], ref[1], flow[1], mask=mask[1], block=16, refine=1, pred=True, stats=True)
    for p, f_, nm in zip(one, full, NAMES):
        assert same_bits(p, f_[1]), nm
    gray = [dev(a) for a in scene(h, w, 1)]
    a = block_motion(gray[0], gray[1], gray[2], block=32)
    b = block_motion(gray[0].unsqueeze(-1), gray[1].unsqueeze(-1), gray[2], block=32)            # (n, h, w, 1) is (n, h, w)
    for p, q in zip(a, b):
        assert same_bits(p, q)
    torch.cuda.synchronize()


@pytest.mark.parametrize("noc", [1, 3])
def test_the_bound_image(noc):
    """a flow of constant (-4096, 4096) and one of (4096, -4096) with refine 3: every tap of every candidate clamps"""
    from flowonthego_amd.blockmotion import block_motion
    h, w = 19, 67
    cur, ref, _, _ = scene(h, w, noc)
    for sign in (1.0, -1.0):
        flow = np.empty((len(cur), h, w, 2), np.float32)
        flow[:] = (-4096.0 * sign, 4096.0 * sign)
        for block in (8, 16, 32):
            got = block_motion(dev(cur), dev(ref), dev(flow), block=block, refine=3, pred=True, stats=True)
            want = R.block_motion(cur, ref, flow, None, block, 3)
            assert_equals_restatement(got, want, (sign, block))
            assert (np.abs(want[0].astype(int)) <= R.QMAX).all()
        # a cur of the corner's value is predicted exactly by the vector at the bound: it wins everywhere and does not move
        flat = np.ascontiguousarray(np.broadcast_to(ref[:, h - 1 if sign > 0 else 0, 0 if sign > 0 else w - 1][:, None, None], cur.shape))
        mv, cost, kind = block_motion(dev(flat), dev(ref), dev(flow), block=16, refine=3)
        assert (mv.cpu().numpy() == (-16384 * sign, 16384 * sign)).all() and (kind == 1).all() and (cost[..., 0].cpu().numpy() == 0).all()


# ---- the fused form ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noc,block,refine", [(1, 16, 2), (3, 8, 3), (1, 32, 1), (3, 16, 0)])
def test_fused_equals_dense_on_the_upsampled_flow(noc, block, refine):
    from flowonthego_amd.blockmotion import block_motion
    n = 3
    for w, h in ((128, 40), (67, 37)):                        # 128 x 40 needs no padding; 67 x 37: the pyramid pads to 68 x 40
        rng = np.random.default_rng(300 + block + w)
        o = make_ctx(2, w, h, max_batch=n, finest_scale=1, coarsest_scale=2, use_var_ref=False)
        assert ((o.padw, o.padh) != (0, 0)) == (w == 67)
        wl, hl = o.out_size()
        cf = (rng.standard_normal((n, hl, wl, 2)) * 1.5).astype(np.float32)
        cf[0, 0, :3] = (np.nan, 0.0)
        cf[-1, hl // 2, :2] = (np.inf, 1.0)
        cf[1, hl // 3, wl // 2] = (3e38, -3e38)
        cf[2, hl // 4, wl // 3] = (5000.0, -2100.0)
        cur, ref, _, mask = (dev(a) for a in scene(h, w, noc))
        cf = dev(cf)
        kw = dict(mask=mask, block=block, refine=refine, pred=True, stats=True)
        got = o.upsample_crop_block_motion(cf, cur, ref, fused=True, **kw)
        unf = o.upsample_crop_block_motion(cf, cur, ref, fused=False, **kw)
        want = block_motion(cur, ref, o.upsample_crop(cf), **kw)
        torch.cuda.synchronize()
        for g, u, w_, nm in zip(got, unf, want, NAMES):
            assert same_bits(g, w_) and same_bits(u, w_), nm
        assert ((got[2] & 7) != 0).any()                           # the flow proposed vectors that won
        plain = o.upsample_crop_block_motion(cf, cur, ref, block=block, refine=refine)
        assert len(plain) == 3
        for g, w_ in zip(plain, block_motion(cur, ref, o.upsample_crop(cf), block=block, refine=refine)):
            assert same_bits(g, w_)


# ---- the whole thing in one call --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("occlusion", [False, True])
def test_ofclass_block_motion_is_the_explicit_sequence(occlusion, alley):
    from test_gpu_temporal import sequence
    frames = dev(sequence(alley)[0].astype(np.uint8))             # the clean window sliding over an 8-bit frame: whole numbers
    I0, I1 = frames[:4].contiguous(), frames[1:5].contiguous()
    mb = 3                                                         # two chunks: 3 pairs and 1
    o = make_ctx(2, 96, 64, max_batch=mb, bidir=occlusion)
    kw = dict(block=16, refine=2, pred=True, stats=True)
    got = o.block_motion(I0, I1, occlusion=occlusion, **kw)
    parts = []
    for s in range(0, 4, mb):
        a, b = I0[s:s + mb], I1[s:s + mb]
        if occlusion:
            fw, bw = o.calc_bidirectional_u8(a, b)
            m = o.upsample_crop_fb_check(fw, bw)[0]
        else:
            fw, m = o.calc_batch_u8(a, b), None
        parts.append((fw,) + o.upsample_crop_block_motion(fw, a, b, mask=m, **kw))
    torch.cuda.synchronize()
    assert len(got) == 6 and got[1].shape == (4, 4, 6, 2) and got[2].shape == (4, 4, 6, 2) and got[3].shape == (4, 4, 6)
    assert got[4].shape == I0.shape and got[5].shape == (4, 11)
    for j, nm in enumerate(("flow",) + NAMES):
        want = torch.cat([p[j].view(torch.int32) if p[j].dtype == torch.uint32 else p[j] for p in parts])
        assert same_bits(got[j].view(torch.int32) if got[j].dtype == torch.uint32 else got[j], want), nm
    assert (got[5][:, 0] <= got[5][:, 1]).all() and (got[5][:, 4] < 24).all()      # the flow's vectors won somewhere
    only = o.block_motion(I0, I1, occlusion=occlusion, block=16, refine=2)
    assert len(only) == 4 and same_bits(only[1], got[1]) and same_bits(only[3], got[3])


# ---- every refused argument -------------------------------------------------------------------------------------------------------
def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def test_arguments_are_refused_and_nothing_is_launched():
    import flowonthego_amd as F
    from flowonthego_amd.blockmotion import block_motion
    L = F.lib()
    n, h, w = 2, 21, 70
    rng = np.random.default_rng(5)
    s = dict(n=n, w=w, h=h, ch=1, block=16, refine=2, cur=dev(rng.integers(0, 256, (n, h, w), dtype=np.uint8)),
             ref=dev(rng.integers(0, 256, (n, h, w), dtype=np.uint8)), flow=dev(rng.standard_normal((n, h, w, 2)).astype(np.float32)),
             mask=None, mv=torch.full((n, 2, 5, 2), -7, dtype=torch.int16, device="cuda"),
             cost=torch.full((n, 2, 5, 2), -7, dtype=torch.int32, device="cuda"),
             kind=torch.full((n, 2, 5), 99, dtype=torch.uint8, device="cuda"), pred=torch.full((n, h, w), 99, dtype=torch.uint8, device="cuda"),
             stats=torch.full((n, 11), -7, dtype=torch.int64, device="cuda"))

    def call(**over):
        a = dict(s, **over)
        return L.fotg_block_motion(0, a["n"], _p(a["cur"]), _p(a["ref"]), a["w"], a["h"], a["ch"], _p(a["flow"]), _p(a["mask"]),
                                   a["block"], a["refine"], _p(a["mv"]), _p(a["cost"]), _p(a["kind"]), _p(a["pred"]), _p(a["stats"]), None)

    bad = [dict(n=0), dict(n=-1), dict(n=65536), dict(w=0), dict(h=-1), dict(w=16385), dict(h=16385), dict(ch=2), dict(ch=0), dict(ch=4),
           dict(block=12), dict(block=0), dict(block=64), dict(block=-8), dict(refine=4), dict(refine=-1), dict(cur=None), dict(ref=None),
           dict(flow=None), dict(mv=None), dict(cost=None), dict(kind=None), dict(pred=s["cur"]), dict(pred=s["ref"][1:])]
    for b in bad:
        assert call(**b) == FOTG_ERR_ARG, b
    torch.cuda.synchronize()
    assert (s["mv"] == -7).all() and (s["cost"] == -7).all() and (s["kind"] == 99).all() and (s["pred"] == 99).all() and (s["stats"] == -7).all()
    assert call() == 0 and call(pred=None, stats=None) == 0
    torch.cuda.synchronize()
    assert (s["kind"] != 99).all() and (s["stats"][:, 4:].sum(dim=1) == 10).all()
    # the module: FotgError for block 12, refine 4, f32 frames, two channels and mismatched shapes
    cur, ref, flow = s["cur"], s["ref"], s["flow"]
    two = torch.zeros((n, h, w, 2), dtype=torch.uint8, device="cuda")
    for args, kw in (((cur, ref, flow), dict(block=12)), ((cur, ref, flow), dict(refine=4)), ((cur, ref, flow), dict(refine=1.0)),
                     ((cur.float(), ref.float(), flow), {}), ((cur, ref.float(), flow), {}), ((two, two, flow), {}),
                     ((cur[:, :20], ref[:, :20], flow), {}), ((cur, ref[:1], flow), {}), ((cur, ref, flow[..., :1]), {}),
                     ((cur, ref, flow.double()), {}), ((cur, ref, flow), dict(mask=torch.zeros((n, h, w + 1), dtype=torch.uint8, device="cuda"))),
                     ((cur.cpu(), ref.cpu(), flow), {})):
        with pytest.raises(F.FotgError):
            block_motion(*args, **kw)
    # the fused form
    o = make_ctx(2, 64, 48, max_batch=2)
    wl, hl = o.out_size()
    cf = torch.zeros((2, hl, wl, 2), device="cuda")
    fr = torch.zeros((2, 48, 64), dtype=torch.uint8, device="cuda")
    mv = torch.full((2, 3, 4, 2), -7, dtype=torch.int16, device="cuda")
    cost = torch.zeros((2, 3, 4, 2), dtype=torch.int32, device="cuda")
    kind = torch.zeros((2, 3, 4), dtype=torch.uint8, device="cuda")
    fused = lambda ctx=o._h, n=2, f=cf, c=fr, r=fr, ch=1, block=16, refine=2, m=mv: L.fotg_upsample_crop_block_motion(
        ctx, n, _p(f), _p(c), _p(r), ch, None, block, refine, _p(m), _p(cost), _p(kind), None, None, None)
    for b in (dict(ctx=None), dict(n=3), dict(n=0), dict(f=None), dict(c=None), dict(r=None), dict(ch=2), dict(block=12), dict(refine=4),
              dict(m=None)):
        assert fused(**b) == FOTG_ERR_ARG, b
    torch.cuda.synchronize()
    assert (mv == -7).all()
    assert fused() == 0
    op = F.operating_point(2, 64, 1)
    op.depth_mode = True
    from flowonthego_amd.oflow import OFClass
    od = OFClass(op, F.img_params(width=64, height=48), max_batch=2)
    assert fused(ctx=od._h) == FOTG_ERR_ARG
    with pytest.raises(F.FotgError):
        od.block_motion(fr, fr)
    with pytest.raises(F.FotgError):
        o.block_motion(fr, fr, occlusion=True)                     # occlusion=True needs a bidir context
    with pytest.raises(F.FotgError):
        o.block_motion(fr.float(), fr.float())
    for kw in (dict(block=12), dict(refine=4)):
        with pytest.raises(F.FotgError):
            o.upsample_crop_block_motion(cf, fr, fr, **kw)
    torch.cuda.synchronize()
