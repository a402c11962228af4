"""GPU tests of the object tracks (fotg_object_overlap / fotg_upsample_crop_object_overlap / fotg_object_links / fotg_object_tracks,
flowonthego_amd.tracks, OFClass.track_objects).

The definition is integer arithmetic, so every output equals the numpy restatement (tests/tracks_ref.py) byte for byte, and the fused
overlap equals the dense one on fotg_upsample_crop's output bit for bit.  No tolerance appears anywhere; every call is made twice
and the bytes compared.

The sizes are the smallest at which the vote kernel's paths differ (a lane owns four adjacent pixels, a wave a strip of 256 pixels x
8 rows, a workgroup four such strips): 1 x 1, 5 x 3 (narrower than a lane's four pixels), 19 x 67 (a width that is no multiple of
four: every row starts at another alignment, with pixels taken one by one at both ends) and 40 x 130 (several waves and workgroups
both ways)."""
import ctypes as C

import numpy as np
import pytest
import torch

import tracks_ref as R
from test_gpu_warp import dev, make_ctx, same_bits

pytestmark = pytest.mark.gpu

FOTG_ERR_ARG = 1
SIZES = ((1, 1), (5, 3), (19, 67), (40, 130))          # (h, w)
K, N = 16, 3
_SCENES, _WANT = {}, {}


def scene(h, w, n=N, seed=0):
    """ids_a, ids_b (n, h, w), objects_a, objects_b (n, K, 11), flow (n, h, w, 2), mask (n, h, w) of a case, computed once (nobody
    writes to them): random blobs; vectors of a few pixels with fractions exactly at .5; NaN, infinities and +-5000 on foreground
    pixels; border strips whose vectors leave the frame by every edge; a mask with every code"""
    key = (h, w, n, seed)
    if key in _SCENES:
        return _SCENES[key]
    rng = np.random.default_rng(1000 * h + w + seed)
    code = np.zeros((2 * n, h, w), np.uint8)
    for k in range(2 * n):
        for _ in range(1 + (h * w) // 150):
            bh, bw = rng.integers(1, max(2, h // 2 + 1)), rng.integers(1, max(2, w // 3 + 1))
            y, x = rng.integers(0, h), rng.integers(0, w)
            code[k, y:y + bh, x:x + bw] = 1
    ids, objects = R.labelled(code, K)
    flow = (rng.integers(-3, 4, (n, h, w, 2)) + rng.choice([0.0, 0.5, -0.5, 0.25, 1.5], (n, h, w, 2))).astype(np.float32)
    b = max(1, min(h, w) // 8)
    flow[:, :b, :, 1] -= h
    flow[:, -b:, :, 1] += h + 0.5
    flow[:, b:-b or None, :b, 0] -= w + 0.5
    flow[:, b:-b or None, -b:, 0] += w
    fg = np.argwhere(ids[:n] >= 0)
    special = [(np.nan, 0), (0, np.nan), (np.inf, 1), (1, -np.inf), (5000, 0), (0, -5000), (-5000, 5000), (4096, 0), (0, -4096), (3e38, 0)]
    for s, p in zip(special, fg[rng.permutation(len(fg))[:len(special)]]):
        flow[tuple(p)] = s
    mask = rng.choice(np.array([0, 0, 0, 0, 0, 0, 1, 2, 3, 200], np.uint8), (n, h, w))
    _SCENES[key] = (ids[:n], ids[n:], objects[:n], objects[n:], flow, mask)
    return _SCENES[key]


def want_overlap(h, w, masked, ka=K, kb=K):
    key = (h, w, masked, ka, kb)
    if key not in _WANT:
        a, b, _, _, flow, mask = scene(h, w)
        _WANT[key] = R.overlap_batch(a, b, flow, mask if masked else None, ka, kb)
    return _WANT[key]


def assert_equal(got, want, what):
    got = [g.cpu().numpy() for g in got]
    for k, (g, w_) in enumerate(zip(got, want)):
        assert g.dtype == w_.dtype and g.shape == w_.shape, (what, k, g.dtype, g.shape, w_.dtype, w_.shape)
        assert np.array_equal(g, w_), (what, k, np.argwhere(g != w_)[:5].tolist())


def twice(fn):
    """two identical calls give identical bytes"""
    a, b = fn(), fn()
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert same_bits(x, y)
    return a


# ---- step 1, the dense form ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True])
def test_overlap_equals_the_restatement(masked):
    from flowonthego_amd.tracks import object_overlap
    for h, w in SIZES:
        a, b, _, _, flow, mask = (dev(t) for t in scene(h, w))
        got = twice(lambda: object_overlap(a, b, flow, mask if masked else None, ka=K, kb=K))
        votes, sent = want_overlap(h, w, masked)
        assert_equal(got, (votes, sent), (h, w))
        # the four columns add up to the pixels carrying the id
        area = np.stack([np.bincount(i[i >= 0], minlength=K) for i in scene(h, w)[0]])
        assert np.array_equal(got[1].cpu().numpy().sum(axis=2), area)
    # every branch is populated at the two larger sizes
    for h, w in SIZES[2:]:
        sent = want_overlap(h, w, masked)[1].sum(axis=(0, 1))
        assert (sent[:3] > 0).all() and sent[3] >= 7, sent


def test_row_counts_below_the_ids_and_unequal():
    from flowonthego_amd.tracks import object_overlap
    h, w = 19, 67
    a, b, _, _, flow, mask = scene(h, w)
    assert a.max() >= 3 and b.max() >= 3                          # there are ids beyond the row counts below
    for ka, kb in ((2, K), (K, 3), (5, 7), (1, 1), (1024, 1024)):
        got = twice(lambda: object_overlap(dev(a), dev(b), dev(flow), dev(mask), ka=ka, kb=kb))
        assert_equal(got, want_overlap(h, w, True, ka, kb), (ka, kb))
    # ids far beyond the rows, and negative ones other than -1, are background: nothing is written out of bounds
    wild = a.copy()
    wild[a == 1] = 1 << 30
    wild[a == 2] = -(1 << 31)
    got = twice(lambda: object_overlap(dev(wild), dev(b), dev(flow), dev(mask), ka=K, kb=K))
    assert_equal(got, R.overlap_batch(wild, b, flow, mask, K, K), "wild")
    # a single pair without the batch dimension is its slice of the batch
    one = object_overlap(dev(a[1]), dev(b[1]), dev(flow[1]), dev(mask[1]), ka=K, kb=K)
    assert_equal(one, [t[1] for t in want_overlap(h, w, True)], "single")


def test_unaligned_pointers_take_the_scalar_path():
    """views that start 4 bytes (ids), 8 bytes (flow) and 1 byte (mask) into an allocation"""
    from flowonthego_amd.tracks import object_overlap
    h, w = 40, 130
    a, b, _, _, flow, mask = scene(h, w)
    shift = lambda t, per: torch.cat([t.flatten()[:per], t.flatten()])[per:].view(t.shape)
    da, df, dm = shift(dev(a), 1), shift(dev(flow), 2), shift(dev(mask), 1)
    assert da.data_ptr() % 16 == 4 and df.data_ptr() % 16 == 8 and dm.data_ptr() % 4 == 1 and da.is_contiguous()
    for args in ((da, dev(b), dev(flow), dev(mask)), (dev(a), dev(b), df, dev(mask)), (dev(a), dev(b), dev(flow), dm)):
        assert_equal(twice(lambda: object_overlap(*args, ka=K, kb=K)), want_overlap(h, w, True), "unaligned")


def checkerboard():
    """40 x 130 at 4-connectivity, labelled with max_objects = 1024: 2600 single-pixel components, the first 1024 with a row, the
    others -1; its complement as frame b"""
    from flowonthego_amd.objects import label_components
    h, w = 40, 130
    ys, xs = np.mgrid[0:h, 0:w]
    code = np.stack([(xs + ys) % 2 == 0, (xs + ys) % 2 == 1]).astype(np.uint8)
    objects, ids, st = label_components(dev(code), (1,), 4, None, 1, 1024, ids=True, stats=True)
    assert st[:, 1].tolist() == [2600, 2600] and st[:, 3].tolist() == [1024, 1024]
    return ids, objects


def test_checkerboard_uses_all_1024_rows():
    """waves hold many distinct keys: more than a wave's 64 lanes can keep, so the pending keys leave mid-strip"""
    from flowonthego_amd.tracks import link_tracks, object_links, object_overlap
    ids, objects = checkerboard()
    h, w = ids.shape[1:]
    rng = np.random.default_rng(4)
    flow = (rng.integers(-2, 3, (1, h, w, 2)) + rng.choice([0.0, 0.5], (1, h, w, 2))).astype(np.float32)
    ida, idb = ids[:1].contiguous(), ids[1:].contiguous()
    got = twice(lambda: object_overlap(ida, idb, dev(flow), None, ka=1024, kb=1024))
    ia, ib = ids.cpu().numpy()
    assert ia.max() == 1023 and (ia == -1).sum() == h * w - 1024
    votes, sent = R.overlap_batch(ia[None], ib[None], flow, None, 1024, 1024)
    assert_equal(got, (votes, sent), "checkerboard")
    assert (votes > 0).sum() > 300                                 # many distinct keys
    obj = objects.cpu().numpy()
    for mv, mf in ((1, 0.0), (1, 1.0), (2, 0.25)):
        links = twice(lambda: object_links(got[0], objects[:1], objects[1:], min_votes=mv, min_frac=mf))
        want = R.links_batch(votes, obj[:1], obj[1:], mv, int(round(mf * 256)))
        assert_equal(links, want, ("links", mv, mf))
    links = object_links(got[0], objects[:1], objects[1:], min_votes=1, min_frac=0.0)
    tr = twice(lambda: link_tracks(objects, links[0], links[1], max_tracks=1500, stats=True))
    assert_equal(tr, R.tracks(obj, *R.links_batch(votes, obj[:1], obj[1:], 1, 0), 1500), "tracks")
    assert tr[2][0] > 1024 and 0 < tr[2][2] < 1024                 # some rows of frame 1 are linked, the others start tracks


def test_one_object_covering_the_frame():
    """every lane shares one key: the aggregation's extreme"""
    from flowonthego_amd.tracks import object_overlap
    h, w = 40, 130
    ids = np.zeros((2, h, w), np.int32)
    flow = np.zeros((2, h, w, 2), np.float32)
    flow[1] = (1.5, -2.5)                                          # rounds to (2, -2)
    got = twice(lambda: object_overlap(dev(ids), dev(ids), dev(flow), None, ka=1, kb=1))
    assert got[0].flatten().tolist() == [h * w, (h - 2) * (w - 2)]
    assert got[1].tolist() == [[[h * w, 0, 0, 0]], [[(h - 2) * (w - 2), 0, h * w - (h - 2) * (w - 2), 0]]]
    got = twice(lambda: object_overlap(dev(ids), dev(ids), dev(flow), None, ka=3, kb=5))
    assert_equal(got, R.overlap_batch(ids, ids, flow, None, 3, 5), "one object")


# ---- steps 2 and 3 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_votes,min_frac", [(1, 0.0), (1, 0.25), (4, 0.5), (1, 1.0), (30, 0.0)])
def test_links_equal_the_restatement(min_votes, min_frac):
    from flowonthego_amd.tracks import object_links
    for h, w in SIZES:
        _, _, oa, ob, _, _ = scene(h, w)
        for masked in (False, True):
            votes = want_overlap(h, w, masked)[0]
            got = twice(lambda: object_links(dev(votes), dev(oa), dev(ob), min_votes=min_votes, min_frac=min_frac))
            assert_equal(got, R.links_batch(votes, oa, ob, min_votes, int(round(min_frac * 256))), (h, w, masked))
    # ka != kb, and a single pair
    h, w = 19, 67
    _, _, oa, ob, _, _ = scene(h, w)
    votes = want_overlap(h, w, True, 5, 7)[0]
    oa5, ob7 = np.ascontiguousarray(oa[:, :5]), np.ascontiguousarray(ob[:, :7])
    got = twice(lambda: object_links(dev(votes), dev(oa5), dev(ob7), min_votes=min_votes, min_frac=min_frac))
    want = R.links_batch(votes, oa5, ob7, min_votes, int(round(min_frac * 256)))
    assert_equal(got, want, "5 x 7")
    one = object_links(dev(votes[2]), dev(oa5[2]), dev(ob7[2]), min_votes=min_votes, min_frac=min_frac)
    assert_equal(one, [t[2] for t in want], "single")


def sequence(h, w, frames=5, seed=3):
    """blobs drifting with their own velocity over `frames` frames, some leaving, some meeting: code, flow"""
    key = ("seq", h, w, frames, seed)
    if key not in _SCENES:
        rng = np.random.default_rng(seed + h)
        rects = tuple((int(rng.integers(0, w)), int(rng.integers(0, h)), int(rng.integers(2, 9)), int(rng.integers(2, 7)),
                       int(rng.integers(-4, 5)), int(rng.integers(-2, 3))) for _ in range(7))
        code, flow = R.fixed_scene(h, w, frames, rects)
        flow += rng.choice(np.array([0.0, 0.25, -0.25], np.float32), flow.shape)
        ids, objects = R.labelled(code, K)
        _SCENES[key] = (ids, objects, flow[:-1].copy())
    return _SCENES[key]


@pytest.mark.parametrize("case", ["fixed", "19x67", "40x130"])
def test_tracks_equal_the_restatement(case):
    import flowonthego_amd as F
    from flowonthego_amd.tracks import link_tracks, object_links, object_overlap, track_objects
    if case == "fixed":
        code, flow = R.fixed_scene()
        ids, objects = R.labelled(code, 8)
        flows, kw = flow[:-1].copy(), dict(min_votes=1, min_frac=0.25, max_tracks=16)
    else:
        h, w = (int(v) for v in case.split("x"))
        ids, objects, flows = sequence(h, w)
        kw = dict(min_votes=2, min_frac=0.25, max_tracks=5)          # fewer table rows than tracks
    want = R.track_objects(ids, objects, flows, None, kw["min_votes"], 64, kw["max_tracks"])
    dids, dobj, dfl = dev(ids), dev(objects), dev(flows)
    kk = objects.shape[1]
    votes, sent = twice(lambda: object_overlap(dids[:-1], dids[1:], dfl, None, ka=kk, kb=kk))
    ab, ba = twice(lambda: object_links(votes, dobj[:-1], dobj[1:], kw["min_votes"], kw["min_frac"]))
    track, table, st = twice(lambda: link_tracks(dobj, ab, ba, kw["max_tracks"], stats=True))
    assert_equal((votes, sent, ab, ba, track, table, st), [want[k] for k in ("votes", "sent", "link_ab", "link_ba", "track", "tracks", "stats")], case)
    # the whole thing in one call, with the per-pixel track ids; the package attribute is the same function
    got = twice(lambda: F.track_objects(dids, dobj, dfl, track_ids=True, stats=True, **kw))
    assert len(got) == 4 and same_bits(got[0], track) and same_bits(got[1], table) and same_bits(got[3], st)
    tid = np.where(ids >= 0, np.take_along_axis(want["track"], np.maximum(ids, 0).reshape(len(ids), -1), 1).reshape(ids.shape), -1)
    assert_equal(got[2:3], [tid.astype(np.int32)], "track_ids")
    plain = track_objects(dids, dobj, dfl, **kw)
    assert len(plain) == 2 and same_bits(plain[0], track) and same_bits(plain[1], table)
    if case == "fixed":
        assert want["track"][:, :4].tolist() == [[0, 1, 2, 3]] * 3 + [[0, 1, 2, -1]] * 2 + [[0, 2, -1, -1]] * 3
        assert want["tracks"][:4, 7].tolist() == [0, 2, 0, 3] and want["tracks"][:4, 1].tolist() == [7, 4, 7, 2] and want["stats"][0] == 4
    else:
        assert want["stats"][0] > kw["max_tracks"] and want["stats"][2] > 0
        assert case != "19x67" or set(want["tracks"][:, 7].tolist()) == {0, 2, 3}             # alive, merged and lost tracks


# ---- the fused form -----------------------------------------------------------------------------------------------------------------
def test_fused_equals_dense_on_the_upsampled_flow():
    from flowonthego_amd.tracks import object_overlap
    n = N
    for w, h in ((128, 40), (67, 37)):                            # 128 x 40 needs no padding; 67 x 37: the pyramid pads to 68 x 40
        rng = np.random.default_rng(300 + w)
        o = make_ctx(2, w, h, max_batch=n, finest_scale=1, coarsest_scale=2, use_var_ref=False)
        wl, hl = o.out_size()
        assert wl < w and hl < h
        cf = (rng.standard_normal((n, hl, wl, 2)) * 2.5).astype(np.float32)
        cf[0, 0, :3] = (np.nan, 0.0)
        cf[-1, hl // 2, :2] = (np.inf, 1.0)
        cf[1, hl // 3, wl // 2] = (3e38, -3e38)
        cf[2, hl // 4, wl // 3] = (5000.0, -2100.0)
        a, b, _, _, _, mask = (dev(t) for t in scene(h, w))
        cf = dev(cf)
        for m in (None, mask):
            got = twice(lambda: o.upsample_crop_object_overlap(cf, a, b, mask=m, ka=K, kb=K))
            unf = o.upsample_crop_object_overlap(cf, a, b, mask=m, ka=K, kb=K, fused=False)
            want = object_overlap(a, b, o.upsample_crop(cf), m, ka=K, kb=K)
            torch.cuda.synchronize()
            for g, u, w_ in zip(got, unf, want):
                assert same_bits(g, w_) and same_bits(u, w_)
            assert (got[0] > 0).any() and (got[1][..., 1] > 0).any() and ((got[1][..., 3] > 0).any() or m is None)
        o.close()


# ---- the whole thing in one call ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bidir", [False, True])
def test_ofclass_track_objects_is_the_documented_composition(bidir, natural_images):
    import flowonthego_amd as F
    import motion_ref as M
    from flowonthego_amd.motion import _sequence_flows
    from flowonthego_amd.tracks import link_tracks, object_links
    frames, _ = M.jittered_crops(natural_images["road_HD"], T=4, patch=True)
    T, (h, w) = len(frames) - 1, frames.shape[1:]
    dfr = dev(frames)
    o = make_ctx(2, w, h, max_batch=T, bidir=bidir)
    kw = dict(min_area=16, max_objects=32)
    got = o.track_objects(dfr, min_votes=8, min_frac=0.25, max_tracks=64, track_ids=True, stats=True, **kw)
    fw, mask = _sequence_flows(o, dfr)
    params, code, res = o.upsample_crop_fit_motion(fw, mask, code=True, residual=True)
    objects, ids = F.label_components(code, (1,), 8, res, 16, 32, ids=True)
    votes, _ = o.upsample_crop_object_overlap(fw[:-1], ids[:-1], ids[1:], None if mask is None else mask[:-1], ka=32, kb=32)
    ab, ba = object_links(votes, objects[:-1], objects[1:], 8, 0.25)
    track, table, st = link_tracks(objects, ab, ba, 64, stats=True)
    torch.cuda.synchronize()
    assert len(got) == 6 and got[2].shape == (T, 32) and got[3].shape == (64, 8) and got[4].shape == (T, h, w) and got[5].shape == (4,)
    for g, w_ in zip(got, (params, objects, track, table, None, st)):
        assert w_ is None or same_bits(g, w_)
    tr, idn = track.cpu().numpy(), ids.cpu().numpy()
    tid = np.where(idn >= 0, np.take_along_axis(tr, np.maximum(idn, 0).reshape(T, -1), 1).reshape(idn.shape), -1)
    assert np.array_equal(got[4].cpu().numpy(), tid)
    # the pasted patch moves on its own: a track follows it through all T object maps
    t = table.cpu().numpy()
    assert ((t[:, 1] - t[:, 0] == T - 1) & (t[:, 5] > 1000)).any(), t[:int(st[1])]
    short = o.track_objects(dfr, min_votes=8, min_frac=0.25, max_tracks=64, **kw)
    assert len(short) == 4 and same_bits(short[2], track) and same_bits(short[3], table)
    o.close()


# ---- every refused argument ---------------------------------------------------------------------------------------------------------
def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def test_arguments_are_refused_and_nothing_is_launched():
    import flowonthego_amd as F
    from flowonthego_amd.tracks import link_tracks, object_links, object_overlap, track_objects
    L = F.lib()
    n, h, w, k = 2, 9, 14, 4
    ids = torch.zeros((n + 1, h, w), dtype=torch.int32, device="cuda")
    flow = torch.zeros((n, h, w, 2), device="cuda")
    votes = torch.full((n, k, k), -7, dtype=torch.int32, device="cuda")
    sent = torch.full((n, k, 4), -7, dtype=torch.int64, device="cuda")
    objects = torch.ones((n + 1, k, 11), dtype=torch.int64, device="cuda")
    ab = torch.full((n, k, 3), -7, dtype=torch.int32, device="cuda")
    ba = torch.full((n, k, 3), -7, dtype=torch.int32, device="cuda")
    track = torch.full((n + 1, k), -7, dtype=torch.int32, device="cuda")
    table = torch.full((8, 8), -7, dtype=torch.int64, device="cuda")

    def ov(n_=n, a=ids[:-1], b=ids[1:], f=flow, ka=k, kb=k, v=votes, s=sent):
        return L.fotg_object_overlap(0, n_, _p(a), _p(b), w, h, _p(f), None, ka, kb, _p(v), _p(s), None)

    for bad in (dict(n_=0), dict(n_=65536), dict(ka=0), dict(kb=1025), dict(a=None), dict(f=None), dict(v=None), dict(s=None),
                dict(v=ids.view(torch.int32)), dict(s=flow), dict(v=sent)):
        assert ov(**bad) == FOTG_ERR_ARG, bad
    assert L.fotg_object_links(0, n, _p(votes), _p(objects), _p(objects[1:]), k, k, 0, 64, _p(ab), _p(ba), None) == FOTG_ERR_ARG
    assert L.fotg_object_links(0, n, _p(votes), _p(objects), _p(objects[1:]), k, k, 1, 257, _p(ab), _p(ba), None) == FOTG_ERR_ARG
    assert L.fotg_object_links(0, n, _p(votes), _p(objects), _p(objects[1:]), k, k, 1, 64, _p(ab), _p(ab), None) == FOTG_ERR_ARG
    assert L.fotg_object_tracks(0, n, k, _p(objects), _p(ab), _p(ba), 0, _p(track), _p(table), None, None) == FOTG_ERR_ARG
    assert L.fotg_object_tracks(0, n, k, _p(objects), _p(ab), _p(ba), 8, _p(track), _p(objects), None, None) == FOTG_ERR_ARG
    torch.cuda.synchronize()
    assert (votes == -7).all() and (sent == -7).all() and (ab == -7).all() and (ba == -7).all() and (track == -7).all() and (table == -7).all()
    assert ov() == 0
    assert L.fotg_object_links(0, n, _p(votes), _p(objects), _p(objects[1:]), k, k, 1, 64, _p(ab), _p(ba), None) == 0
    assert L.fotg_object_tracks(0, n, k, _p(objects), _p(ab), _p(ba), 8, _p(track), _p(table), None, None) == 0     # stats may be null
    torch.cuda.synchronize()
    # every row is written (area 1); only row 0 is linked: the other rows start a track per frame, two of them beyond the table
    assert votes[:, 0, 0].tolist() == [h * w] * n and track.tolist() == [[0, 1, 2, 3], [0, 4, 5, 6], [0, 7, 8, 9]]
    assert table[0].tolist() == [0, 2, 0, 0, 3, 1, 2 * h * w, 0] and table[1:, 7].tolist() == [3] * 3 + [3] * 3 + [0]
    # the module: FotgError for wrong types, shapes, devices and parameters
    a, b = ids[:-1], ids[1:]
    for args, kw in (((a, b, flow), dict(ka=0)), ((a, b, flow), dict(kb=1025)), ((a.long(), b, flow), {}), ((a, b[:1], flow), {}),
                     ((a, b, flow[..., :1]), {}), ((a, b, flow.double()), {}), ((a.cpu(), b.cpu(), flow), {}),
                     ((a, b, flow, torch.zeros((n, h, w + 1), dtype=torch.uint8, device="cuda")), {})):
        with pytest.raises(F.FotgError):
            object_overlap(*args, **kw)
    for kw in (dict(min_votes=0), dict(min_frac=1.5), dict(min_frac=-0.1), dict(min_votes=1.0)):
        with pytest.raises(F.FotgError):
            object_links(votes, objects[:-1], objects[1:], **kw)
    with pytest.raises(F.FotgError):
        object_links(votes, objects[:-1, :3], objects[1:])
    for mt in (0, 65537):
        with pytest.raises(F.FotgError):
            link_tracks(objects, ab, ba, max_tracks=mt)
    with pytest.raises(F.FotgError):
        track_objects(ids[:1], objects[:1], flow[:0])
    # the fused form
    o = make_ctx(2, 64, 48, max_batch=2)
    wl, hl = o.out_size()
    cf = torch.zeros((2, hl, wl, 2), device="cuda")
    fid = torch.zeros((2, 48, 64), dtype=torch.int32, device="cuda")
    fv = torch.full((2, k, k), -7, dtype=torch.int32, device="cuda")
    fs = torch.zeros((2, k, 4), dtype=torch.int64, device="cuda")
    fused = lambda ctx=o._h, n_=2, f=cf, a=fid, v=fv, ka=k: L.fotg_upsample_crop_object_overlap(ctx, n_, _p(f), _p(a), _p(fid), None, ka, k, _p(v),
                                                                                            _p(fs), None)
    for bad in (dict(ctx=None), dict(n_=3), dict(n_=0), dict(f=None), dict(a=None), dict(v=None), dict(ka=0), dict(ka=1025)):
        assert fused(**bad) == FOTG_ERR_ARG, bad
    torch.cuda.synchronize()
    assert (fv == -7).all()
    assert fused() == 0
    op = F.operating_point(2, 64, 1)
    op.depth_mode = True
    from flowonthego_amd.oflow import OFClass
    od = OFClass(op, F.img_params(width=64, height=48), max_batch=2)
    assert fused(ctx=od._h) == FOTG_ERR_ARG
    fr = torch.zeros((3, 48, 64), dtype=torch.uint8, device="cuda")
    with pytest.raises(F.FotgError):
        od.track_objects(fr)
    with pytest.raises(F.FotgError):
        o.track_objects(fr[:2])                                     # two frames give one object map and nothing to link
    with pytest.raises(F.FotgError):
        o.upsample_crop_object_overlap(cf, fid, fid, ka=0)
    torch.cuda.synchronize()
