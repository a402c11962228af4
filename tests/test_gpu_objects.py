"""GPU tests of the connected-component labelling (fotg_label_components, flowonthego_amd.objects) and of moving_objects.

Every output -- labels, ids, objects, stats -- equals the numpy restatement (tests/objects_ref.py) byte for byte: on seeded random
maps at three foreground densities, both connectivities, one and two foreground codes, with and without values; on structured maps
that stress the merges across tile edges and corners; under min_area and max_objects; written one element into larger tensors;
twice; on a non-default stream.  The labelling's tile is 64 x 16 (flowonthego_amd.objects.TILE, no larger than 64 in either
direction), so the structured maps are 200 x 150: four tiles across with a partial last one, ten down with a partial last one."""
import ctypes as C

import numpy as np
import pytest
import torch

import motion_ref as M
import objects_ref as R

pytestmark = pytest.mark.gpu

f32 = np.float32
KEYS = ("objects", "labels", "ids", "stats")


def _O():
    import flowonthego_amd.objects as O
    return O


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()       # (a copy: the shared inputs stay read-only)


def gpu(code, fg=(1,), conn=8, values=None, min_area=1, max_objects=256):
    out = _O().label_components(dev(code), fg, conn, None if values is None else dev(values), min_area, max_objects, labels=True, ids=True,
                                stats=True)
    torch.cuda.synchronize()
    return dict(zip(KEYS, (o.cpu().numpy() for o in out)))


def assert_same(got, want, what=""):
    for k in KEYS:
        a, b = got[k], want[k]
        assert a.shape == b.shape and a.dtype == b.dtype, (what, k, a.shape, b.shape, a.dtype, b.dtype)
        if a.tobytes() != b.tobytes():
            bad = np.argwhere(a != b)
            raise AssertionError("%s %s: %d elements differ, first at %s: %s != %s" % (what, k, len(bad), bad[0], a[tuple(bad[0])], b[tuple(bad[0])]))


# ---- seeded random maps -------------------------------------------------------------------------------------------------------------
SHAPES = {"67x45x3": (67, 45, 3),          # partial tiles in both directions, no alignment, a batch
          "1x1": (1, 1, 2), "33x1": (33, 1, 1), "1x33": (1, 33, 1), "3x2": (3, 2, 1)}
MAXOBJ = {k: w * h for k, (w, h, n) in SHAPES.items()}      # a row for every possible component: every record is compared
DENSITY = (0.3, 0.6, 0.9)                  # 0.6: near the percolation threshold, large ragged components
_IN = {}


def random_map(shape, density):
    """code (n, h, w) uint8 over 0 .. 3 plus some bytes >= 8, code 1 with the given share and code 2 with a fifth of the rest; values
    (n, h, w, 2) f32 with a NaN, an infinity and a 5000 px vector among the foreground.  Images 0 and 2 of a batch of three are equal."""
    key = (shape, density)
    if key not in _IN:
        w, h, n = SHAPES[shape]
        rng = np.random.default_rng(int(density * 10) + 100 * w + h)
        r = rng.random((n, h, w))
        code = np.where(r < density, 1, np.where(r < density + (1 - density) * 0.2, 2, np.where(r < density + (1 - density) * 0.6, 0, 3))).astype(np.uint8)
        code[rng.random((n, h, w)) < 0.03] = 8
        code[rng.random((n, h, w)) < 0.02] = 255
        code[rng.random((n, h, w)) < 0.01] = 9                   # (bit 1 of 9 is set: a code >= 8 is background all the same)
        values = (rng.standard_normal((n, h, w, 2)) * 3).astype(f32)
        values[rng.random((n, h, w)) < 0.05, 0] = np.nan
        values[rng.random((n, h, w)) < 0.05, 1] = np.inf
        values[rng.random((n, h, w)) < 0.05, 0] = -np.inf
        values[rng.random((n, h, w)) < 0.05, 1] = 5000.0
        values[rng.random((n, h, w)) < 0.05, 0] = -4096.0        # just inside
        if n == 3:
            code[2], values[2] = code[0], values[0]
        code.setflags(write=False)
        values.setflags(write=False)
        _IN[key] = (code, values)
    return _IN[key]


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("density", DENSITY)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_random_maps_equal_the_restatement(shape, density, conn):
    code, values = random_map(shape, density)
    for fg in ((1,), (1, 2)):
        for val in (None, values):
            want = R.components_batch(code, R.fg_set(fg), conn, val, 1, MAXOBJ[shape])
            got = gpu(code, fg, conn, val, 1, MAXOBJ[shape])
            assert_same(got, want, "%s d=%.1f conn=%d fg=%s values=%s" % (shape, density, conn, fg, val is not None))
            if shape == "67x45x3":
                # equal images of a batch get equal records; nothing joins across images (every label lies inside its own image)
                for k in KEYS:
                    assert np.array_equal(got[k][0], got[k][2]), k
                assert got["labels"].max() < 67 * 45 and not np.array_equal(got["labels"][0], got["labels"][1])
                assert got["stats"][:, 1].min() > 0


# ---- structured maps at 200 x 150 x 2 ------------------------------------------------------------------------------------------------
W, H = 200, 150


def spiral(w, h):
    """a one-pixel-wide rectangular spiral from the top-left corner inwards, one pixel of background between its turns"""
    a = np.zeros((h, w), np.uint8)
    x = y = d = 0
    a[0, 0] = 1
    inside = lambda x, y: 0 <= x < w and 0 <= y < h
    while True:
        dx, dy = ((1, 0), (0, 1), (-1, 0), (0, -1))[d]
        moved = 0
        while inside(x + dx, y + dy) and not a[y + dy, x + dx] and not (inside(x + 2 * dx, y + 2 * dy) and a[y + 2 * dy, x + 2 * dx]):
            x, y = x + dx, y + dy
            a[y, x] = 1
            moved += 1
        if moved < 2:
            return a
        d = (d + 1) % 4


def structured(name):
    if name not in _IN:
        tw, th = _O().TILE
        assert tw <= 64 and th <= 64 and W > 3 * tw and H > 3 * th
        yy, xx = np.mgrid[0:H, 0:W]
        if name == "spiral":
            a = spiral(W, H)
        elif name == "comb":                # teeth that join only in the last row
            a = np.zeros((H, W), np.uint8)
            a[:, ::2] = 1
            a[H - 1, :] = 1
        elif name == "checkerboard":
            a = ((xx + yy) % 2 == 0).astype(np.uint8)
        elif name == "all_foreground":
            a = np.ones((H, W), np.uint8)
        elif name == "all_background":
            a = np.zeros((H, W), np.uint8)
        if name == "corner":
            # image 0: two blobs that meet only at the tile corner (tw, th), along the main diagonal; image 1: along the other
            # diagonal at the corner (2 tw, th)
            code = np.zeros((2, H, W), np.uint8)
            code[0, th - 4:th, tw - 5:tw] = 1
            code[0, th:th + 6, tw:tw + 7] = 1
            code[1, th - 3:th, 2 * tw:2 * tw + 5] = 1
            code[1, th:th + 4, 2 * tw - 6:2 * tw] = 1
        else:
            code = np.stack([a, a[:, ::-1]])          # the same figure mirrored: other roots, other merge directions
        rng = np.random.default_rng(3)
        values = rng.integers(-2000, 2001, (2, H, W, 2)).astype(f32) / f32(8)
        code.setflags(write=False)
        values.setflags(write=False)
        _IN[name] = (code, values)
    return _IN[name]


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("name", ["spiral", "comb", "checkerboard", "all_foreground", "all_background", "corner"])
def test_structured_maps_equal_the_restatement(name, conn):
    code, values = structured(name)
    want = R.components_batch(code, 2, conn, values, 1, 256)
    got = gpu(code, (1,), conn, values, 1, 256)
    assert_same(got, want, "%s conn=%d" % (name, conn))
    comps = got["stats"][:, 1].tolist()
    if name in ("spiral", "comb", "all_foreground"):
        assert comps == [1, 1] and got["objects"][:, 0, 1].tolist() == got["stats"][:, 0].tolist()
    elif name == "checkerboard":
        assert comps == ([1, 1] if conn == 8 else [H * W // 2] * 2)
    elif name == "all_background":
        assert comps == [0, 0] and not got["objects"].any() and (got["ids"] == -1).all() and not got["stats"].any()
    else:
        assert comps == ([1, 1] if conn == 8 else [2, 2])


# ---- min_area and max_objects ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["checkerboard", "random"])
def test_min_area_and_max_objects(which):
    if which == "checkerboard":
        code, values = structured("checkerboard")
        min_area = 1
    else:
        code, values = random_map("67x45x3", 0.3)
        min_area = 3
    full = gpu(code, (1,), 4, values, min_area, 1000)
    assert_same(full, R.components_batch(code, 2, 4, values, min_area, 1000), which + " full")
    got = gpu(code, (1,), 4, values, min_area, 5)
    assert_same(got, R.components_batch(code, 2, 4, values, min_area, 5), which + " 5")
    assert np.array_equal(got["objects"], full["objects"][:, :5])                   # the first five in raster order
    assert np.array_equal(got["stats"][:, :3], full["stats"][:, :3]) and got["stats"][:, 3].tolist() == [5] * len(code)
    assert (got["stats"][:, 2] > 5).all() and np.array_equal(got["labels"], full["labels"])
    assert np.array_equal(got["ids"], np.where(full["ids"] < 5, full["ids"], -1)) and (got["ids"] == -1).sum() > (full["ids"] == -1).sum()


# ---- guards, repeatability, streams ----------------------------------------------------------------------------------------------------
def raw(code, values, conn, min_area, max_objects, stream=None, off=1):
    """fotg_label_components into slices that start `off` elements into larger, pre-filled tensors -> (outputs, guards untouched)"""
    import flowonthego_amd as F
    L = F.lib()
    n, h, w = code.shape
    sizes = dict(objects=(n * max_objects * 11, torch.int64), labels=(n * h * w, torch.int32), ids=(n * h * w, torch.int32), stats=(n * 4, torch.int64))
    big = {k: torch.full((s + 2 * off,), -77, dtype=dt, device="cuda") for k, (s, dt) in sizes.items()}
    view = {k: big[k][off:off + sizes[k][0]] for k in big}
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    dcode, dval = dev(code), None if values is None else dev(values)
    torch.cuda.synchronize()
    st = L.fotg_label_components(0, n, p(dcode), w, h, 2, conn, p(dval), min_area, max_objects, p(view["labels"]), p(view["ids"]),
                                 p(view["objects"]), p(view["stats"]), C.c_void_p(stream.cuda_stream) if stream is not None else None)
    assert st == 0
    (stream or torch.cuda.current_stream()).synchronize()
    torch.cuda.synchronize()
    guards = all((big[k][:off] == -77).all().item() and (big[k][off + sizes[k][0]:] == -77).all().item() for k in big)
    shapes = dict(objects=(n, max_objects, 11), labels=(n, h, w), ids=(n, h, w), stats=(n, 4))
    return {k: view[k].cpu().numpy().reshape(shapes[k]) for k in big}, guards


def test_guards_repeatability_and_streams():
    code, values = random_map("67x45x3", 0.6)
    want = R.components_batch(code, 2, 8, values, 2, 40)
    a, guards = raw(code, values, 8, 2, 40)
    assert guards
    assert_same(a, want, "raw")
    b, guards = raw(code, values, 8, 2, 40)
    assert guards
    assert_same(b, a, "second run")
    s = torch.cuda.Stream()
    c, guards = raw(code, values, 8, 2, 40, stream=s)
    assert guards
    assert_same(c, a, "non-default stream")
    # through the module on a stream of torch's, the outputs one by one
    O = _O()
    with torch.cuda.stream(s):
        only = O.label_components(dev(code), (1,), 8, dev(values), 2, 40)
        single = O.label_components(dev(code[1]), (1,), 8, dev(values[1]), 2, 40, ids=True)
    s.synchronize()
    assert only.cpu().numpy().tobytes() == a["objects"].tobytes()
    assert single[0].shape == (40, 11) and single[1].shape == (45, 67)
    assert np.array_equal(single[0].cpu().numpy(), a["objects"][1]) and np.array_equal(single[1].cpu().numpy(), a["ids"][1])


# ---- moving objects ----------------------------------------------------------------------------------------------------------------------
RECTS = (((40, 30, 95, 69), (12.0, -9.0)), ((200, 100, 259, 147), (-10.0, 11.0)))      # (x0, y0, x1, y1) inclusive, the offset
P_BG = (0.01, -0.005, 1.5, 0.004, 0.006, -2.0)


def moving_scene():
    w, h = 320, 192
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    flow = np.stack([P_BG[0] * xs + P_BG[1] * ys + P_BG[2], P_BG[3] * xs + P_BG[4] * ys + P_BG[5]], -1).astype(f32)
    for (x0, y0, x1, y1), off in RECTS:
        flow[y0:y1 + 1, x0:x1 + 1] = off
    return flow


def test_moving_objects_finds_the_two_rectangles():
    import flowonthego_amd as F
    flow = moving_scene()
    dflow = dev(flow)
    params, objects, ids, stats = F.moving_objects(dflow, ids=True, stats=True)
    prm = F.fit_motion(dflow)
    torch.cuda.synchronize()
    assert params.cpu().numpy().tobytes() == prm.cpu().numpy().tobytes()
    fit = M.fit(flow, None, 2, 3, 1.0)
    assert params.cpu().numpy().tobytes() == fit["params"].tobytes()
    want = R.components(fit["code"], 2, 8, fit["residual"], 64, 256)
    got = dict(objects=objects.cpu().numpy(), ids=ids.cpu().numpy(), stats=stats.cpu().numpy())
    for k in got:
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), k
    assert got["stats"][2] == 2 and got["stats"][3] == 2 and not got["objects"][2:].any()            # exactly two objects
    summ = F.object_summary(objects).cpu().numpy()
    assert np.array_equal(summ[:2], R.summary(want["objects"])[:2]) and np.isnan(summ[2:]).all()
    for row, ((x0, y0, x1, y1), off) in enumerate(RECTS):
        o = got["objects"][row]
        assert o[2:6].tolist() == [x0, y0, x1, y1] and o[1] == o[8] == (x1 - x0 + 1) * (y1 - y0 + 1)
        # the mean motion is the offset minus the background at the centroid (the background is affine): the fixed point rounds a
        # pixel's residual by at most 1/512 px; a noiseless background is fitted far closer than the 1/512 px left to this bound
        cx, cy = (x0 + x1) / 2.0, (y0 + y1) / 2.0
        true = (off[0] - (P_BG[0] * cx + P_BG[1] * cy + P_BG[2]), off[1] - (P_BG[3] * cx + P_BG[4] * cy + P_BG[5]))
        print("object %d: mean motion %.5f %.5f, true %.5f %.5f" % (row, summ[row, 2], summ[row, 3], true[0], true[1]))
        assert summ[row, 0] == cx and summ[row, 1] == cy
        assert abs(summ[row, 2] - true[0]) <= 1 / 256 and abs(summ[row, 3] - true[1]) <= 1 / 256


def test_ofclass_moving_objects_equals_the_module_functions(natural_images):
    import flowonthego_amd as F
    from flowonthego_amd.oflow import OFClass
    frames, _ = M.jittered_crops(natural_images["road_HD"], T=3, patch=True)
    T, (h, w) = len(frames) - 1, frames.shape[1:]
    dfr = dev(frames)
    for bidir in (False, True):
        op = F.operating_point(2, w, 1)
        op.bidir = bidir
        o = OFClass(op, F.img_params(width=w, height=h), max_batch=T)
        got = o.moving_objects(dfr, min_area=16, max_objects=32, ids=True, stats=True)
        if bidir:
            fw, bw = o.calc_sequence_bidirectional(dfr)
            mask = o.upsample_crop_fb_check(fw, bw)[0]
        else:
            fw, mask = o.calc_sequence(dfr), None
        params, code, res = o.upsample_crop_fit_motion(fw, mask, code=True, residual=True)
        want = (params,) + F.label_components(code, (1,), 8, res, 16, 32, ids=True, stats=True)
        torch.cuda.synchronize()
        assert len(got) == 4 and got[0].shape == (T, 6) and got[1].shape == (T, 32, 11) and got[2].shape == (T, h, w) and got[3].shape == (T, 4)
        for a, b in zip(got, want):
            assert a.dtype == b.dtype and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
        # and the labelling of these real codes equals the restatement
        ref = R.components_batch(code.cpu().numpy(), 2, 8, res.cpu().numpy(), 16, 32)
        for k, a in zip(("objects", "ids", "stats"), got[1:]):
            assert a.cpu().numpy().tobytes() == ref[k].tobytes(), k
        print("bidir=%s: %s components, %s kept" % (bidir, got[3][:, 1].tolist(), got[3][:, 2].tolist()))
        o.close()
    op = F.operating_point(2, 64, 1)
    op.depth_mode = True
    od = OFClass(op, F.img_params(width=64, height=48), max_batch=2)
    with pytest.raises(F.FotgError):                             # a depth-mode context is refused like the motion fit
        od.moving_objects(dfr)
    od.close()
