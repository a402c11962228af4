"""The binary morphology without a GPU: the numpy restatement tests/morph_ref.py equals an independent per-pixel loop on tiny maps
and obeys the algebra of the definition for every radius 0 .. 8 -- erosion is the complement of the dilation of the complement,
an opening shrinks and a closing grows, both are idempotent, a single pixel dilates into the disc, a full frame does not erode,
radius 0 is the map of the foreground set, the statistics add up --; the foreground composition with open = close = 0 is today's
foreground_objects; the Python forms refuse bad arguments before anything is launched."""
import numpy as np
import pytest

import morph_ref as R

RADII = list(range(9))


def per_pixel(X, op, r):
    """the definition, one pixel and one neighbour at a time"""
    h, w = X.shape
    out = np.zeros((h, w), bool)
    for y in range(h):
        for x in range(w):
            vals = [X[yy, xx] for yy in range(max(0, y - r), min(h, y + r + 1)) for xx in range(max(0, x - r), min(w, x + r + 1))
                    if (xx - x) ** 2 + (yy - y) ** 2 <= r * r]
            out[y, x] = any(vals) if op == "dilate" else all(vals)
    return out


def random_maps(seed, n=3, h=23, w=31):
    rng = np.random.default_rng(seed)
    dens = (0.5, 0.08, 0.92)
    return np.stack([(rng.random((h, w)) < dens[i % 3]) for i in range(n)])


@pytest.mark.parametrize("r", [0, 1, 2, 3, 5, 8])
def test_restatement_equals_the_per_pixel_loop(r):
    rng = np.random.default_rng(r)
    for h, w, p in ((7, 9, 0.5), (5, 3, 0.2), (1, 1, 1.0), (1, 17, 0.7), (12, 11, 0.85)):
        X = rng.random((h, w)) < p
        for op, fn in (("dilate", R.dilate), ("erode", R.erode)):
            assert np.array_equal(fn(X, r), per_pixel(X, op, r)), (h, w, op, r)


@pytest.mark.parametrize("r", RADII)
def test_algebra_of_the_definition(r):
    X = random_maps(10 + r)
    er, di = R.erode(X, r), R.dilate(X, r)
    assert np.array_equal(er, ~R.dilate(~X, r))                       # the duality, exactly, border included
    assert not (er & ~X).any() and not (X & ~di).any()
    op, cl = R.dilate(er, r), R.erode(di, r)
    assert not (op & ~X).any() and not (X & ~cl).any()                # open is a subset of X, X of close
    assert np.array_equal(R.dilate(R.erode(op, r), r), op) and np.array_equal(R.erode(R.dilate(cl, r), r), cl)       # idempotent
    # through the public form of the restatement, with its statistics
    x8 = X.astype(np.uint8) * 3
    for name, want in (("erode", er), ("dilate", di), ("open", op), ("close", cl)):
        out, st = R.morphology(x8, name, r)
        assert out.dtype == np.uint8 and np.array_equal(out, want.astype(np.uint8)) and st.shape == (3, 4) and st.dtype == np.int64
        assert (st[:, 0] == X.sum((1, 2))).all() and (st[:, 1] == want.sum((1, 2))).all()
        assert (st[:, 1] == st[:, 0] + st[:, 2] - st[:, 3]).all()     # the statistics add up
        assert not st[:, 2 if name in ("erode", "open") else 3].any()
    if r == 0:
        for name in R.STAGES:
            assert np.array_equal(R.morphology(x8, name, 0)[0], X.astype(np.uint8))


@pytest.mark.parametrize("r", RADII)
def test_a_single_pixel_dilates_into_the_disc_and_a_full_frame_stays_full(r):
    X = np.zeros((21, 25), bool)
    X[10, 12] = True
    want = np.zeros_like(X)
    for dx, dy in R.disc(r):
        want[10 + dy, 12 + dx] = True
    assert np.array_equal(R.dilate(X, r), want) and want.sum() == len(R.disc(r))
    assert (0, r) in R.disc(r) and (r, 0) in R.disc(r) and all(dx * dx + dy * dy <= r * r for dx, dy in R.disc(r))
    assert len(R.disc(r)) == (1, 5, 13, 29, 49, 81, 113, 149, 197)[r]             # the lattice points of the disc
    # at a corner only the part inside the frame
    C = np.zeros((6, 7), bool)
    C[0, 0] = True
    assert R.dilate(C, r).sum() == sum(1 for dx, dy in R.disc(r) if 0 <= dx < 7 and 0 <= dy < 6)
    for h, w in ((1, 1), (3, 5), (21, 25)):
        assert R.erode(np.ones((h, w), bool), r).all()                # the border does not erode
        assert not R.dilate(np.zeros((h, w), bool), r).any()
    # an opening keeps the disc of its radius and deletes the smaller one
    if r > 0:
        assert np.array_equal(R.dilate(R.erode(want, r), r), want)
        small = R.dilate(X, r - 1)
        assert not R.dilate(R.erode(small, r), r).any()


def test_the_foreground_set():
    x = np.arange(256, dtype=np.uint8).reshape(16, 16)
    assert np.array_equal(R.fg_map(x), x != 0)
    assert np.array_equal(R.fg_map(x, (1, 4)), (x == 1) | (x == 4))
    assert np.array_equal(R.fg_map(x, (0,)), x == 0)
    out, st = R.morphology(x, "dilate", 0, fg=(1, 4))
    assert out.sum() == 2 and st.tolist() == [2, 2, 0, 0]
    out, st = R.clean_mask(np.stack([x, x]), 0, 0, fg=(7,))
    assert out.shape == (2, 16, 16) and out.sum() == 2 and st.shape == (2, 2, 4) and st[0].tolist() == [[1, 1, 0, 0], [1, 1, 0, 0]]


def test_cleaning_deletes_speckle_and_fills_pin_holes():
    x = np.zeros((40, 50), np.uint8)
    x[10:30, 10:35] = 1
    x[15, 20] = 0                                                     # a pin-hole
    x[20:22, 25] = 0
    x[3, 3] = x[36, 44] = x[5, 40] = 1                                # speckle
    out, st = R.clean_mask(x, 1, 2)
    want = np.zeros_like(x)
    want[10:30, 10:35] = 1
    want[[10, 10, 29, 29], [10, 34, 10, 34]] = 0                      # the opening by the 5-pixel cross rounds the corners
    assert np.array_equal(out, want)
    assert st[0].tolist() == [x.sum(), x.sum() - 3 - 4, 0, 3 + 4] and st[1].tolist() == [x.sum() - 7, want.sum(), 1 + 2, 0]


def test_the_composition_without_cleaning_is_todays_foreground_objects():
    """open = close = 0 takes today's path; the cleaned path at radius 0 -- the 0 / 1 map of the codes (1, 4), components of (1,) --
    finds the same objects, ids and confirmations: cleaning changes the map and nothing else"""
    import objects_ref as OR
    rng = np.random.default_rng(5)
    code = rng.choice(np.arange(5, dtype=np.uint8), size=(2, 24, 30), p=(0.55, 0.3, 0.03, 0.02, 0.1))
    code[0, 4:12, 5:15] = 1
    code[0, 6, 8] = 4
    code[1, 10:20, 3:9] = 1                                            # weak throughout
    code[1, 9, 2:10] = code[1, 20, 2:10] = 0
    code[1, 9:21, 2] = code[1, 9:21, 9] = 0
    ev = np.zeros((2, 24, 30, 2), np.float32)
    ev[..., 0] = code == 4
    ev[..., 1] = np.where((code == 1) | (code == 4), 9.25, 0)
    today = OR.components_batch(code, OR.fg_set((1, 4)), 8, ev, min_area=4, max_objects=16)
    ob, ids, conf = R.foreground_objects(code, ev, 8, 4, 16)
    assert np.array_equal(ob, today["objects"]) and np.array_equal(ids, today["ids"]) and np.array_equal(conf, today["objects"][..., 9] > 0)
    ident, _ = R.clean_mask(code, 0, 0, fg=(1, 4))
    assert np.array_equal(ident, ((code == 1) | (code == 4)).astype(np.uint8))
    via = OR.components_batch(ident, OR.fg_set((1,)), 8, ev, min_area=4, max_objects=16)
    assert np.array_equal(via["objects"], today["objects"]) and np.array_equal(via["ids"], today["ids"])
    assert conf.any() and not conf.all()
    # with cleaning: the components are those of the cleaned map, and a pixel the closing adds brings no strong evidence
    ob2, ids2, conf2 = R.foreground_objects(code, ev, 8, 4, 16, open=1, close=2)
    cleaned, _ = R.clean_mask(code, 1, 2, fg=(1, 4))
    assert np.array_equal(ids2 >= 0, (cleaned == 1) & (ids2 >= 0)) and ob2[..., 9].sum() <= 256 * (code == 4).sum()
    assert not np.array_equal(ids2, ids)


class _Fake:
    """stands where a tensor is expected"""


def test_python_refusals_launch_nothing():
    import torch
    from flowonthego_amd import FotgError
    from flowonthego_amd import morph
    assert morph.OPS == ("erode", "dilate", "open", "close") and morph.STATS == ("before", "after", "added", "removed") and morph.MAX_RADIUS == 8
    m = torch.zeros((4, 5), dtype=torch.uint8)                        # a host tensor: refused last, so everything before it is decided first
    for bad in (dict(op="grow"), dict(radius=9), dict(radius=-1), dict(radius=1.0), dict(radius=True), dict(fg=(8,)), dict(fg=()), dict(fg=(-1,)),
                dict(fg="x"), dict(mask=_Fake()), dict(mask=m), dict(mask=m.float())):
        kw = dict(dict(mask=m, op="open", radius=1), **bad)
        with pytest.raises(FotgError):
            morph.morphology(**kw)
    for bad in (dict(open=9), dict(close=-1), dict(open=1.5), dict(fg=(9,)), dict()):
        with pytest.raises(FotgError):
            morph.clean_mask(m, **bad)
    for stages in ([], [("erode", 1)] * 3, [("open", 1)], [("erode", 9)], "x", [("erode",)]):
        with pytest.raises(FotgError):
            morph.chain(m, stages)
    with pytest.raises(FotgError):
        morph.chain(m, [("erode", 1)], out=False, stats=False)
    from flowonthego_amd.subtract import foreground_objects
    with pytest.raises(FotgError):
        foreground_objects(m, None, open=9)
    with pytest.raises(FotgError):
        foreground_objects(m, None, close=-1)
