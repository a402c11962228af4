"""The binary morphology on the GPU: fotg_morph equals the numpy restatement tests/morph_ref.py byte for byte in out and stats, for
the four operations at the radii 0, 1, 2, 5, 8, for two-stage chains up to a halo of 16 with mixed operations and radii, and for
both forms of the foreground set; on patterns placed against the geometry of the 64 x 64 tile (single set and single clear pixels
at tile corners and frame borders and exactly r, r + 1, r1 + r2 and r1 + r2 + 1 pixels from a tile edge on both axes and both
sides, empty, full, noise, lines, the disc an opening keeps and the one it deletes), on a frame that crosses the tile in both
directions by an odd amount, whose width is no multiple of 4, and on frames smaller than the halo; a dilation is grow_mask; single
and batched calls, each output alone and repeated calls give the same bytes; an output that is not aligned takes the scalar
stores and writes nothing outside; OFClass.foreground(open=, close=) is the documented composition and without them what it was;
the tool writes what the call returns."""
import ctypes as C

import numpy as np
import pytest
import torch

import morph_ref as R
from host_checks import read_png_rgb, run_cli
from test_gpu_subtract import host
from test_gpu_warp import dev, make_ctx, same_bits

pytestmark = pytest.mark.gpu

TW, TH = 64, 64                    # the kernel's tile
BIG = (139, 150)                   # h, w: two tiles and 11 rows, two tiles and 22 columns; 150 is no multiple of 4
SMALL = [(3, 5), (1, 1), (1, 17)]
OPS = ("erode", "dilate", "open", "close")
RADII = (0, 1, 2, 5, 8)
CHAINS = [(("erode", 8), ("dilate", 8)), (("dilate", 8), ("erode", 8)), (("dilate", 5), ("dilate", 3)), (("erode", 2), ("erode", 7)),
          (("erode", 1), ("dilate", 3)), (("dilate", 8), ("erode", 2)), (("erode", 0), ("dilate", 8)), (("dilate", 3), ("erode", 0)),
          (("erode", 8), ("erode", 8)), (("dilate", 8), ("dilate", 8))]


def disc_at(h, w, cx, cy, r):
    yy, xx = np.mgrid[:h, :w]
    return (xx - cx) ** 2 + (yy - cy) ** 2 <= r * r


def tile_masks(h, w, ra, rb):
    """one map per pattern, as bool.  Single pixels at the corners of the 64 x 64 tiles and of the frame; each frame border; pixels
    exactly d = ra, ra + 1, ra + rb and ra + rb + 1 away from the first tile edge on both axes, on either side of it; lines one
    pixel wide; the disc of radius ra and the one of radius ra - 1; noise; nothing; everything -- and the complement of each, for
    the single clear pixels"""
    pats = []
    m = np.zeros((h, w), bool)
    for y in (0, TH - 1, TH, 2 * TH - 1, 2 * TH, h - 1):
        for x in (0, TW - 1, TW, 2 * TW - 1, 2 * TW, w - 1):
            if y < h and x < w:
                m[y, x] = True
    pats.append(m)
    for sl in ((0, slice(None)), (h - 1, slice(None)), (slice(None), 0), (slice(None), w - 1)):
        m = np.zeros((h, w), bool)
        m[sl] = True
        pats.append(m)
    for d in sorted({ra, ra + 1, ra + rb, ra + rb + 1}):
        m = np.zeros((h, w), bool)
        # d beyond the tile's last / first column and row, from inside and from outside
        for x, y in ((TW - 1 + d, 5), (TW - d, h - 6), (10, TH - 1 + d), (w - 10, TH - d), (2 * TW - 1 - d, TH + 3), (2 * TW + d, 2 * TH - d)):
            if 0 <= x < w and 0 <= y < h:
                m[y, x] = True
        pats.append(m)
    m = np.zeros((h, w), bool)
    m[h // 2, :] = True                                               # a line one pixel wide: an opening deletes it from r = 1 on
    m[:, min(w - 1, TW + 1)] = True
    pats.append(m)
    m = np.zeros((h, w), bool)
    idx = np.arange(min(h, w))
    m[idx, idx] = True                                                # a diagonal
    pats.append(m)
    pats.append(disc_at(h, w, TW - 2, TH - 1, ra) | disc_at(h, w, w - 20, h - 12, max(ra - 1, 0)))
    rng = np.random.default_rng(h * 1000 + w + 10 * ra + rb)
    pats.append(rng.random((h, w)) < 0.5)
    pats.append(rng.random((h, w)) < 0.03)
    pats.append(np.zeros((h, w), bool))
    pats.append(np.ones((h, w), bool))
    pats = np.stack(pats)
    return np.concatenate((pats, ~pats[:-2]))


def as_bytes(P, fg, seed=0):
    """the bool patterns as a byte map whose set pixels are those of P under fg: any non-zero bytes, or the codes of fg among
    other codes and bytes of 8 and more, which belong to no set"""
    rng = np.random.default_rng(seed)
    if fg is None:
        return np.where(P, rng.choice(np.array([1, 2, 8, 128, 255], np.uint8), P.shape), 0).astype(np.uint8)
    others = np.array([c for c in (0, 1, 2, 3, 4, 5, 6, 7) if c not in fg] + [8, 9, 130, 255], np.uint8)
    return np.where(P, rng.choice(np.array(fg, np.uint8), P.shape), rng.choice(others, P.shape)).astype(np.uint8)


def gpu_chain(x, stages, fg=None):
    from flowonthego_amd.morph import chain
    out, stats = chain(dev(x), list(stages), fg=fg, out=True, stats=True)
    torch.cuda.synchronize()
    return host(out), host(stats)


def assert_chain(x, stages, fg, what):
    got, want = gpu_chain(x, stages, fg), R.chain(x, stages, fg)
    assert got[0].dtype == np.uint8 and got[1].dtype == np.int64 and got[0].shape == x.shape
    bad = np.argwhere(got[0] != want[0])
    assert len(bad) == 0, (what, stages, fg, len(bad), bad[:5])
    assert np.array_equal(got[1], want[1]), (what, stages, fg, got[1][:3], want[1][:3])
    return got


@pytest.mark.parametrize("fg", [None, (1, 4)])
@pytest.mark.parametrize("r", RADII)
@pytest.mark.parametrize("op", OPS)
def test_the_four_operations_equal_the_restatement(op, r, fg):
    import flowonthego_amd as F
    rb = r if op in ("open", "close") else 0
    P = tile_masks(BIG[0], BIG[1], r, rb)
    x = as_bytes(P, fg, r)
    want, wstats = R.morphology(x, op, r, fg)
    out, stats = F.morphology(dev(x), op, r, fg=fg, stats=True)
    torch.cuda.synchronize()
    bad = np.argwhere(host(out) != want)
    assert len(bad) == 0, (len(bad), bad[:5])
    assert np.array_equal(host(stats), wstats)
    assert same_bits(F.morphology(dev(x), op, r, fg=fg), out)
    k_disc = 5 + len({r, r + 1, r + rb, r + rb + 1}) + 2              # the map with the two discs
    if op == "open" and r > 0:                                         # the opening keeps the disc of its radius and deletes the smaller one
        assert np.array_equal(want[k_disc].astype(bool), disc_at(BIG[0], BIG[1], TW - 2, TH - 1, r))
    if r == 0:
        assert np.array_equal(want, P.astype(np.uint8))


@pytest.mark.parametrize("fg", [None, (1, 4)])
@pytest.mark.parametrize("stages", CHAINS)
def test_two_stage_chains_equal_the_restatement(stages, fg):
    P = tile_masks(BIG[0], BIG[1], stages[0][1], stages[1][1])
    assert_chain(as_bytes(P, fg, 3), stages, fg, "big")


@pytest.mark.parametrize("h,w", SMALL + [(33, 65), (TH, TW), (2 * TH + 1, 4 * TW - 1)])
def test_small_frames_and_frames_at_the_tile_size(h, w):
    rng = np.random.default_rng(h * 31 + w)
    P = np.stack([rng.random((h, w)) < p for p in (0.5, 0.1, 0.9)] + [np.zeros((h, w), bool), np.ones((h, w), bool)])
    P[1, 0, 0] = P[1, h - 1, w - 1] = True
    P[2, 0, w - 1] = P[2, h - 1, 0] = False
    for fg in (None, (0, 7)):
        x = as_bytes(P, fg, h)
        for op in ("erode", "dilate"):
            for r in (1, 8):
                assert_chain(x, ((op, r),), fg, (h, w))
        for stages in CHAINS[:4] + CHAINS[8:]:
            got = assert_chain(x, stages, fg, (h, w))
        assert not got[0][3].any() and got[0][4].all() and got[1][4].tolist() == [h * w, h * w, 0, 0]


@pytest.mark.parametrize("r", range(9))
def test_a_dilation_is_grow_mask(r):
    import flowonthego_amd as F
    rng = np.random.default_rng(r)
    for shape in ((3, 37, 131), (5, 3), (40, 200)):
        x = dev((rng.random(shape) < 0.02).astype(np.uint8) * 200)
        assert same_bits(F.morphology(x, "dilate", r), F.grow_mask(x, r)), shape


def test_each_output_alone_single_calls_and_repeats():
    from flowonthego_amd.morph import chain, clean_mask, morphology
    P = tile_masks(71, 131, 3, 2)[:12]
    x = dev(as_bytes(P, None, 1))
    stages = [("erode", 3), ("dilate", 2)]
    full = chain(x, stages, out=True, stats=True)
    for _ in range(3):
        again = chain(x, stages, out=True, stats=True)
        assert same_bits(again[0], full[0]) and same_bits(again[1], full[1])           # the same bytes every time, stats included
    o = chain(x, stages, out=True, stats=False)
    s = chain(x, stages, out=False, stats=True)
    assert isinstance(o, torch.Tensor) and isinstance(s, torch.Tensor) and same_bits(o, full[0]) and same_bits(s, full[1])
    for i in range(len(P)):
        one = chain(x[i], stages, out=True, stats=True)
        assert one[0].shape == (71, 131) and one[1].shape == (4,) and same_bits(one[0], full[0][i]) and same_bits(one[1], full[1][i])
    # the input is left as it was, and a view that is not contiguous is taken as its values
    assert same_bits(x, dev(as_bytes(P, None, 1)))
    assert same_bits(morphology(x[:, ::2, 1:], "close", 2), morphology(x[:, ::2, 1:].contiguous(), "close", 2))
    # clean_mask is the composition, with either part left out too
    for a, b in ((1, 2), (0, 2), (2, 0), (0, 0), (8, 8)):
        out, st = clean_mask(x, a, b, stats=True)
        want, wst = R.clean_mask(host(x), a, b)
        assert np.array_equal(host(out), want) and np.array_equal(host(st), wst), (a, b)
        assert same_bits(clean_mask(x, a, b), out)
        assert same_bits(out, morphology(morphology(x, "open", a), "close", b))
    one, st1 = clean_mask(x[0], 1, 2, stats=True)
    assert one.shape == (71, 131) and st1.shape == (2, 4) and same_bits(one, clean_mask(x, 1, 2)[0])


def test_an_output_that_is_not_aligned_takes_the_scalar_stores():
    """out at every offset from an 8-byte boundary: the same bytes, and nothing written outside"""
    from flowonthego_amd import lib
    from flowonthego_amd._args import _ptr, _stream
    for h, w in ((67, 136), (21, 83)):                                 # rows of 136 bytes keep the offset; rows of 83 change it row by row
        n = 2
        P = tile_masks(h, w, 2, 1)[[0, 9]]
        x = dev(as_bytes(P, None, 2))
        want, wstats = R.chain(host(x), [("dilate", 2), ("erode", 1)])
        size = n * h * w
        ops, radii = (C.c_int * 2)(1, 0), (C.c_int * 2)(2, 1)
        for off in range(9):
            buf = torch.full((size + 64,), 77, dtype=torch.uint8, device="cuda")
            stats = torch.full((n, 4), -1, dtype=torch.int64, device="cuda")
            o = buf[off:off + size]
            assert lib().fotg_morph(0, n, _ptr(x), w, h, 0, 2, ops, radii, _ptr(o), _ptr(stats), _stream(torch.device("cuda", 0))) == 0
            torch.cuda.synchronize()
            assert np.array_equal(host(o).reshape(n, h, w), want), (h, w, off)
            assert (buf[:off] == 77).all() and (buf[off + size:] == 77).all() and np.array_equal(host(stats), wstats)


# ---- the pipeline ------------------------------------------------------------------------------------------------------------------
def test_ofclass_foreground_with_cleaning_is_the_documented_composition(natural_images):
    import flowonthego_amd as F
    import motion_ref as M
    from flowonthego_amd.erase import ofc_remove_objects
    frames_np, _ = M.jittered_crops(natural_images["road_HD"], T=4, patch=True)
    frames = dev(frames_np)
    K, h, w = frames_np.shape
    o = make_ctx(2, w, h, max_batch=K - 1)
    plain = o.foreground(frames, min_area=32)
    zeros = o.foreground(frames, min_area=32, open=0, close=0)
    torch.cuda.synchronize()
    for x, y in zip(plain, zeros):
        assert same_bits(x, y)                                         # with zeros every byte is what it is without them
    mask, objects, confirmed, plate, code = o.foreground(frames, min_area=32, open=1, close=2)
    # call for call: the code map is the one without cleaning; its set (1, 4) opened, then closed; the components of the cleaned map
    assert same_bits(code, plain[4]) and same_bits(plate, plain[3])
    _, pcode, _ = o.background(frames)
    params = F.upsample_crop_fit_motion(o, o.calc_sequence(frames), None, "affine", code=True)[0]
    back = F.frame_motions(F.plate_motions(params, 0))
    code2, evidence = F.subtract_background(frames, plate, motions=back, plate_code=pcode, code=True, evidence=True)
    cleaned = F.morphology(F.morphology(code2, "open", 1, fg=(1, 4)), "close", 2)
    ob2, ids2 = F.label_components(cleaned, fg=(1,), values=evidence, min_area=32, max_objects=256, ids=True)
    conf2 = ob2[..., 9] > 0
    torch.cuda.synchronize()
    assert same_bits(code2, code) and same_bits(objects, ob2) and same_bits(confirmed, conf2) and same_bits(mask, F.foreground_mask(ids2, conf2))
    assert np.array_equal(host(cleaned), R.clean_mask(host(code), 1, 2, fg=(1, 4))[0])
    ob3, ids3, conf3 = F.foreground_objects(code, evidence, 8, 32, 256, open=1, close=2)
    assert same_bits(ob3, objects) and same_bits(conf3, confirmed)
    # the cleaning does something on this scene, and the confirmed objects lie inside the cleaned map
    assert mask.any() and not same_bits(mask, plain[0]) and not (host(mask) & ~host(cleaned).astype(bool)).any()
    # the same reaches the removal, whose method keeps its signature
    clean, rcode, rmask, rplate = ofc_remove_objects(o, frames, min_area=32, open=1, close=2)
    want = F.remove_objects(frames, plate, mask, motions=back, plate_code=pcode, grow=2, feather=3, dst=True, code=True)
    assert same_bits(rmask, mask) and same_bits(clean, want[0]) and same_bits(rcode, want[1])
    c0 = ofc_remove_objects(o, frames, min_area=32)
    c1 = o.remove_objects(frames, min_area=32)
    for x, y in zip(c0, c1):
        assert same_bits(x, y)
    for bad in (dict(open=9), dict(close=-1), dict(open=1.5)):
        with pytest.raises(F.FotgError):
            o.foreground(frames, **bad)
    o.close()


# ---- the tool ----------------------------------------------------------------------------------------------------------------------
def test_cli_writes_what_the_call_returns(tmp_path):
    import flowonthego_amd as F
    from host_checks import gray_png_bytes
    rng = np.random.default_rng(3)
    x = np.zeros((50, 77), np.uint8)
    x[10:35, 12:60] = 1
    x[rng.random(x.shape) < 0.04] ^= 1
    code = np.where(x == 1, rng.choice(np.array([1, 4], np.uint8), x.shape), rng.choice(np.array([0, 2, 3], np.uint8), x.shape)).astype(np.uint8)
    npy, png, out = (str(tmp_path / n) for n in ("m.npy", "m.png", "o.png"))
    np.save(npy, code)
    open(png, "wb").write(gray_png_bytes(x * np.uint8(200)))
    white = lambda m: np.broadcast_to((m * np.uint8(255))[..., None], m.shape + (3,))
    run = run_cli("clean_mask", [npy, out, "--fg", "1,4"])
    assert run.returncode == 0, run.stderr
    want, st = F.clean_mask(dev(code), 1, 2, fg=(1, 4), stats=True)
    want, st = host(want), host(st)
    assert np.array_equal(read_png_rgb(out), white(want)) and np.array_equal(want, R.clean_mask(code, 1, 2, fg=(1, 4))[0])
    assert run.stdout.strip().splitlines() == ["mask of 77 x 50:"] + [
        "  %s by radius %d: %d set pixels before, %d after, %d added, %d removed" % ((nm, r) + tuple(st[k])) for k, (nm, r) in enumerate((("open", 1), ("close", 2)))]
    run = run_cli("clean_mask", [png, out, "--op", "erode", "--radius", "3"])
    assert run.returncode == 0, run.stderr
    assert np.array_equal(read_png_rgb(out), white(R.morphology(x, "erode", 3)[0]))
    run = run_cli("clean_mask", [png, out, "--open", "2", "--close", "0"])
    assert run.returncode == 0, run.stderr
    assert np.array_equal(read_png_rgb(out), white(R.morphology(x, "open", 2)[0]))
