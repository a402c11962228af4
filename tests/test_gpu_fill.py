"""The pull-push hole filling on the GPU: fotg_fill / fotg_fill_u8 equal the numpy restatement tests/fill_ref.py byte for byte in dst,
code and stats, for float32 frames of 1, 2 and 3 channels and 8-bit frames of 1 and 3, for both forms of the hole set, on frames
that cross the 64 x 64 tile by odd amounts and whose levels reach above the tile's (139 x 150, 200 x 300), that are odd at every
level (129 x 257), that are a tile or a tile and a row, and that are smaller than a block of any level; on hole patterns placed
against the tile's geometry and the frame's borders, from no hole to no known pixel; values that are holes without a map; single
and batched calls, each output alone and repeated calls give the same bytes; a dst at any alignment writes nothing outside; the
limits the header promises; fill_flow, fill_removed and the two OFClass compositions; the tool writes what the call returns."""
import ctypes as C

import numpy as np
import pytest
import torch

import fill_ref as R
from host_checks import gray_png_bytes, read_png_rgb, run_cli
from test_gpu_subtract import host
from test_gpu_warp import dev, make_ctx, np_same_bits, same_bits

pytestmark = pytest.mark.gpu

f32 = np.float32
T = 64                                                                # the kernels' tile
FRAMES = [(139, 150), (200, 300), (129, 257), (64, 64), (65, 64), (1, 1), (1, 17), (3, 5)]          # h, w
KINDS = [(f32, 1), (f32, 2), (f32, 3), (np.uint8, 1), (np.uint8, 3)]
FG = (2, 3)


def frame(shape, ch, dtype, seed):
    rng = np.random.default_rng(seed)
    shape = tuple(shape) + (ch,)
    if dtype == np.uint8:
        return rng.integers(0, 256, shape).astype(np.uint8)
    return ((rng.random(shape) - 0.3) * 700).astype(f32)             # more than 8 fractional bits: q rounds, the sums are signed


def patterns(h, w, seed=0):
    """bool (P, h, w), True = hole"""
    rng = np.random.default_rng(1000 * h + w + seed)
    Z = lambda: np.zeros((h, w), bool)
    pats = [Z(), ~Z()]                                                # none; all (the empty image)
    for y, x in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)):     # all but one pixel, in each corner in turn
        m = ~Z()
        m[y, x] = False
        pats.append(m)
    m = Z()                                                           # single holes at tile corners and frame borders ...
    for y in (0, T - 1, T, 2 * T - 1, 2 * T, h - 1):
        for x in (0, T - 1, T, 2 * T - 1, 2 * T, w - 1):
            if y < h and x < w:
                m[y, x] = True
    pats += [m, ~m]                                                   # ... and single known pixels there
    m = Z()
    m[min(T, h - 1):2 * T, min(T, w - 1):2 * T] = True                # a whole tile
    pats.append(m)
    m = Z()
    m[h // 8:h // 8 + T + T // 2 + 3, w // 9:w // 9 + 2 * T + 5] = True               # a rectangle larger than a tile
    pats.append(m)
    m = Z()
    m[:, :w // 2 + 22] = True                                         # a half-frame hole
    pats.append(m)
    m = ~Z()
    m[h // 3:h // 3 + max(1, h // 4), w // 3:w // 3 + max(1, w // 4)] = False         # holes touching every border
    pats.append(m)
    for sl in ((0, slice(None)), (h - 1, slice(None)), (slice(None), 0), (slice(None), w - 1)):
        m = Z()
        m[sl] = True
        pats.append(m)
    m = Z()
    m[::2] = True                                                     # 1-pixel stripes
    pats.append(m)
    m = Z()
    m[:, 1::2] = True
    pats.append(m)
    yy, xx = np.mgrid[:h, :w]
    pats.append((yy + xx) % 2 == 0)                                   # a checkerboard
    pats.append(rng.random((h, w)) < 0.5)
    pats.append(rng.random((h, w)) < 0.97)                            # the sparse-to-dense case
    return np.stack(pats)


def as_bytes(P, fg, seed=0):
    """the bool patterns as a byte map whose holes are those of P under fg"""
    rng = np.random.default_rng(seed)
    if fg is None:
        return np.where(P, rng.choice(np.array([1, 2, 8, 128, 255], np.uint8), P.shape), 0).astype(np.uint8)
    others = np.array([c for c in range(8) if c not in fg] + [8, 9, 130, 255], np.uint8)
    return np.where(P, rng.choice(np.array(fg, np.uint8), P.shape), rng.choice(others, P.shape)).astype(np.uint8)


def gpu_fill(src, hole, fg=None):
    from flowonthego_amd.fill import fill_holes
    out = fill_holes(dev(src), None if hole is None else dev(hole), fg=fg, dst=True, code=True, stats=True)
    torch.cuda.synchronize()
    return [host(o) for o in out]


def assert_same(got, want, what):
    for g, w_, nm in zip(got, want, ("dst", "code", "stats")):
        assert np_same_bits(g, w_), (what, nm, g.shape, w_.shape, np.argwhere(np.asarray(g != w_))[:5], g.reshape(-1)[:8], w_.reshape(-1)[:8])


@pytest.mark.parametrize("dtype,ch", KINDS)
@pytest.mark.parametrize("h,w", FRAMES)
def test_gpu_equals_the_restatement(h, w, dtype, ch):
    P = patterns(h, w)
    src = np.stack([frame((h, w), ch, dtype, 31 * k + ch) for k in range(len(P))])
    for fg in (None, FG):
        hole = as_bytes(P, fg, h + w)
        want = R.fill_holes(src, hole, fg)
        assert_same(gpu_fill(src, hole, fg), want, (h, w, dtype, ch, fg))
    st = want[2]
    assert st[0].tolist() == [h * w, 0, 0, 0] and st[1, :3].tolist() == [0, 0, h * w] and (st[:, :3].sum(1) == h * w).all()
    if (h, w) in ((139, 150), (200, 300)):
        assert st[10, 3] >= 7 - (h == 139) and st[2, 3] == 9 - (h == 139)            # the levels above the tile's are exercised
    if ch == 1:                                                       # the form without a channel dimension
        got = gpu_fill(src[..., 0], hole, FG)
        assert_same(got, (want[0][..., 0],) + tuple(want[1:]), "no channel dimension")


@pytest.mark.parametrize("ch", [1, 2, 3])
def test_values_that_are_holes_without_a_map(ch):
    h, w = 139, 150
    src = np.stack([frame((h, w), ch, f32, k) for k in range(4)])
    bad = (np.nan, np.inf, -np.inf, 1e9, 32768.5, -1e30)
    rng = np.random.default_rng(ch)
    for k in range(4):
        ys, xs = rng.integers(0, h, 40), rng.integers(0, w, 40)
        for i, (y, x) in enumerate(zip(ys, xs)):
            src[k, y, x, i % ch] = bad[i % len(bad)]                  # in one channel only
    src[0, 0, 0], src[0, h - 1, w - 1] = 32768.0, -32768.0            # the largest known values
    src[1, 60:130, 50:140, ch - 1] = 1e9                              # a .flo file's unknown region, across tiles
    src[3] = np.nan                                                   # nothing known, though with two channels the first is
    if ch > 1:
        src[3, :, :, 0] = 5.0
    want = R.fill_holes(src)
    got = gpu_fill(src, None)
    assert_same(got, want, "no map")
    assert want[2][3].tolist() == [0, 0, h * w, 9] and np.isfinite(got[0][:3]).all() and (want[1][:3].sum((1, 2)) >= 30).all()
    hole = as_bytes(patterns(h, w)[[8, 11, 18, 0]], None)
    assert_same(gpu_fill(src, hole), R.fill_holes(src, hole), "with a map")
    assert_same(gpu_fill(src[1], hole[1]), R.fill_holes(src[1], hole[1]), "single")
    assert_same(gpu_fill(src[1], None), R.fill_holes(src[1]), "single, no map")


def test_each_output_alone_single_calls_repeats_and_views():
    from flowonthego_amd.fill import fill_holes
    import flowonthego_amd as F
    h, w = 71, 131
    P = patterns(h, w)[[0, 1, 6, 9, 18, 19]]
    for dtype, ch in ((f32, 2), (np.uint8, 3)):
        src_np, hole_np = np.stack([frame((h, w), ch, dtype, k) for k in range(len(P))]), as_bytes(P, None, 2)
        src, hole = dev(src_np), dev(hole_np)
        full = fill_holes(src, hole, dst=True, code=True, stats=True)
        for _ in range(3):
            again = fill_holes(src, hole, dst=True, code=True, stats=True)
            assert all(same_bits(a, b) for a, b in zip(again, full))                   # the same bytes every time, stats included
        flags = ("dst", "code", "stats")
        for j, keep in enumerate(flags):
            one = fill_holes(src, hole, **{f: f == keep for f in flags})
            assert isinstance(one, torch.Tensor) and same_bits(one, full[j]), keep
        assert same_bits(F.fill_holes(src, hole), full[0])                             # the callable tool module
        for i in range(len(P)):
            one = fill_holes(src[i], hole[i], dst=True, code=True, stats=True)
            assert one[0].shape == (h, w, ch) and one[1].shape == (h, w) and one[2].shape == (4,)
            assert all(same_bits(a, b[i]) for a, b in zip(one, full)), i
        # the inputs are left as they were, and a view that is not contiguous is taken as its values
        assert same_bits(src, dev(src_np)) and same_bits(hole, dev(hole_np))
        v, hv = src[:, ::2, 1:], hole[:, ::2, 1:]
        assert same_bits(fill_holes(v, hv), fill_holes(v.contiguous(), hv.contiguous()))
        assert np_same_bits(host(fill_holes(v, hv)), R.fill_holes(host(v), host(hv))[0])
    for bad in (dict(dst=False), dict(fg=(8,)), dict(fg=())):
        with pytest.raises(F.FotgError):
            fill_holes(src, hole, **bad)
    for s, m in ((src, None), (src.double(), hole), (src[..., :2], hole), (src, hole[:, :-1]), (src.cpu(), hole), (dev(np.zeros((2, 4, 4, 4), f32)), None)):
        with pytest.raises(F.FotgError):
            fill_holes(s, m)


@pytest.mark.parametrize("dtype,ch", [(np.uint8, 1), (np.uint8, 3), (f32, 1), (f32, 3)])
def test_a_dst_at_any_alignment_writes_nothing_outside(dtype, ch):
    """dst at every offset 0 .. 8 (bytes; float32: elements) from an 8-byte boundary: the same bytes, and the guard bytes keep theirs"""
    from flowonthego_amd import lib
    from flowonthego_amd._args import _ptr, _stream
    tdt = torch.uint8 if dtype == np.uint8 else torch.float32
    fn = lib().fotg_fill_u8 if dtype == np.uint8 else lib().fotg_fill
    for h, w in ((67, 136), (21, 83)):                                 # rows of 136 pixels keep the offset; rows of 83 change it row by row
        n = 2
        src_np, hole_np = np.stack([frame((h, w), ch, dtype, k) for k in range(n)]), as_bytes(patterns(h, w)[[9, 18]], None)
        want = R.fill_holes(src_np, hole_np)
        src, hole = dev(src_np), dev(hole_np)
        size = n * h * w * ch
        for off in range(9):
            buf = torch.full((size + 64,), 77, dtype=tdt, device="cuda")
            cbuf = torch.full((n * h * w + 64,), 55, dtype=torch.uint8, device="cuda")
            stats = torch.full((n, 4), -1, dtype=torch.int64, device="cuda")
            o, c = buf[off:off + size], cbuf[off:off + n * h * w]
            assert fn(0, n, _ptr(src), w, h, ch, _ptr(hole), 0, _ptr(o), _ptr(c), _ptr(stats), _stream(torch.device("cuda", 0))) == 0
            torch.cuda.synchronize()
            assert np_same_bits(host(o).reshape(n, h, w, ch), want[0]) and np.array_equal(host(c).reshape(n, h, w), want[1]), (h, w, off)
            assert (buf[:off] == 77).all() and (buf[off + size:] == 77).all() and (cbuf[:off] == 55).all() and (cbuf[off + n * h * w:] == 55).all()
            assert np.array_equal(host(stats), want[2])


# ---- the limits the header promises --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(1, 16384), (16384, 1), (3, 16384), (16384, 3)])
def test_the_longest_frames_have_fourteen_levels(h, w):
    rng = np.random.default_rng(h)
    for dtype, ch in ((f32, 2), (np.uint8, 3)):
        src = frame((h, w), ch, dtype, 5)[None]
        hole = np.ones((3, h, w), bool)
        hole[0].reshape(-1)[rng.integers(0, h * w, 9)] = False        # nine known pixels in 16384: depth up to 14
        hole[1].reshape(-1)[0] = False                                # one known pixel, at the start
        hole[2] = rng.random((h, w)) < 0.5
        hb = hole.astype(np.uint8)
        srcs = np.repeat(src, 3, axis=0)
        want = R.fill_holes(srcs, hb)
        assert_same(gpu_fill(srcs, hb), want, (h, w, dtype))
        assert want[2][1, 3] == 14


def test_one_call_of_65535_images_between_guard_elements():
    from flowonthego_amd import lib
    from flowonthego_amd._args import _ptr, _stream
    n, h, w, ch, G = 65535, 2, 3, 3, 32
    base_src = np.stack([frame((h, w), ch, f32, k) for k in range(16)])
    base_hole = (np.random.default_rng(1).random((16, h, w)) < 0.5).astype(np.uint8)
    base_hole[0], base_hole[1] = 0, 1
    want = R.fill_holes(base_src, base_hole)
    idx = np.arange(n) % 16
    src, hole = dev(base_src[idx]), dev(base_hole[idx])
    buf = torch.full((n * h * w * ch + 2 * G,), -7.0, dtype=torch.float32, device="cuda")
    cbuf = torch.full((n * h * w + 2 * G,), 9, dtype=torch.uint8, device="cuda")
    sbuf = torch.full((n * 4 + 2 * G,), -3, dtype=torch.int64, device="cuda")
    o, c, s = buf[G:-G], cbuf[G:-G], sbuf[G:-G]
    assert lib().fotg_fill(0, n, _ptr(src), w, h, ch, _ptr(hole), 0, _ptr(o), _ptr(c), _ptr(s), _stream(torch.device("cuda", 0))) == 0
    torch.cuda.synchronize()
    assert np_same_bits(host(o).reshape(n, h, w, ch), want[0][idx]) and np.array_equal(host(c).reshape(n, h, w), want[1][idx])
    assert np.array_equal(host(s).reshape(n, 4), want[2][idx])
    for b, v in ((buf, -7.0), (cbuf, 9), (sbuf, -3)):
        assert (b[:G] == v).all() and (b[-G:] == v).all()


def test_element_offsets_beyond_two_to_the_31_equal_chunks_of_eight():
    """10930 frames of 256 x 256 x 3 float32: 2.15e9 elements, 8.6 GB each way; the levels of one call pass 1 GiB, so the call works
    through the batch in three chunks of its own"""
    from flowonthego_amd.fill import fill_holes, scratch_bytes
    n, h, w, ch = 10930, 256, 256, 3
    assert n * h * w * ch > 2 ** 31 and scratch_bytes(n, w, h, ch) <= 2 ** 30 < n * scratch_bytes(1, w, h, ch)
    g = torch.Generator(device="cuda").manual_seed(5)
    src = torch.empty((n, h, w, ch), dtype=torch.float32, device="cuda")
    hole = torch.empty((n, h, w), dtype=torch.uint8, device="cuda")
    for s in range(0, n, 1024):                                       # (in parts: the generators' temporaries stay small)
        src[s:s + 1024] = torch.rand(src[s:s + 1024].shape, generator=g, device="cuda") * 255
        hole[s:s + 1024] = torch.rand(hole[s:s + 1024].shape, generator=g, device="cuda") < 0.4
    hole[:, 40:200, 30:170] = 1
    hole[n - 1] = 1                                                   # the last image knows nothing
    hole[n - 2, :, :] = 1
    hole[n - 2, 255, 255] = 0
    dst, code, stats = fill_holes(src, hole, dst=True, code=True, stats=True)
    for s in range(0, n, 8):
        d8, c8, s8 = fill_holes(src[s:s + 8], hole[s:s + 8], dst=True, code=True, stats=True)
        assert same_bits(d8, dst[s:s + 8]) and same_bits(c8, code[s:s + 8]) and same_bits(s8, stats[s:s + 8]), s
    st = host(stats)
    assert st[n - 1].tolist() == [0, 0, h * w, 9] and st[n - 2].tolist() == [1, h * w - 1, 0, 8] and (st[:n - 2, 3] >= 5).all()
    one = R.fill_holes(host(src[n - 3]), host(hole[n - 3]))
    assert np_same_bits(host(dst[n - 3]), one[0]) and np.array_equal(st[n - 3], one[2])


# ---- the uses -------------------------------------------------------------------------------------------------------------------------
def test_fill_flow_on_a_consistency_mask():
    import flowonthego_amd as F
    rng = np.random.default_rng(3)
    n, h, w = 2, 75, 141
    fw = (rng.standard_normal((n, h, w, 2)) * 0.4 + (1.5, -0.5)).astype(f32)
    bw = (-fw + rng.standard_normal((n, h, w, 2)) * 0.05).astype(f32)
    bw[:, 20:50, 30:100] += 3.0                                       # an inconsistent region
    fw[0, 5, 5] = 1e9
    mask = F.fb_check(dev(fw), dev(bw))[0]
    got = F.fill_flow(dev(fw), mask)
    torch.cuda.synchronize()
    want = R.fill_holes(fw, host(mask))
    assert host(mask)[:, 20:50, 30:100].any() and np_same_bits(host(got), want[0]) and np.isfinite(host(got)).all()
    assert np_same_bits(host(F.fill_flow(dev(fw[0]), mask[0])), want[0][0])
    assert np_same_bits(host(F.fill_flow(dev(fw))), R.fill_holes(fw)[0])               # without a mask: the unknown vector alone
    with pytest.raises(F.FotgError):
        F.fill_flow(dev(fw[..., :1]))


def test_fill_removed_fills_exactly_the_holes_remove_objects_counts():
    import flowonthego_amd as F
    from flowonthego_amd.fill import fill_holes, removed_holes
    from test_gpu_erase import removal
    from test_gpu_subtract import case
    for noc, u8 in ((1, False), (3, True)):
        frames, plates, index, flows, motions, pcode, mask = case(noc, u8, 9, (33, 129), (131, 30, 1, -2))
        rm = removal((33, 129))
        rm[0, 3:30, 60:125] = 1                                       # a removal that leaves the plate
        clean, code, alpha, stats = F.remove_objects(dev(frames), dev(plates), dev(rm), motions=dev(motions), index=list(index), origin=(1, -2),
                                                     plate_code=dev(pcode), mask=dev(mask), grow=3, feather=4, dst=True, code=True, alpha=True,
                                                     stats=True)
        filled, fcode = F.fill_removed(clean, code, alpha, fill_code=True)
        torch.cuda.synchronize()
        holes = host(removed_holes(code, alpha))
        assert holes.sum() > 0 and np.array_equal(holes.sum((1, 2)), host(stats)[:, 5])
        if not u8:                                                    # a float frame's own NaN and 1e6 pixels are holes as well
            holes = holes | ~np.stack([R.known_map(c.reshape(c.shape[:2] + (-1,))) for c in host(clean)])
        assert np.array_equal(host(fcode) != 0, holes != 0)
        want = R.fill_holes(host(clean), host(removed_holes(code, alpha)))
        assert np_same_bits(host(filled), want[0]) and np.array_equal(host(fcode), want[1])
        assert same_bits(F.fill_removed(clean, code, alpha), filled)
        keep = host(fcode) == 0
        assert np_same_bits(host(filled)[keep], host(clean)[keep])


def test_ofclass_compositions_are_the_documented_ones(natural_images):
    import flowonthego_amd as F
    import motion_ref as M
    from flowonthego_amd.fill import fill_holes
    frames_np, _ = M.jittered_crops(natural_images["road_HD"], T=4, patch=True)
    frames = dev(frames_np)
    K, h, w = frames_np.shape
    o = make_ctx(2, w, h, max_batch=2, bidir=True)
    I0, I1 = frames[:-1], frames[1:]
    before = o.calc_filtered(I0, I1)
    fw_f, code, stats = o.calc_filled(I0, I1, code=True, stats=True)
    parts = []
    for s in range(0, K - 1, 2):
        fw, bw = o.bidirectional_flows(I0[s:s + 2], I1[s:s + 2])
        m, mb = o.upsample_crop_fb_check(fw, bw)
        parts.append((o.upsample_crop(fw), m, o.upsample_crop(bw), mb, fw))
    full, m = torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
    torch.cuda.synchronize()
    want = fill_holes(full, m, dst=True, code=True, stats=True)
    assert all(same_bits(a, b) for a, b in zip((fw_f, code, stats), want)) and m.any() and same_bits(code != 0, m != 0)
    assert np_same_bits(host(fw_f), R.fill_holes(host(full), host(m))[0])
    both = o.calc_filled(I0, I1, both=True)
    assert same_bits(both[0], fw_f) and same_bits(both[1], fill_holes(torch.cat([p[2] for p in parts]), torch.cat([p[3] for p in parts])))
    assert same_bits(o.upsample_crop_fill_flow(parts[0][4], parts[0][1]), fw_f[:2]) and same_bits(F.upsample_crop_fill_flow(o, parts[0][4]), full[:2])
    after = o.calc_filtered(I0, I1)
    assert same_bits(before, after)                                   # the existing method's result is what it was
    o.close()
    with pytest.raises(F.FotgError):
        make_ctx(2, w, h, max_batch=2).calc_filled(I0, I1)

    o = make_ctx(2, w, h, max_batch=K - 1)
    plain = o.remove_objects(frames, min_area=32)
    clean, code, mask, plate, fcode = o.remove_objects_filled(frames, min_area=32)
    holes = (((plain[1] == 2) | (plain[1] == 3)) & (F.grow_mask(plain[2], 2) != 0)).to(torch.uint8)
    _, rcode, alpha = F.remove_objects(frames, plain[3], plain[2], motions=F.frame_motions(F.plate_motions(
        F.upsample_crop_fit_motion(o, o.calc_sequence(frames), None, "affine", code=True)[0], 0)), plate_code=o.background(frames)[1], grow=2,
        feather=3, dst=True, code=True, alpha=True)
    torch.cuda.synchronize()
    assert same_bits(rcode, plain[1]) and same_bits(holes, F.fill.removed_holes(rcode, alpha))                 # alpha == 256 is the grown mask
    want = fill_holes(plain[0], holes, dst=True, code=True)
    assert same_bits(clean, want[0]) and same_bits(fcode, want[1]) and same_bits(clean, F.fill_removed(plain[0], rcode, alpha))
    assert same_bits(code, plain[1]) and same_bits(mask, plain[2]) and same_bits(plate, plain[3])
    again = o.remove_objects(frames, min_area=32)
    assert all(same_bits(a, b) for a, b in zip(plain, again))
    o.close()


# ---- the tool ----------------------------------------------------------------------------------------------------------------------
def test_cli_writes_what_the_call_returns(tmp_path):
    from flowonthego_amd.flo import read_flo, write_flo
    h, w = 50, 77
    p = lambda nm: str(tmp_path / nm)
    P = patterns(h, w)[9]
    x = frame((h, w), 1, np.uint8, 1)[..., 0]
    codes = as_bytes(P, FG, 3)
    np.save(p("x.npy"), x)
    np.save(p("codes.npy"), codes)
    open(p("x.png"), "wb").write(gray_png_bytes(x))
    open(p("m.png"), "wb").write(gray_png_bytes(P.astype(np.uint8) * np.uint8(200)))
    run = run_cli("fill_holes", [p("x.npy"), p("o.npy"), "--hole", p("codes.npy"), "--fg", "2,3", "--code", p("c.png")])
    assert run.returncode == 0, run.stderr
    want = R.fill_holes(x, codes, FG)
    assert np.array_equal(np.load(p("o.npy")), want[0])
    assert run.stdout.strip().splitlines() == ["image 0 of %d x %d: %d known, %d filled, %d unfilled, depth %d" % ((w, h) + tuple(want[2]))]
    assert np.array_equal(read_png_rgb(p("c.png")), np.array(((255, 255, 255), (220, 30, 30), (128, 128, 128)), np.uint8)[want[1]])
    run = run_cli("fill_holes", [p("x.png"), p("o.png"), "--hole", p("m.png")])
    assert run.returncode == 0, run.stderr
    assert np.array_equal(read_png_rgb(p("o.png")), np.repeat(want[0][..., None], 3, axis=2))
    flow = frame((h, w), 2, f32, 2)
    flow[P] = 1e9
    write_flo(p("f.flo"), flow)
    run = run_cli("fill_holes", [p("f.flo"), p("g.flo")])
    assert run.returncode == 0, run.stderr
    assert np_same_bits(read_flo(p("g.flo")), R.fill_holes(flow)[0])
