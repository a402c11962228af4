"""The motion blur's definition (no GPU needed): properties of the numpy restatement tests/motionblur_ref.py, which the GPU equals
byte for byte (tests/test_gpu_motionblur.py), and the scenes of those GPU tests, with the assertion that they reach every branch of
the definition.  No tolerance appears anywhere."""
import numpy as np

import motionblur_ref as R

SIZES = ((1, 1), (5, 3), (33, 70), (70, 130))          # (h, w): 70 x 130 is 3 x 5 tiles, one of them with all nine neighbours
N = 3
_SCENES, _WANT = {}, {}
TILE_STEP = R.TILE

# vectors in pixels.  Unknown ones (every image gets them), then what only image 1 gets: exactly +-4096 (known, far past the cap), at
# the cap of max_blur 32 at shutter 0.5 (128 px -> 512), one step above it, a diagonal that the cap shortens by an inexact division
UNKNOWN = [(np.nan, 0), (0, np.nan), (np.inf, 1), (1, -np.inf), (5000, 0), (0, -5000), (-5000, 5000), (3e38, 0), (4096.5, 0)]
LONG = [(4096, 0), (0, -4096), (-4096, 4096), (128, 0), (128.25, 0), (96, 128), (-90.5, 91)]


def scene(h, w, n=N):
    """flow (n, h, w, 2), mask (n, h, w) and frames (u8 gray, u8 RGB, f32 gray, f32 RGB) of a case, computed once (nobody writes to
    them).  Vectors are multiples of 1/512 pixel, so that u s has fractions exactly at .5 (ties of rintf).
    Image 0: a still background (below the copy threshold) and a block moving by (12.25, -3.5) px: tiles on the copy path next to
    tiles that gather.  Image 1: random vectors of up to 8 px, the LONG vectors and a block moving by 200 px, which the cap shortens
    to a streak that crosses a whole tile (L = 32).  Image 2: (2.5, 0) px everywhere (L = 1, and every pixel ties for the tile
    maximum) with (0, 2.5) and (0, -2.5) px sprinkled in: ties between different vectors.  Every image: the UNKNOWN vectors."""
    key = (h, w, n)
    if key in _SCENES:
        return _SCENES[key]
    rng = np.random.default_rng(77 * h + w)
    flow = np.zeros((n, h, w, 2), np.float32)
    flow[0] = rng.integers(-200, 201, (h, w, 2)) / 512.0
    flow[0, h // 2:h // 2 + 12, 2:11] = (12.25, -3.5)
    if n > 1:
        flow[1] = rng.integers(-4096, 4097, (h, w, 2)) / 512.0
        flow[1, 2 * h // 3:2 * h // 3 + 5, w // 3:w // 3 + 7] = (200.0, 0.0)
    if n > 2:
        flow[2] = (2.5, 0.0)
        flow[2][rng.random((h, w)) < 0.02] = (0.0, 2.5)
        flow[2, ::TILE_STEP, ::TILE_STEP] = (0.0, -2.5)          # the first pixel of every tile
        flow[2, h - 1, w - 1] = (2.515625, 0.0)                  # 10.0625 -> 10 as its neighbours
    px = rng.permutation(h * w)
    for i in range(n):
        special = UNKNOWN + (LONG if i == 1 else [])
        for s, p in zip(special, np.roll(px, 5 * i)[:len(special)]):
            if h * w > 1 or i != 2:
                flow[i, p // w, p % w] = s
    mask = rng.choice(np.array([0, 0, 0, 0, 0, 0, 0, 0, 1, 2, 3, 200], np.uint8), (n, h, w))
    gray = rng.integers(0, 256, (n, h, w), dtype=np.uint8)
    rgb = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    fgray = ((rng.random((n, h, w)) - 0.25) * 300.0).astype(np.float32)
    frgb = ((rng.random((n, h, w, 3)) - 0.25) * 300.0).astype(np.float32)
    _SCENES[key] = (flow, mask, {"u8-1": gray, "u8-3": rgb, "f32-1": fgray, "f32-3": frgb})
    return _SCENES[key]


def want(h, w, kind, masked, s256=128, max_blur=32):
    key = (h, w, kind, masked, s256, max_blur)
    if key not in _WANT:
        flow, mask, frames = scene(h, w)
        _WANT[key] = R.blur(frames[kind], flow, mask if masked else None, s256, max_blur)
    return _WANT[key]


def texture(h, w, seed=0, top=100):
    return np.random.default_rng(seed).integers(0, top + 1, (1, h, w), dtype=np.uint8)


# ---- properties of the definition ------------------------------------------------------------------------------------------------
def test_identity_for_zero_and_sub_threshold_flow():
    h, w = 40, 70
    for kind in ("u8", "f32"):
        frame = texture(h, w, 1, 255) if kind == "u8" else np.random.default_rng(2).standard_normal((1, h, w, 3)).astype(np.float32)
        for u in (0.0, 1.75):                                        # 1.75 px at shutter 0.5: hx = 7, lenD = 7, one below the threshold
            flow = np.zeros((1, h, w, 2), np.float32)
            flow[..., 0] = u
            dst, code, vec, st = R.blur(frame, flow)
            assert dst.dtype == frame.dtype and np.array_equal(dst.view(np.uint8), frame.view(np.uint8)) and not code.any()
            assert (vec[..., 0] == int(4 * u)).all() and st[0, R.C0] == h * w and st[0, R.TAPS] == 0 and st[0, R.COPY_TILES] == 2 * 3
            assert st[0, R.MAX_LEN] == int(4 * u)
        flow[..., 0] = 2.0                                           # hx = 8: the gather path, L = 1, weights 16, 8 + 16 - 8 = 16
        dst, code, _, st = R.blur(frame, flow)
        assert (code[:, :, 1:-1] == 1).all() and st[0, R.COPY_TILES] == 0 and st[0, R.TAPS] == 3 * h * w


def test_uniform_whole_pixel_flow_is_the_rounded_box_mean():
    h, w = 9, 100
    frame = texture(h, w, 3, 255)
    for m, vx, vy in ((1, 4.0, 0.0), (3, -12.0, 0.0), (5, 20.0, 0.0), (32, 128.0, 0.0), (2, 0.0, 8.0)):
        flow = np.zeros((1, h, w, 2), np.float32)
        flow[..., 0], flow[..., 1] = vx, vy
        dst, code, _, st = R.blur(frame, flow)
        f = frame[0].astype(np.int64) if vy == 0 else frame[0].astype(np.int64).T
        d = dst[0] if vy == 0 else dst[0].T
        cd = code[0] if vy == 0 else code[0].T
        size = f.shape[1]
        box = sum(f[:, m + k:size - m + k] for k in range(-m, m + 1))
        assert np.array_equal(d[:, m:size - m], (2 * box + (2 * m + 1)) // (2 * (2 * m + 1))), (m, vx, vy)
        assert (cd[:, m:size - m] == 1).all() and (cd[:, :m] == 2).all() and (cd[:, size - m:] == 2).all()
        assert st[0, R.TAPS] == (2 * m + 1) * h * w and st[0, R.MAX_LEN] == 16 * m


def _moving_rectangle(h=96, w=192, y0=40, y1=60, x0=60, x1=80, u=8.0):
    frame = texture(h, w, 4)
    frame[0, y0:y1, x0:x1] = 255
    flow = np.zeros((1, h, w, 2), np.float32)
    flow[0, y0:y1, x0:x1, 0] = u
    return frame, flow


def test_a_moving_object_smears_one_way():
    """a white rectangle moving by 8 px (half-streak 2 px at shutter 0.5) over a still, darker texture"""
    y0, y1, x0, x1 = 40, 60, 60, 80
    frame, flow = _moving_rectangle()
    dst, code, vec, st = R.blur(frame, flow)
    changed = dst[0] != frame[0]
    assert (vec[0, y0:y1, x0:x1] == (32, 0)).all() and st[0, R.MAX_LEN] == 32
    # the background within the half-streak of the trailing and the leading edge takes colour from the rectangle
    assert changed[y0:y1, x0 - 2:x0].all() and changed[y0:y1, x1:x1 + 2].all()
    assert (dst[0, y0:y1, x0 - 2:x0] > frame[0, y0:y1, x0 - 2:x0]).all()
    # beyond the streak, and beside the rectangle across the motion, nothing changes
    assert not changed[:, :x0 - 2].any() and not changed[:, x1 + 2:].any()
    assert not changed[:y0].any() and not changed[y1:].any()
    assert (code[0][changed] == 1).all() and not code[0, :y0].any()
    # the rectangle's own edge takes background in: a streak, not a sharp edge
    assert changed[y0:y1, x0:x0 + 2].all() and not changed[y0:y1, x0 + 2:x1 - 2].any()
    # a plain average of the pixel's own vector would have left the background sharp; the copy path took the far tiles
    assert st[0, R.COPY_TILES] > 0


def test_a_fast_region_across_the_line_does_not_smear():
    h, w = 64, 96
    frame = texture(h, w, 5)
    flow = np.zeros((1, h, w, 2), np.float32)
    frame[0, 10:20, 10:20] = 255
    flow[0, 10:20, 10:20] = (16.0, 0.0)                             # sets D = (64, 0) for every tile around
    frame[0, 30:50, 50:60] = 200
    flow[0, 30:50, 50:60] = (0.0, 12.0)                             # fast, but across the line: r = 0
    dst, code, vec, _ = R.blur(frame, flow)
    _, D, lenD, L = R.tile_view(vec.astype(np.int64))
    assert (D[0, :2, :2] == (64, 0)).all() and (L[0, :2, :2] == 4).all()
    assert (vec[0, 30:50, 50:60] == (0, 48)).all()
    assert np.array_equal(dst[0, 24:, 40:], frame[0, 24:, 40:]) and not code[0, 24:, 40:].any()
    assert (dst[0, 10:20, 20:24] != frame[0, 10:20, 20:24]).all()     # while the region along the line does smear


def test_the_cap():
    for max_blur, at, above in ((7, (28.0, 0.0), (28.25, 0.0)), (32, (0.0, -128.0), (0.0, -128.25)), (5, (12.0, 16.0), (12.25, 16.0)),
                                (1, (4.0, 0.0), (4096.0, 4096.0))):
        flow = np.array([[at, above]], np.float32)[None]
        H, unknown = R.half_vectors(flow, None, 128, max_blur)
        cap16 = 16 * max_blur
        assert not unknown.any()
        assert (H[0, 0, 0] == np.rint(np.array(at) * 4)).all() and R.mag(H[0, 0, 0, 0], H[0, 0, 0, 1]) == cap16       # kept
        assert R.mag(H[0, 0, 1, 0], H[0, 0, 1, 1]) <= cap16 and (np.abs(H[0, 0, 1]) <= np.abs(np.rint(np.array(above) * 4))).all()
        assert R.mag(H[0, 0, 1, 0], H[0, 0, 1, 1]) >= cap16 - 2                                                   # shortened, not dropped
    H, _ = R.half_vectors(np.array([[[[96.0, 128.0]]]], np.float32), None, 128, 32)
    assert H[0, 0, 0].tolist() == [384 * 512 // 640, 512 * 512 // 640]                                            # towards zero
    H, _ = R.half_vectors(np.array([[[[-96.0, -128.0]]]], np.float32), None, 128, 32)
    assert H[0, 0, 0].tolist() == [-(384 * 512 // 640), -(512 * 512 // 640)]
    # ties of rintf go to even: 0.125 px and 0.375 px at shutter 0.5 are 0.5 and 1.5
    H, _ = R.half_vectors(np.array([[[[0.125, 0.375]]]], np.float32), None, 128, 32)
    assert H[0, 0, 0].tolist() == [0, 2]
    for s, s256 in ((1 / 256, 1), (0.5, 128), (2, 512)):
        assert R.shutter256(s) == s256


def test_every_branch_is_populated():
    """what the scenes of tests/test_gpu_motionblur.py reach, at the default shutter 0.5 and max_blur 32"""
    for h, w in SIZES[2:]:
        flow, mask, frames = scene(h, w)
        for masked in (False, True):
            dst, code, vec, st = want(h, w, "u8-1", masked)
            assert sorted(np.unique(code)) == [0, 1, 2, 3], (h, w, masked)
            assert (st[:, R.TAPS] > 0).all() and st[:, :4].sum() == N * h * w
            tm, D, lenD, L = R.tile_view(vec.astype(np.int64))
            assert (L == 1).any() and (L == 32).any() and (L == 0).any() and ((L > 1) & (L < 32)).any(), np.unique(L)
            assert st[0, R.COPY_TILES] > 0 and st[1, R.COPY_TILES] == 0 and st[1, R.MAX_LEN] == 512 and st[2, R.MAX_LEN] == 10
            assert (code == 2).sum() > 0                                 # clamped taps
        H, unknown = R.half_vectors(flow)
        # a tie in the tile maximum between different vectors, decided by the index: the first pixel of a tile of image 2
        sq = H[2, ..., 0] ** 2 + H[2, ..., 1] ** 2
        assert sq.max() == 100 and (H[2][sq == 100] == (10, 0)).all(1).any() and (H[2][sq == 100] == (0, 10)).all(1).any()
        assert (R.tile_max(H)[2] == (0, -10)).all()
        # ... and between tiles, decided by the raster order
        assert (R.neighbour_max(R.tile_max(H))[2] == (0, -10)).all()
        # unknown pixels of every kind; exactly 4096 is known
        u, v = flow[..., 0], flow[..., 1]
        for kind in (np.isnan(u) | np.isnan(v), np.isinf(u) | np.isinf(v), np.isfinite(u) & (np.abs(u) > 4096), np.isfinite(v) & (np.abs(v) > 4096)):
            assert kind.any() and unknown[kind].all()
        assert ((np.abs(u) == 4096) & ~unknown).any() and sorted(np.unique(mask)) == [0, 1, 2, 3, 200]
        assert (R.half_vectors(flow, mask)[1] & ~unknown).any()
        # vectors at and above the cap, and rintf ties
        x = np.nan_to_num(flow[1].astype(np.float64), posinf=0.0, neginf=0.0) * 4
        assert (np.abs(x - np.floor(x) - 0.5) == 0).any()
        raw = R.mag(*np.rint(np.nan_to_num(np.clip(flow[1], -4096, 4096)) * 4).astype(np.int64).transpose(2, 0, 1))
        assert (raw == 512).any() and (raw == 513).any() and (raw > 10000).any()
