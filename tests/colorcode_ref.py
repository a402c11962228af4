"""numpy restatement of the reference's Middlebury colour code (flow_code/C/colorcode.cpp computeColor, color_flow.cpp MotionToColor):
the project's contract for fotg_flow_color.  Every operation in the reference's precision -- f32 sqrt, lerps and division, double
where the reference's expression is double -- except the angle, which is the correctly rounded f32 of atan2 instead of glibc's
atan2f.  Test helper only; the product has no CPU path."""
import os

import numpy as np

f32, f64 = np.float32, np.float64
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "colorcode_ref.npz")


def _wheel():
    segs = [(15, lambda i: (255, 255 * i // 15, 0)), (6, lambda i: (255 - 255 * i // 6, 255, 0)), (4, lambda i: (0, 255, 255 * i // 4)),
            (11, lambda i: (0, 255 - 255 * i // 11, 255)), (13, lambda i: (255 * i // 13, 0, 255)), (6, lambda i: (255, 0, 255 - 255 * i // 6))]
    return np.array([f(i) for n, f in segs for i in range(n)], dtype=np.int64)


WHEEL = _wheel()                                       # 55 x 3, R G B
WHEEL_F = (WHEEL / 255.0).astype(f32)                  # colorwheel[k][b] / 255.0, stored to float


def unknown(u, v):
    return (np.abs(u) > f32(1e9)) | (np.abs(v) > f32(1e9)) | np.isnan(u) | np.isnan(v)


def compute_color(fx, fy):
    """computeColor over arrays of float32 -> (..., 3) uint8, R, G, B"""
    fx, fy = np.asarray(fx, f32), np.asarray(fy, f32)
    with np.errstate(all="ignore"):
        rad = np.sqrt(fx * fx + fy * fy)
        ang = np.arctan2((-fy).astype(f64), (-fx).astype(f64)).astype(f32)
        a = (ang.astype(f64) / np.pi).astype(f32)
        fk = ((a.astype(f64) + 1.0) / 2.0 * 54).astype(f32)
        k0 = fk.astype(np.int64)
        k1 = (k0 + 1) % 55
        f = (fk - k0.astype(f32)).astype(f32)
        out = np.empty(fx.shape + (3,), np.uint8)
        for b in range(3):
            col0, col1 = WHEEL_F[k0, b], WHEEL_F[k1, b]
            col = (f32(1) - f) * col0 + f * col1
            col = np.where(rad <= f32(1), f32(1) - rad * (f32(1) - col), (col.astype(f64) * .75).astype(f32)).astype(f32)
            out[..., b] = (255.0 * col.astype(f64)).astype(np.int64)
    return out


def stats(flow):
    """the five values MotionToColor prints: maxrad, minu, maxu, minv, maxv over the known vectors, with its initial values"""
    u, v = flow[..., 0].astype(f32), flow[..., 1].astype(f32)
    k = ~unknown(u, v)
    if not k.any():
        return np.array([-1, 999, -999, 999, -999], f32)
    u, v = u[k], v[k]
    rad = np.sqrt(u * u + v * v)
    return np.array([rad.max(), min(u.min(), f32(999)), max(u.max(), f32(-999)), min(v.min(), f32(999)), max(v.max(), f32(-999))], f32)


def motion_to_color(flow, maxmotion=-1.0):
    """MotionToColor of one (h, w, 2) float32 field -> ((h, w, 3) uint8 R, G, B, stats)"""
    flow = np.asarray(flow, f32)
    st = stats(flow)
    maxrad = st[0]
    if f32(maxmotion) > 0:
        maxrad = f32(maxmotion)
    if maxrad == 0:
        maxrad = f32(1)
    u, v = flow[..., 0], flow[..., 1]
    k = ~unknown(u, v)
    rgb = np.zeros(flow.shape[:2] + (3,), np.uint8)
    with np.errstate(all="ignore"):
        rgb[k] = compute_color(u[k] / maxrad, v[k] / maxrad)
    return rgb, st


def grid_vectors():
    """the fixture's 160 000 "random" vectors, made with integer arithmetic only (so every machine makes the same bits and the
    fixture stores only the reference's outputs): a 400 x 400 grid of integers jittered by a hash in the low 7 bits, each row
    band of 25 rows scaled by its own power of two (2^-22 .. 2^-7): |v| from about 2e-3 to 280, every angle, in and beyond the
    unit disc.  Neighbouring vectors have neighbouring colours, which keeps the stored outputs small."""
    u64 = np.uint64
    jj, ii = np.meshgrid(np.arange(400, dtype=u64), np.arange(400, dtype=u64), indexing="ij")
    m = u64(0xffffffff)
    h = (ii * u64(0x9E3779B1) + jj * u64(0x85EBCA77) + u64(12345)) & m
    h = ((h ^ (h >> u64(15))) * u64(0x2C1B3C6D)) & m
    h = h ^ (h >> u64(13))
    i, j = ii.astype(np.int64) - 200, jj.astype(np.int64) - 200
    x = (i * 128 + (h & u64(127)).astype(np.int64) - 64).astype(f32)          # |integer| < 2^15: exact in f32
    y = (j * 128 + ((h >> u64(7)) & u64(127)).astype(np.int64) - 64).astype(f32)
    scale = np.ldexp(f32(1), (jj.astype(np.int64) // 25 - 22).astype(np.int32)).astype(f32)   # exact powers of two
    return np.stack([x * scale, y * scale], -1).reshape(-1, 2)


def load_fixture():
    """tests/golden/colorcode_ref.npz (tests/golden/make_colorcode_golden.py) ->
    (vectors (k, 2) f32, the reference's computeColor of them (k, 3) u8 R G B, kind (k,): 0 grid, 1 named edge case, 2 wheel
    boundary), [(run name, flow (h, w, 2), maxmotion, row step, reference RGB of rows ::step, reference printed stats)]"""
    z = np.load(FIXTURE)
    named = z["cc_named_in"]
    vin = np.concatenate([named, grid_vectors()])
    vout = np.concatenate([z["cc_named_out"], z["cc_grid_out"]])
    kind = np.concatenate([z["cc_named_kind"], np.zeros(len(vin) - len(named), np.uint8)])
    alley = np.load(os.path.join(os.path.dirname(FIXTURE), "alley_0001_flo.npz"))["flow"]
    runs = []
    for name in [str(n) for n in z["mtc_runs"]]:
        field = str(z["mtc/%s/field" % name])
        flow = alley if field == "alley" else z["field/%s" % field]
        runs.append((name, flow, float(z["mtc/%s/maxmotion" % name]), int(z["mtc/%s/rows" % name]), z["mtc/%s/rgb" % name],
                     z["mtc/%s/stats" % name]))
    return vin, vout, kind, runs
