"""The binary morphology restated in numpy, straight from the definition in include/fotg.h (fotg_morph): a loop over the offsets of
the disc, one shifted copy of the map per offset.  No scipy, nothing clever: this is what the GPU has to equal byte for byte."""
import numpy as np

STAGES = {"erode": ("erode",), "dilate": ("dilate",), "open": ("erode", "dilate"), "close": ("dilate", "erode")}


def fg_map(x, fg=None):
    """(..., h, w) uint8 -> bool: the set pixels.  fg None: every non-zero byte; otherwise the byte values (each 0 .. 7) that are set"""
    x = np.asarray(x)
    if fg is None:
        return x != 0
    out = np.zeros(x.shape, bool)
    for c in fg:
        assert 0 <= int(c) <= 7
        out |= x == int(c)
    return out


def disc(r):
    """the offsets (dx, dy) with dx^2 + dy^2 <= r^2"""
    return [(dx, dy) for dy in range(-r, r + 1) for dx in range(-r, r + 1) if dx * dx + dy * dy <= r * r]


def dilate(X, r):
    """(..., h, w) bool: set iff some pixel of the frame within the disc is set"""
    X = np.asarray(X, bool)
    h, w = X.shape[-2:]
    out = np.zeros_like(X)
    for dx, dy in disc(r):
        # out[y, x] |= X[y + dy, x + dx] where (x + dx, y + dy) lies in the frame
        y0, y1, x0, x1 = max(0, -dy), min(h, h - dy), max(0, -dx), min(w, w - dx)
        if y0 < y1 and x0 < x1:
            out[..., y0:y1, x0:x1] |= X[..., y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return out


def erode(X, r):
    """(..., h, w) bool: set iff every pixel of the frame within the disc is set; pixels outside the frame take no part"""
    X = np.asarray(X, bool)
    h, w = X.shape[-2:]
    out = np.ones_like(X)
    for dx, dy in disc(r):
        y0, y1, x0, x1 = max(0, -dy), min(h, h - dy), max(0, -dx), min(w, w - dx)
        if y0 < y1 and x0 < x1:
            out[..., y0:y1, x0:x1] &= X[..., y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return out


def chain(x, stages, fg=None):
    """x (n, h, w) or (h, w) uint8; stages: pairs ("erode" | "dilate", r) -> (out uint8 0 / 1 of x's shape, stats int64 (n, 4) or
    (4,): set before, set after, added, removed)"""
    X = fg_map(x, fg)
    Y = X
    for op, r in stages:
        assert 0 <= r <= 8
        Y = erode(Y, r) if op == "erode" else dilate(Y, r)
    stats = np.stack((X.sum((-2, -1)), Y.sum((-2, -1)), (Y & ~X).sum((-2, -1)), (X & ~Y).sum((-2, -1))), axis=-1).astype(np.int64)
    return Y.astype(np.uint8), stats


def morphology(x, op, r, fg=None):
    return chain(x, [(s, r) for s in STAGES[op]], fg)


def clean_mask(x, open=1, close=2, fg=None):
    """the opening, then the closing: (out, stats (n, 2, 4) or (2, 4))"""
    a, sa = morphology(x, "open", open, fg)
    b, sb = morphology(a, "close", close)
    return b, np.stack((sa, sb), axis=-2)


def foreground_objects(code, evidence, connectivity=8, min_area=64, max_objects=256, open=0, close=0):
    """flowonthego_amd.subtract.foreground_objects restated over objects_ref: (objects, ids, confirmed).  With open = close = 0 the
    components of the codes (1, 4) as they are; otherwise those of the cleaned map, with the same evidence"""
    import objects_ref as OR
    if open or close:
        cleaned, _ = clean_mask(code, open, close, fg=(1, 4))
        res = OR.components_batch(cleaned, OR.fg_set((1,)), connectivity, evidence, min_area=min_area, max_objects=max_objects)
    else:
        res = OR.components_batch(code, OR.fg_set((1, 4)), connectivity, evidence, min_area=min_area, max_objects=max_objects)
    return res["objects"], res["ids"], res["objects"][..., 9] > 0
