"""The connected-component labelling of flowonthego_amd.objects (fotg_label_components, csrc/components.hip.h) restated in plain
numpy / Python, written for clarity.  The definition, in order:

Input: code (h, w) uint8; fg_codes, an 8-bit set: pixel p is foreground iff code[p] < 8 and (fg_codes >> code[p]) & 1;
  connectivity 4 or 8; values None or (h, w, 2) float32.  A batch is labelled image by image: nothing joins across images.
Label: the linear index y*w + x of the component's first pixel in raster order (= the minimum over its pixels).
Record (OBJECT), eleven int64: label, area, xmin, ymin, xmax, ymax, sum x, sum y, n_val, sum U, sum V, where U = (int)rintf(256 u),
  V = (int)rintf(256 v) and a vector takes part iff |u| <= 4096 and |v| <= 4096 (false for a NaN or an infinity); n_val counts those
  pixels.  All three are 0 without values.
Selection: kept iff area >= min_area; the kept components in ascending label order are the rows of objects (max_objects, 11); at
  most the first max_objects are written, the other rows are zero.
labels int32 (h, w): the label or -1 (background); ids int32 (h, w): the row in objects, or -1 (background, too small, beyond
  max_objects); stats int64 (4,) (OBJECT_STATS): foreground pixels, components, kept components, rows written."""
import numpy as np

OBJECT = ("label", "area", "xmin", "ymin", "xmax", "ymax", "sum_x", "sum_y", "n_val", "sum_u", "sum_v")
OBJECT_STATS = ("foreground", "components", "kept", "written")


def fg_set(fg):
    """codes (1,), (0, 3) ... -> the 8-bit set"""
    s = 0
    for c in fg:
        s |= 1 << int(c)
    return s


def foreground(code, fg_codes):
    c = code.astype(np.int64)
    return (c < 8) & (((fg_codes >> np.minimum(c, 7)) & 1) == 1)


def label(fg, connectivity):
    """(h, w) bool -> (h, w) int32: union-find in raster order, the smaller root wins"""
    h, w = fg.shape
    parent = list(range(h * w))

    def find(a):
        r = a
        while parent[r] != r:
            r = parent[r]
        while parent[a] != r:
            parent[a], a = r, parent[a]
        return r

    def union(a, b):
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)

    before = [(0, -1), (-1, 0)] if connectivity == 4 else [(0, -1), (-1, -1), (-1, 0), (-1, 1)]
    f = fg.tolist()
    for y in range(h):
        for x in range(w):
            if not f[y][x]:
                continue
            for dy, dx in before:
                yy, xx = y + dy, x + dx
                if 0 <= yy and 0 <= xx < w and f[yy][xx]:
                    union(y * w + x, yy * w + xx)
    out = np.full(h * w, -1, np.int32)
    for p in np.flatnonzero(fg.ravel()):
        out[p] = find(int(p))
    return out.reshape(h, w)


def fixed_point(values):
    """(h, w, 2) float32 -> admissible (h, w) bool, U, V (h, w) int64 (0 where not admissible)"""
    u, v = values[..., 0].astype(np.float32), values[..., 1].astype(np.float32)
    with np.errstate(invalid="ignore"):
        ok = (np.abs(u) <= np.float32(4096)) & (np.abs(v) <= np.float32(4096))
    U = np.where(ok, np.rint(np.where(ok, u, 0) * np.float32(256)), 0).astype(np.int64)
    V = np.where(ok, np.rint(np.where(ok, v, 0) * np.float32(256)), 0).astype(np.int64)
    return ok, U, V


def components(code, fg_codes=2, connectivity=8, values=None, min_area=1, max_objects=256):
    """one image -> dict(labels, ids, objects, stats)"""
    code = np.asarray(code)
    h, w = code.shape
    fg = foreground(code, fg_codes)
    labels = label(fg, connectivity)
    if values is not None:
        ok, U, V = fixed_point(np.asarray(values))
    objects = np.zeros((max_objects, 11), np.int64)
    ids = np.full((h, w), -1, np.int32)
    area = np.bincount(labels[labels >= 0], minlength=h * w)    # per label: the labels that occur are the roots
    roots = np.flatnonzero(area)                                # ascending
    kept = [r for r in roots if area[r] >= min_area]
    for row, r in enumerate(kept[:max_objects]):
        ys, xs = np.nonzero(labels == r)
        rec = [r, len(ys), xs.min(), ys.min(), xs.max(), ys.max(), xs.sum(), ys.sum(), 0, 0, 0]
        if values is not None:
            m = ok[ys, xs]
            rec[8:] = [m.sum(), U[ys, xs][m].sum(), V[ys, xs][m].sum()]
        objects[row] = rec
        ids[ys, xs] = row
    stats = np.array([fg.sum(), len(roots), len(kept), min(len(kept), max_objects)], np.int64)
    return dict(labels=labels, ids=ids, objects=objects, stats=stats)


def components_batch(code, fg_codes=2, connectivity=8, values=None, min_area=1, max_objects=256):
    """(n, h, w) -> the same dict, stacked"""
    res = [components(code[i], fg_codes, connectivity, None if values is None else values[i], min_area, max_objects) for i in range(len(code))]
    return {k: np.stack([r[k] for r in res]) for k in res[0]}


def summary(objects):
    """objects (..., 11) -> (..., 4) float64: centroid x, y = sum x / area, sum y / area; mean motion = sum U / (256 n_val), sum V /
    (256 n_val); 0 / 0 is NaN"""
    o = np.asarray(objects).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.stack([o[..., 6] / o[..., 1], o[..., 7] / o[..., 1], o[..., 9] / (256.0 * o[..., 8]), o[..., 10] / (256.0 * o[..., 8])], -1)
