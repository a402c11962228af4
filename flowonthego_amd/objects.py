"""Objects on the GPU: the connected components of a uint8 code map (the codes of fit_motion, fb_check, warp or interpolate) with a
record each -- box, area, coordinate sums and the sums of a per-pixel motion -- over fotg_label_components of libfotg.so, and the
moving objects of a flow on top of it: the pixels that do not follow the camera motion (fit_motion's code 1), grouped, each with its
mean motion relative to the camera.  Exact integers throughout (no floating-point atomics: the same bytes every run); the
definition, in order, is in include/fotg.h and csrc/components.hip.h.  It runs in HIP only; there is no CPU fallback."""
import ctypes as C

import torch

from ._args import _dev_f32, _ptr, _stream, optional, two_channel, unbatch
from ._lib import FotgError, check, lib

OBJECT = ("label", "area", "xmin", "ymin", "xmax", "ymax", "sum_x", "sum_y", "n_val", "sum_u", "sum_v")
OBJECT_STATS = ("foreground", "components", "kept", "written")
MAX_DIM = 16384
MAX_OBJECTS = 65536


def _tile():
    tw, th = C.c_int(0), C.c_int(0)
    check(lib().fotg_components_tile(C.byref(tw), C.byref(th)))
    return tw.value, th.value


def __getattr__(name):
    if name == "TILE":                  # (width, height) of the labelling kernels' tile, from the library
        return _tile()
    raise AttributeError(name)


def _fg_set(fg):
    if isinstance(fg, int) and not isinstance(fg, bool):
        fg = (fg,)
    try:
        codes = [int(c) for c in fg]
    except (TypeError, ValueError):
        raise FotgError("fg must be a code 0 .. 7 or a sequence of them")
    if not codes or any(c < 0 or c > 7 for c in codes):
        raise FotgError("fg must name at least one code, each in 0 .. 7")
    s = 0
    for c in codes:
        s |= 1 << c
    return s


def label_components(code, fg=(1,), connectivity=8, values=None, min_area=1, max_objects=256, labels=False, ids=False, stats=False):
    """code: device tensor (n, h, w) or (h, w) uint8; fg: the codes that are foreground (each 0 .. 7); connectivity 4 or 8; values:
    None or float32 (n, h, w, 2) / (h, w, 2), a vector per pixel (fit_motion's residual).
    Returns objects, int64 (n, max_objects, 11) or (max_objects, 11): one row (OBJECT) per component of at least min_area pixels,
    in ascending order of the label (the linear index y*w + x of the component's first pixel in raster order), at most the first
    max_objects of them, the other rows zero.  sum_u, sum_v are the sums of (int)rint(256 u), (int)rint(256 v) over the n_val pixels
    of the component whose vector is finite and within +-4096 px.  With any of labels / ids / stats a tuple of objects and those
    asked for, in this order: labels int32 (n, h, w) (the label, -1 for background), ids int32 (n, h, w) (the row in objects, -1 for
    background, a component too small or one beyond max_objects), stats int64 (n, 4) (OBJECT_STATS: foreground pixels, components,
    components of at least min_area, rows written).  Components never join across the images of a batch.  Asynchronous on the
    current stream of the code's device."""
    if not isinstance(code, torch.Tensor) or code.dim() not in (2, 3):
        raise FotgError("code must be a (n, h, w) or (h, w) tensor")
    single = code.dim() == 2
    if single:
        code = code.unsqueeze(0)
    n, h, w = (int(v) for v in code.shape)
    if n < 1 or h < 1 or w < 1 or h > MAX_DIM or w > MAX_DIM:
        raise FotgError("code must have between 1 and %d rows and columns: %s" % (MAX_DIM, tuple(code.shape)))
    _dev_f32(code, "code", dtype=torch.uint8)
    values = optional(values, "values", code.device, (n, h, w, 2), single=single)
    if connectivity not in (4, 8):
        raise FotgError("connectivity must be 4 or 8")
    if not isinstance(min_area, int) or isinstance(min_area, bool) or min_area < 1:
        raise FotgError("min_area must be an integer >= 1")
    if not isinstance(max_objects, int) or isinstance(max_objects, bool) or max_objects < 1 or max_objects > MAX_OBJECTS:
        raise FotgError("max_objects must be an integer in 1 .. %d" % MAX_OBJECTS)
    dev = code.device
    outs = (torch.empty((n, max_objects, len(OBJECT)), dtype=torch.int64, device=dev),
            torch.empty((n, h, w), dtype=torch.int32, device=dev) if labels else None,
            torch.empty((n, h, w), dtype=torch.int32, device=dev) if ids else None,
            torch.empty((n, len(OBJECT_STATS)), dtype=torch.int64, device=dev) if stats else None)
    check(lib().fotg_label_components(dev.index or 0, n, _ptr(code), w, h, _fg_set(fg), connectivity, _ptr(values), min_area, max_objects,
                                      _ptr(outs[1]), _ptr(outs[2]), _ptr(outs[0]), _ptr(outs[3]), _stream(dev)))
    return unbatch(outs, single)


def moving_objects(flow, mask=None, model="affine", iters=3, thresh=1.0, min_area=64, max_objects=256, connectivity=8, ids=False,
                   stats=False):
    """flow: device tensor (n, h, w, 2) or (h, w, 2) float32; mask as in fit_motion.  The camera motion is fitted (fit_motion: model,
    iters, thresh), and the pixels that do not follow it (code 1) are grouped into objects with the fit's residual as values: sum_u /
    (256 n_val), sum_v / (256 n_val) of a row is the object's mean motion relative to the camera (object_summary).
    Returns (params, objects[, ids][, stats]) -- params as fit_motion returns them, the rest as label_components."""
    from .motion import fit_motion
    params, code, residual = fit_motion(flow, mask, model, iters, thresh, code=True, residual=True)
    out = label_components(code, (1,), connectivity, residual, min_area, max_objects, ids=ids, stats=stats)
    return (params,) + (out if isinstance(out, tuple) else (out,))


def object_summary(objects):
    """objects (..., 11) int64 -> (..., 4) float64: the centroid (sum_x / area, sum_y / area) and the mean motion (sum_u / (256 n_val),
    sum_v / (256 n_val)) in pixels.  Division by zero yields NaN: every entry of an unwritten (all-zero) row, and the mean motion
    of an object without an admissible vector (or labelled without values)."""
    if not isinstance(objects, torch.Tensor) or objects.dim() < 1 or objects.shape[-1] != len(OBJECT):
        raise FotgError("objects must be a (..., 11) tensor")
    o = objects.to(torch.float64)
    return torch.stack((o[..., 6] / o[..., 1], o[..., 7] / o[..., 1], o[..., 9] / (256.0 * o[..., 8]), o[..., 10] / (256.0 * o[..., 8])), -1)


def ofc_moving_objects(ofc, frames, model="affine", iters=3, thresh=1.0, min_area=64, max_objects=256, connectivity=8, ids=False,
                       stats=False):
    """OFClass.moving_objects: the flows of frames (T+1, ...) first (on a bidir context the forward consistency mask is the fit's
    mask), the motion fit of each with code and residual, then label_components: (params (T, 6), objects (T, max_objects, 11)[,
    ids][, stats])"""
    from .motion import _sequence_flows, upsample_crop_fit_motion
    two_channel(ofc, "the motion fit needs a two-channel flow")
    fw, mask = _sequence_flows(ofc, frames)
    params, code, residual = upsample_crop_fit_motion(ofc, fw, mask, model, iters, thresh, code=True, residual=True)
    out = label_components(code, (1,), connectivity, residual, min_area, max_objects, ids=ids, stats=stats)
    return (params,) + (out if isinstance(out, tuple) else (out,))
