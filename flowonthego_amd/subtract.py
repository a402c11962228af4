"""Background subtraction against a plate on the GPU, with two thresholds for hysteresis: every frame is compared with the plate
(flowonthego_amd.plate) sampled into the frame's own grid along the frame's motion, the difference is averaged over a small window
and classified -- over fotg_subtract / fotg_subtract_motion / fotg_upsample_crop_subtract of libfotg.so.  The definition, in f32
and in order, is in include/fotg.h and csrc/subtract.hip.h.  One kernel samples the plate, stages the differences of a tile and its
halo on chip and writes every output once; it runs in HIP only, there is no CPU fallback.  What it finds and moving_objects does
not: an object that stops, one that moves slowly, the untextured inside of a large one.

The module is callable: flowonthego_amd.subtract(frames, plate, ...) is flowonthego_amd.subtract.subtract_background(frames, plate, ...)."""
import ctypes as C
import math
import struct

import torch

from ._args import _dev_f32, _ptr, _stream, coarse_shape, image_stack, optional, two_channel, unbatch
from ._lib import FotgError, callable_module, check, lib
from .temporal import _ints

CODES = ("background", "foreground", "no_plate", "unknown", "strong")
STATS = CODES + ("sum_diff", "sum_diff_foreground")
FG = (1, 4)                        # the foreground set label_components takes
MAX_DIM = 16384
MAX_ORIGIN = 1 << 20
MAX_Q = 32767                      # the largest difference and threshold, in 1/16 grey levels


def _q16(v, name):
    """lrintf(16 v) of the f32 nearest to v"""
    try:
        f = struct.unpack("f", struct.pack("f", float(v)))[0]
    except (TypeError, ValueError, OverflowError, struct.error):
        raise FotgError("%s must be a number" % name)
    if not math.isfinite(f) or abs(f) > 1e6:
        raise FotgError("%s must be finite and 0 <= 16 low <= 16 high <= %d" % (name, MAX_Q))
    return int(round(16.0 * f))    # (16 f is exact; round() rounds halves to even, as lrintf does)


def _plain(low, high, window, origin, wanted):
    """what is decided from the plain arguments alone: (ox, oy)"""
    L, Hh = _q16(low, "low"), _q16(high, "high")
    if not 0 <= L <= Hh <= MAX_Q:
        raise FotgError("the thresholds must satisfy 0 <= lrintf(16 low) <= lrintf(16 high) <= %d: %d, %d" % (MAX_Q, L, Hh))
    if isinstance(window, bool) or window not in (0, 1, 2):
        raise FotgError("window must be 0, 1 or 2 (1 x 1, 3 x 3, 5 x 5)")
    try:
        ox, oy = (int(v) for v in origin)
    except (TypeError, ValueError):
        raise FotgError("origin must be (ox, oy)")
    if abs(ox) > MAX_ORIGIN or abs(oy) > MAX_ORIGIN:
        raise FotgError("origin must lie within +-%d" % MAX_ORIGIN)
    if not any(wanted):
        raise FotgError("ask for at least one of code, diff, evidence and stats")
    return ox, oy


def _plates(plate, frames, index, n):
    """the plate stack (P, H, W[, c]) of the frames' type and channels and the plate of every frame: (plate, P, H, W, ctypes index)"""
    if isinstance(plate, torch.Tensor) and plate.dim() == frames.dim() - 1:
        plate = plate.unsqueeze(0)
    if not isinstance(plate, torch.Tensor) or plate.dim() != frames.dim() or plate.dtype != frames.dtype \
            or tuple(plate.shape[3:]) != tuple(frames.shape[3:]):
        raise FotgError("plate must be (H, W[, c]) or (P, H, W[, c]) of the frames' type and channels")
    plate, _ = image_stack(plate, "plate", None, None, None, frames.device, (frames.dtype,))
    P, H, W = (int(v) for v in plate.shape[:3])
    if H > MAX_DIM or W > MAX_DIM or P > 65535:
        raise FotgError("a plate must have between 1 and %d rows and columns" % MAX_DIM)
    if index is None:
        if P not in (1, n):
            raise FotgError("%d plates for %d frames: say which with index" % (P, n))
        return plate, P, H, W, None
    index = _ints(index, "index")
    try:
        ix = [int(v) for v in index]
    except (TypeError, ValueError):
        raise FotgError("index must hold one plate index per frame")
    if len(ix) != n or any(v < 0 or v >= P for v in ix):
        raise FotgError("index must hold %d plate indices in 0 .. %d" % (n, P - 1))
    return plate, P, H, W, (C.c_int * n)(*ix)


def _outputs(n, h, w, dev, wanted):
    code, diff, evidence, stats = wanted
    return (torch.empty((n, h, w), dtype=torch.uint8, device=dev) if code else None,
            torch.empty((n, h, w), dtype=torch.int16, device=dev) if diff else None,
            torch.empty((n, h, w, 2), dtype=torch.float32, device=dev) if evidence else None,
            torch.empty((n, len(STATS)), dtype=torch.int64, device=dev) if stats else None)


def subtract_background(frames, plate, flows=None, motions=None, index=None, origin=(0, 0), plate_code=None, mask=None, low=8.0,
                        high=24.0, window=1, code=True, diff=False, evidence=False, stats=False):
    """frames: device tensor (n, h, w) or (n, h, w, c), c in (1, 3), float32 or uint8 -- or, with a single vector source, one frame
    (h, w) / (h, w, c).  plate: (H, W[, c]) or (P, H, W[, c]) of the frames' type (background_plate's dst); index: None (one plate
    for all frames, or plate i for frame i when P == n) or n plate indices (a host list).  origin: (ox, oy), canvas pixel (X, Y) of
    the plate is the reference coordinate (X - ox, Y - oy).  Exactly one source of the vectors frame -> reference: flows
    (n, h, w, 2) / (h, w, 2) float32, or motions (n, 6) / (6,) float64 in fit_motion's convention (frame_motions).  plate_code:
    None or uint8 (P, H, W) / (H, W), non-zero = the plate knows nothing there (background_plate's code); mask: None or uint8
    (n, h, w) / (h, w), non-zero = the vector is unknown (fb_check's).  low, high: the thresholds in grey levels on the window's
    mean difference; window: 0, 1 or 2 (1 x 1, 3 x 3, 5 x 5).
    Returns those asked for, in this order (one alone as itself): code uint8 (n, h, w) (CODES: 0 background, 1 foreground, 2 no
    plate there, 3 unknown, 4 strong foreground); diff int16 (n, h, w), the difference in 1/16 grey levels; evidence float32
    (n, h, w, 2) = (code == 4, diff / 16), the values for label_components(code, fg=(1, 4), ...) (foreground_objects); stats int64
    (n, 7) (STATS).  Asynchronous on the current stream."""
    wanted = (code, diff, evidence, stats)
    ox, oy = _plain(low, high, window, origin, wanted)
    if (flows is None) == (motions is None):
        raise FotgError("give the vectors frame -> reference either as flows or as motions")
    src = flows if flows is not None else motions
    if not isinstance(src, torch.Tensor) or src.dim() not in ((3, 4) if flows is not None else (1, 2)):
        raise FotgError("flows must be (n, h, w, 2) or (h, w, 2), motions (n, 6) or (6,)")
    single = src.dim() == (3 if flows is not None else 1)
    frames, ch = image_stack(frames, "frames", None, None, None, None, (torch.float32, torch.uint8), single=single)
    n, h, w = (int(v) for v in frames.shape[:3])
    if h > MAX_DIM or w > MAX_DIM or n > 65535:
        raise FotgError("frames must have between 1 and %d rows and columns" % MAX_DIM)
    dev = frames.device
    if single:
        src = src.unsqueeze(0)
    if flows is not None:
        src = _dev_f32(src, "flows", dev, (n, h, w, 2))
        fn = "fotg_subtract" if frames.dtype == torch.float32 else "fotg_subtract_u8"
    else:
        src = _dev_f32(src, "motions", dev, (n, 6), torch.float64)
        fn = "fotg_subtract_motion" if frames.dtype == torch.float32 else "fotg_subtract_motion_u8"
    plate, P, H, W, ix = _plates(plate, frames, index, n)
    if isinstance(plate_code, torch.Tensor) and plate_code.dim() == 2:
        plate_code = plate_code.unsqueeze(0)
    optional(plate_code, "plate_code", dev, (P, H, W), torch.uint8)
    mask = optional(mask, "mask", dev, (n, h, w), torch.uint8, single=single)
    outs = _outputs(n, h, w, dev, wanted)
    check(getattr(lib(), fn)(dev.index or 0, n, _ptr(frames), w, h, ch, P, _ptr(plate), W, H, ox, oy, ix, _ptr(src), _ptr(plate_code),
                             _ptr(mask), C.c_float(low), C.c_float(high), window, *(_ptr(o) for o in outs), _stream(dev)))
    return unbatch(outs, single)


def upsample_crop_subtract_background(ofc, coarse_flows, frames, plate, index=None, origin=(0, 0), plate_code=None, mask=None, low=8.0,
                                      high=24.0, window=1, code=True, diff=False, evidence=False, stats=False, fused=True):
    """The context's coarse flows (n, h_l, w_l, 2) -- a batch calc of the pairs (frame i, reference) -- and frames
    (n, h_org, w_org[, c]) -> byte for byte subtract_background(frames, plate, flows=ofc.upsample_crop(coarse_flows), ...).
    fused=True evaluates the upsampling inside the kernel and never writes a full-resolution flow; fused=False runs upsample_crop
    and the dense form."""
    wanted = (code, diff, evidence, stats)
    ox, oy = _plain(low, high, window, origin, wanted)
    two_channel(ofc, "the background subtraction needs a two-channel flow")
    n = int(coarse_flows.shape[0]) if isinstance(coarse_flows, torch.Tensor) and coarse_flows.dim() == 4 else 0
    if n < 1 or n > ofc.max_batch:
        raise FotgError("coarse_flows must be (n, h_l, w_l, 2) with 1 <= n <= max_batch = %d" % ofc.max_batch)
    frames, ch = image_stack(frames, "frames", n, ofc.height_org, ofc.width_org, ofc.device, (torch.float32, torch.uint8))
    coarse_shape(ofc, coarse_flows, "coarse_flows", n)
    h, w = ofc.height_org, ofc.width_org
    if not fused:
        return subtract_background(frames, plate, flows=ofc.upsample_crop(coarse_flows), index=index, origin=origin, plate_code=plate_code,
                                   mask=mask, low=low, high=high, window=window, code=code, diff=diff, evidence=evidence, stats=stats)
    plate, P, H, W, ix = _plates(plate, frames, index, n)
    if isinstance(plate_code, torch.Tensor) and plate_code.dim() == 2:
        plate_code = plate_code.unsqueeze(0)
    optional(plate_code, "plate_code", ofc.device, (P, H, W), torch.uint8)
    optional(mask, "mask", ofc.device, (n, h, w), torch.uint8)
    outs = _outputs(n, h, w, ofc.device, wanted)
    fn = lib().fotg_upsample_crop_subtract if frames.dtype == torch.float32 else lib().fotg_upsample_crop_subtract_u8
    check(fn(ofc._h, n, _ptr(coarse_flows), _ptr(frames), ch, P, _ptr(plate), W, H, ox, oy, ix, _ptr(plate_code), _ptr(mask), C.c_float(low),
             C.c_float(high), window, *(_ptr(o) for o in outs), _stream(ofc.device)))
    return unbatch(outs, False)


def frame_motions(motions):
    """motions (n, 6) float64, the rows of plate_motions (the maps reference -> frame) -> (n, 6): the maps frame -> reference, each
    row [I + A | t] inverted by motion._inverse in its written order.  A row that cannot be inverted is a FotgError."""
    from .motion import _inverse
    if not isinstance(motions, torch.Tensor) or motions.dim() != 2 or motions.shape[1] != 6 or motions.shape[0] < 1 \
            or motions.dtype != torch.float64:
        raise FotgError("motions must be a (n, 6) float64 tensor")
    m = (motions[:, 0] + 1.0, motions[:, 1], motions[:, 2], motions[:, 3], motions[:, 4] + 1.0, motions[:, 5])
    det = m[0] * m[4] - m[1] * m[3]
    if not bool((torch.isfinite(det) & (det != 0)).all()):
        raise FotgError("a motion cannot be inverted")
    i = _inverse(m)
    return torch.stack((i[0] - 1.0, i[1], i[2], i[3], i[4] - 1.0, i[5]), dim=1).contiguous()


def foreground_objects(code, evidence, connectivity=8, min_area=64, max_objects=256, open=0, close=0):
    """code and evidence of subtract_background -> (objects, ids, confirmed): label_components(code, fg=(1, 4), values=evidence,
    ids=True) and confirmed = objects[..., 9] > 0, a bool per row.  sum_u / 256 of a row is the number of strong (code 4) pixels
    of the component, so a component of weak pixels is confirmed only if it holds a strong one: the hysteresis.
    open > 0 or close > 0 (each 0 .. 8): the set fg = (1, 4) of the code map is cleaned first, cleaned = morph.clean_mask(code, open,
    close, fg=(1, 4)), and the components are those of the cleaned map: label_components(cleaned, fg=(1,), values=evidence, ids=True).
    confirmed keeps its meaning: a pixel the closing adds has evidence 0, a strong pixel the opening deletes belongs to no component."""
    from .objects import label_components
    if open or close:
        from .morph import clean_mask
        cleaned = clean_mask(code, open=open, close=close, fg=FG)
        objects, ids = label_components(cleaned, fg=(1,), connectivity=connectivity, values=evidence, min_area=min_area, max_objects=max_objects,
                                        ids=True)
        return objects, ids, objects[..., 9] > 0
    objects, ids = label_components(code, fg=FG, connectivity=connectivity, values=evidence, min_area=min_area, max_objects=max_objects,
                                    ids=True)
    return objects, ids, objects[..., 9] > 0


def foreground_mask(ids, confirmed):
    """ids int32 (n, h, w) / (h, w) and confirmed bool (n, max_objects) / (max_objects,) -> uint8 map of ids' shape: 1 on the pixels
    of the confirmed objects"""
    if not isinstance(ids, torch.Tensor) or not isinstance(confirmed, torch.Tensor) or ids.dim() not in (2, 3) \
            or confirmed.dim() != ids.dim() - 1 or confirmed.dtype != torch.bool or (ids.dim() == 3 and ids.shape[0] != confirmed.shape[0]):
        raise FotgError("ids must be (n, h, w) or (h, w), confirmed a bool tensor (n, max_objects) or (max_objects,)")
    single = ids.dim() == 2
    i3 = ids.unsqueeze(0) if single else ids
    c2 = confirmed.unsqueeze(0) if single else confirmed
    n, h, w = i3.shape
    hit = torch.gather(c2, 1, i3.clamp(min=0).long().view(n, -1)).view(n, h, w) & (i3 >= 0)
    hit = hit.to(torch.uint8)
    return hit[0] if single else hit


def ofc_foreground(ofc, frames, ref=0, model="affine", low=8.0, high=24.0, window=1, min_area=64, max_objects=256, mode="median",
                   exclude_moving=True, open=0, close=0):
    """OFClass.foreground: frames (T+1, h, w[, c]) -> (mask, objects, confirmed, plate, code).  The composition, call for call:
    OFClass.background on the frame grid (plate, its code, and the motions reference -> frame it used), frame_motions,
    subtract_background(frames, plate, motions=..., plate_code=the plate's code, ...) over all T + 1 frames with code and evidence,
    foreground_objects(code, evidence, 8, min_area, max_objects, open, close) -- with open or close above 0 on the code map cleaned
    by morph.clean_mask -- and foreground_mask.  mask uint8 (T+1, h, w): the pixels of the confirmed objects."""
    return _ofc_foreground(ofc, frames, ref, model, low, high, window, min_area, max_objects, mode, exclude_moving, open, close)[:5]


def _ofc_foreground(ofc, frames, ref, model, low, high, window, min_area, max_objects, mode, exclude_moving, open=0, close=0):
    """ofc_foreground's five results, then the plate's code and the motions frame -> reference it subtracted along (what
    flowonthego_amd.erase goes on with)"""
    from .plate import _ofc_plate
    _plain(low, high, window, (0, 0), (True,))
    if open or close:
        from .morph import _radius
        _radius(open, "open")
        _radius(close, "close")
    plate, pcode, _, motions = _ofc_plate(ofc, frames, ref=ref, model=model, mosaic=False, mode=mode, exclude_moving=exclude_moving,
                                          min_count=1)
    back = frame_motions(motions)
    code, evidence = subtract_background(frames, plate, motions=back, plate_code=pcode, low=low, high=high, window=window, code=True,
                                         evidence=True)
    objects, ids, confirmed = foreground_objects(code, evidence, 8, min_area, max_objects, open, close)
    return foreground_mask(ids, confirmed), objects, confirmed, plate, code, pcode, back


callable_module(__name__, __name__, "subtract_background")
