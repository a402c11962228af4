"""Object removal on the GPU: a mask grown by a disc, feathered at its rim and filled from the plate (flowonthego_amd.plate) sampled
into the frame's own grid along the frame's motion, with the sampling rules of the background subtraction -- over fotg_erase /
fotg_erase_motion / fotg_upsample_crop_erase of libfotg.so.  The definition, in integers and f32 and in order, is in include/fotg.h
and csrc/erase.hip.h.  One kernel stages the mask of a tile and its halo on chip as bits, takes the capped distance to it in two
passes and writes every output once; a tile with nothing to remove is copied.  It runs in HIP only, there is no CPU fallback.
Where the plate knows nothing the frame is kept and the pixel is counted as a hole: nothing is inpainted here;
flowonthego_amd.fill.fill_removed fills exactly those pixels from the frame around them.

The module is callable: flowonthego_amd.erase(frames, plate, remove, ...) is flowonthego_amd.erase.remove_objects(frames, plate, remove, ...)."""
import torch

from ._args import _dev_f32, _ptr, _stream, coarse_shape, image_stack, optional, two_channel, unbatch
from ._lib import FotgError, callable_module, check, lib
from .subtract import MAX_DIM, MAX_ORIGIN, _plates

CODES = ("untouched", "replaced", "no_plate", "unknown", "blended")
STATS = CODES + ("holes", "removed", "sum_alpha")
MAX_GROW = 8
MAX_FEATHER = 8
FULL = 256                         # alpha of a pixel that is replaced outright


def _plain(grow, feather, origin, wanted):
    """what is decided from the plain arguments alone: (ox, oy)"""
    for v, name, top in ((grow, "grow", MAX_GROW), (feather, "feather", MAX_FEATHER)):
        if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v <= top:
            raise FotgError("%s must be an integer in 0 .. %d" % (name, top))
    try:
        ox, oy = (int(v) for v in origin)
    except (TypeError, ValueError):
        raise FotgError("origin must be (ox, oy)")
    if abs(ox) > MAX_ORIGIN or abs(oy) > MAX_ORIGIN:
        raise FotgError("origin must lie within +-%d" % MAX_ORIGIN)
    if not any(wanted):
        raise FotgError("ask for at least one of dst, code, alpha and stats")
    return ox, oy


def _outputs(frames, wanted):
    dst, code, alpha, stats = wanted
    n, h, w = frames.shape[:3]
    dev = frames.device
    return (torch.empty_like(frames) if dst else None,
            torch.empty((n, h, w), dtype=torch.uint8, device=dev) if code else None,
            torch.empty((n, h, w), dtype=torch.int16, device=dev) if alpha else None,
            torch.empty((n, len(STATS)), dtype=torch.int64, device=dev) if stats else None)


def remove_objects(frames, plate, remove, flows=None, motions=None, index=None, origin=(0, 0), plate_code=None, mask=None, grow=2,
                   feather=3, dst=True, code=False, alpha=False, stats=False):
    """frames, plate, flows | motions, index, origin, plate_code and mask as in subtract_background (single and batched forms
    alike).  remove: uint8 (n, h, w) / (h, w), non-zero = take this pixel out (foreground_mask's map); grow, feather: integers in
    0 .. 8, the radius of the disc the mask is grown by and the width of the ramp beyond it.
    Returns those asked for, in this order (one alone as itself): dst, the frames with the grown mask filled from the plate; code
    uint8 (n, h, w) (CODES: 0 untouched, 1 replaced, 2 no plate there -- kept, 3 unknown -- kept, 4 blended); alpha int16
    (n, h, w), the weight of the plate in 0 .. 256; stats int64 (n, 8) (STATS: the pixels of each code, the holes -- alpha 256 and
    code 2 or 3 --, the pixels of remove, the sum of alpha).  Asynchronous on the current stream."""
    wanted = (dst, code, alpha, stats)
    ox, oy = _plain(grow, feather, origin, wanted)
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
        fn = "fotg_erase" if frames.dtype == torch.float32 else "fotg_erase_u8"
    else:
        src = _dev_f32(src, "motions", dev, (n, 6), torch.float64)
        fn = "fotg_erase_motion" if frames.dtype == torch.float32 else "fotg_erase_motion_u8"
    plate, P, H, W, ix = _plates(plate, frames, index, n)
    if isinstance(plate_code, torch.Tensor) and plate_code.dim() == 2:
        plate_code = plate_code.unsqueeze(0)
    optional(plate_code, "plate_code", dev, (P, H, W), torch.uint8)
    mask = optional(mask, "mask", dev, (n, h, w), torch.uint8, single=single)
    if remove is None:
        raise FotgError("remove must be a uint8 map of the frames' size")
    remove = optional(remove, "remove", dev, (n, h, w), torch.uint8, single=single)
    outs = _outputs(frames, wanted)
    check(getattr(lib(), fn)(dev.index or 0, n, _ptr(frames), w, h, ch, P, _ptr(plate), W, H, ox, oy, ix, _ptr(src), _ptr(plate_code),
                             _ptr(mask), _ptr(remove), grow, feather, *(_ptr(o) for o in outs), _stream(dev)))
    return unbatch(outs, single)


def upsample_crop_remove_objects(ofc, coarse_flows, frames, plate, remove, index=None, origin=(0, 0), plate_code=None, mask=None, grow=2,
                                 feather=3, dst=True, code=False, alpha=False, stats=False, fused=True):
    """The context's coarse flows (n, h_l, w_l, 2) -- a batch calc of the pairs (frame i, reference) -- and frames
    (n, h_org, w_org[, c]) -> byte for byte remove_objects(frames, plate, remove, flows=ofc.upsample_crop(coarse_flows), ...).
    fused=True evaluates the upsampling inside the kernel, at the pixels under the grown mask only, and never writes a
    full-resolution flow; fused=False runs upsample_crop and the dense form."""
    wanted = (dst, code, alpha, stats)
    ox, oy = _plain(grow, feather, origin, wanted)
    two_channel(ofc, "the object removal needs a two-channel flow")
    n = int(coarse_flows.shape[0]) if isinstance(coarse_flows, torch.Tensor) and coarse_flows.dim() == 4 else 0
    if n < 1 or n > ofc.max_batch:
        raise FotgError("coarse_flows must be (n, h_l, w_l, 2) with 1 <= n <= max_batch = %d" % ofc.max_batch)
    frames, ch = image_stack(frames, "frames", n, ofc.height_org, ofc.width_org, ofc.device, (torch.float32, torch.uint8))
    coarse_shape(ofc, coarse_flows, "coarse_flows", n)
    h, w = ofc.height_org, ofc.width_org
    if not fused:
        return remove_objects(frames, plate, remove, flows=ofc.upsample_crop(coarse_flows), index=index, origin=origin, plate_code=plate_code,
                              mask=mask, grow=grow, feather=feather, dst=dst, code=code, alpha=alpha, stats=stats)
    plate, P, H, W, ix = _plates(plate, frames, index, n)
    if isinstance(plate_code, torch.Tensor) and plate_code.dim() == 2:
        plate_code = plate_code.unsqueeze(0)
    optional(plate_code, "plate_code", ofc.device, (P, H, W), torch.uint8)
    optional(mask, "mask", ofc.device, (n, h, w), torch.uint8)
    if remove is None:
        raise FotgError("remove must be a uint8 map of the frames' size")
    optional(remove, "remove", ofc.device, (n, h, w), torch.uint8)
    outs = _outputs(frames, wanted)
    fn = lib().fotg_upsample_crop_erase if frames.dtype == torch.float32 else lib().fotg_upsample_crop_erase_u8
    check(fn(ofc._h, n, _ptr(coarse_flows), _ptr(frames), ch, P, _ptr(plate), W, H, ox, oy, ix, _ptr(plate_code), _ptr(mask), _ptr(remove),
             grow, feather, *(_ptr(o) for o in outs), _stream(ofc.device)))
    return unbatch(outs, False)


def grow_mask(remove, grow):
    """remove: device uint8 (n, h, w) / (h, w), non-zero = set; grow in 0 .. 8 -> uint8 map of remove's shape: 1 on the dilation of
    the set pixels by the disc dx^2 + dy^2 <= grow^2.  It is alpha == 256 of fotg_erase with feather 0 and alpha as its only output:
    a pass that reads remove alone and needs no frames, no plate and no vectors."""
    _plain(grow, 0, (0, 0), (True,))
    if not isinstance(remove, torch.Tensor) or remove.dim() not in (2, 3) or remove.dtype != torch.uint8 or not remove.is_cuda:
        raise FotgError("remove must be a device uint8 tensor (n, h, w) or (h, w)")
    single = remove.dim() == 2
    rm = (remove.unsqueeze(0) if single else remove).contiguous()
    n, h, w = (int(v) for v in rm.shape)
    if not (1 <= h <= MAX_DIM and 1 <= w <= MAX_DIM and 1 <= n <= 65535):
        raise FotgError("remove must have between 1 and %d rows and columns" % MAX_DIM)
    alpha = torch.empty((n, h, w), dtype=torch.int16, device=rm.device)
    check(lib().fotg_erase(rm.device.index or 0, n, None, w, h, 1, 1, None, 1, 1, 0, 0, None, None, None, None, _ptr(rm), grow, 0, None,
                           None, _ptr(alpha), None, _stream(rm.device)))
    out = (alpha == FULL).to(torch.uint8)
    return out[0] if single else out


def ofc_remove_objects(ofc, frames, ref=0, model="affine", low=8.0, high=24.0, window=1, min_area=64, max_objects=256, grow=2, feather=3,
                       mask=None, open=0, close=0):
    """OFClass.remove_objects: frames (T+1, h, w[, c]) -> (clean, code, mask, plate).  The composition, call for call:
    OFClass.foreground(frames, ref, model, low, high, window, min_area, max_objects) for the mask of the confirmed objects and the
    plate, then remove_objects(frames, plate, mask, motions=frame_motions(the plate's motions), plate_code=the plate's code, grow=,
    feather=, dst=True, code=True) -- the code OFClass.background returns with this plate and the motions frame -> reference
    OFClass.foreground subtracted along; neither is computed again.  clean: the frames without the confirmed objects; code:
    remove_objects' code map (CODES).
    open, close: OFClass.foreground's, the radii the foreground is opened and closed by before the objects are taken (OFClass.remove_objects
    keeps its signature: the cleaning reaches the removal through this function and the tool's --open and --close).
    mask (the tool's --mask): a uint8 map (T+1, h, w) to take out instead; then nothing is subtracted: OFClass.background's plate,
    code and motions, and remove_objects with them."""
    _plain(grow, feather, (0, 0), (True,))
    if mask is None:
        from .subtract import _ofc_foreground
        mask, _, _, plate, _, pcode, back = _ofc_foreground(ofc, frames, ref, model, low, high, window, min_area, max_objects, "median", True,
                                                             open, close)
    else:
        from .plate import _ofc_plate
        from .subtract import frame_motions
        plate, pcode, _, motions = _ofc_plate(ofc, frames, ref=ref, model=model, mosaic=False, mode="median", exclude_moving=True, min_count=1)
        back = frame_motions(motions)
    clean, code = remove_objects(frames, plate, mask, motions=back, plate_code=pcode, grow=grow, feather=feather, dst=True, code=True)
    return clean, code, mask, plate


callable_module(__name__, __name__, "remove_objects")
