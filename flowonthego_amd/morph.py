"""Binary morphology of masks and code maps on the GPU: erode, dilate, open and close by a disc -- over fotg_morph of libfotg.so.
The definition is in include/fotg.h and csrc/morph.hip.h.  One kernel stages a tile and its halo on chip as bits, dilates the rows
with shifts and ors and writes every output once; an opening or a closing is one launch whose intermediate map never reaches
memory.  Exact, in integers; it runs in HIP only, there is no CPU fallback.  It is the step between the maps of subtract_background,
fit_motion and fb_check and the stages that read masks: label_components, foreground_mask, remove_objects,
background_plate(exclude=), track_objects, motion_histograms(ids=)."""
import ctypes as C

import torch

from ._args import _ptr, _stream, unbatch
from ._lib import FotgError, check, lib

OPS = ("erode", "dilate", "open", "close")
STATS = ("before", "after", "added", "removed")
MAX_RADIUS = 8
MAX_DIM = 16384
ERODE, DILATE = 0, 1
_STAGES = {"erode": (ERODE,), "dilate": (DILATE,), "open": (ERODE, DILATE), "close": (DILATE, ERODE)}


def _radius(r, name="radius"):
    if isinstance(r, bool) or not isinstance(r, int) or not 0 <= r <= MAX_RADIUS:
        raise FotgError("%s must be an integer in 0 .. %d" % (name, MAX_RADIUS))
    return r


def _fg_codes(fg):
    """None: every non-zero byte (0); otherwise label_components' 8-bit set of the codes 0 .. 7"""
    if fg is None:
        return 0
    from .objects import _fg_set
    return _fg_set(fg)


def chain(mask, stages, fg=None, out=True, stats=False):
    """mask: device uint8 (n, h, w) / (h, w); stages: one or two pairs (op, radius) with op "erode" or "dilate" and radius in
    0 .. 8, evaluated in this order in one launch; fg: None -- every non-zero byte is set -- or the byte values 0 .. 7 that are set,
    as for label_components.  Returns those asked for (one alone as itself): out uint8 of mask's shape, 0 or 1; stats int64
    (n, 4) / (4,) (STATS: the set pixels before and after, the pixels added and removed).  Asynchronous on the current stream."""
    try:
        stages = [(str(o), r) for o, r in stages]
    except (TypeError, ValueError):
        raise FotgError("stages must be one or two pairs (op, radius)")
    if len(stages) not in (1, 2) or any(o not in ("erode", "dilate") for o, _ in stages):
        raise FotgError('stages must be one or two pairs (op, radius) with op "erode" or "dilate"')
    for _, r in stages:
        _radius(r)
    fgc = _fg_codes(fg)
    if not (out or stats):
        raise FotgError("ask for at least one of out and stats")
    if not isinstance(mask, torch.Tensor) or mask.dim() not in (2, 3) or mask.dtype != torch.uint8 or not mask.is_cuda:
        raise FotgError("mask must be a device uint8 tensor (n, h, w) or (h, w)")
    single = mask.dim() == 2
    m = (mask.unsqueeze(0) if single else mask).contiguous()
    n, h, w = (int(v) for v in m.shape)
    if not (1 <= h <= MAX_DIM and 1 <= w <= MAX_DIM and 1 <= n <= 65535):
        raise FotgError("mask must have between 1 and %d rows and columns and at most 65535 maps" % MAX_DIM)
    dev = m.device
    outs = (torch.empty((n, h, w), dtype=torch.uint8, device=dev) if out else None,
            torch.empty((n, len(STATS)), dtype=torch.int64, device=dev) if stats else None)
    ops = (C.c_int * len(stages))(*(ERODE if o == "erode" else DILATE for o, _ in stages))
    radii = (C.c_int * len(stages))(*(r for _, r in stages))
    check(lib().fotg_morph(dev.index or 0, n, _ptr(m), w, h, fgc, len(stages), ops, radii, _ptr(outs[0]), _ptr(outs[1]), _stream(dev)))
    return unbatch(outs, single)


def morphology(mask, op, radius, fg=None, stats=False):
    """mask: device uint8 (n, h, w) / (h, w); op: "erode", "dilate", "open" (erode, then dilate) or "close" (dilate, then erode) by
    the disc dx^2 + dy^2 <= radius^2, radius an integer in 0 .. 8; fg as in chain.  Pixels outside the frame take no part: the
    border does not erode.  Returns the uint8 0 / 1 map of mask's shape, with stats=True (map, stats) -- one launch either way."""
    if op not in OPS:
        raise FotgError("op must be one of %s" % ", ".join(OPS))
    _radius(radius)
    return chain(mask, [("erode" if o == ERODE else "dilate", radius) for o in _STAGES[op]], fg=fg, out=True, stats=stats)


def clean_mask(mask, open=1, close=2, fg=None, stats=False):
    """morphology(morphology(mask, "open", open, fg), "close", close): the opening deletes what the disc of radius `open` does not
    fit into (speckle), the closing fills what the disc of radius `close` does not fit into (pin-holes, gaps).  A launch per part
    (the fused two-stage launch is the unit; DESIGN.md section 28 has the timings), none for a part of radius 0 unless it is the
    only one.  Returns the uint8 0 / 1 map; with stats=True (map, stats), stats int64 (n, 2, 4) / (2, 4): the opening's row and the
    closing's (STATS), a part that was not launched with nothing added and nothing removed."""
    _radius(open, "open")
    _radius(close, "close")
    if close == 0:
        first = morphology(mask, "open", open, fg=fg, stats=stats)
        if not stats:
            return first
        out, so = first
        sc = torch.stack((so[..., 1], so[..., 1], torch.zeros_like(so[..., 1]), torch.zeros_like(so[..., 1])), dim=-1)
        return out, torch.stack((so, sc), dim=-2)
    if open == 0:
        res = morphology(mask, "close", close, fg=fg, stats=stats)
        if not stats:
            return res
        out, sc = res
        so = torch.stack((sc[..., 0], sc[..., 0], torch.zeros_like(sc[..., 0]), torch.zeros_like(sc[..., 0])), dim=-1)
        return out, torch.stack((so, sc), dim=-2)
    first = morphology(mask, "open", open, fg=fg, stats=stats)
    if not stats:
        return morphology(first, "close", close)
    out, sc = morphology(first[0], "close", close, stats=True)
    return out, torch.stack((first[1], sc), dim=-2)
