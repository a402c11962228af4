"""Warp an image along a flow on the GPU (motion compensation), over fotg_warp / fotg_upsample_crop_warp of libfotg.so: the
reference's image_warp (kroeger/FDF1.0.1/opticalflow_aux.c:18-60) with per-pixel validity codes (the alphabet of
flowonthego_amd.consistency: 0 valid, 1 occluded, 2 the vector leaves the frame, 3 unknown) and photometric residuals.  The
definition, in f32 and in order, is in include/fotg.h and csrc/warp.hip.h.  The warp runs in HIP only; there is no CPU fallback.

The module is callable: flowonthego_amd.warp(src, flow, ...) is flowonthego_amd.warp.warp(src, flow, ...)."""
import ctypes as C

import torch

from ._args import _ptr, _stream, coarse_flow, coarse_shape, dense_flow, image_stack, optional, unbatch
from ._lib import callable_module, check, lib

STATS = ("valid", "occluded", "outside", "unknown", "sum_abs_warped", "sum_abs_unwarped")


def _images(src, ref, occ, n, h, w, device, single):
    """src / ref / occ of a batch of n flows of h x w checked and batched: (src, ref, occ, channels)"""
    src, ch = image_stack(src, "src", n, h, w, device, (torch.float32, torch.uint8), single)
    ref = optional(ref, "ref", device, src.shape, src.dtype, single)
    return src, ref, optional(occ, "occ", device, (n, h, w), torch.uint8, single), ch


def _outputs(src, n, h, w, stats):
    dst = torch.empty_like(src)
    code = torch.empty((n, h, w), dtype=torch.uint8, device=src.device) if stats else None
    st = torch.empty((n, 6), dtype=torch.float64, device=src.device) if stats else None
    return dst, code, st


def warp(src, flow, ref=None, occ=None, fill=None, stats=False):
    """src: device tensor (n, h, w) / (n, h, w, c) or a single image (h, w) / (h, w, c), c in (1, 3), float32 or uint8 -- the
    image to pull back (frame 1 for a forward flow); flow: (n, h, w, 2) or (h, w, 2) float32.
    occ: None or uint8 (n, h, w) / (h, w), a mask of fb_check (mask for the forward flow, mask_bw for the backward one).
    fill=None: reference mode (every pixel with a finite vector gets the value of the clamped taps, unknown ones 0);
    fill=V: every pixel whose code is not 0 gets V.
    ref: None or the image src is compared with (frame 0), for the residual sums.
    Returns dst (src's shape and dtype); with stats=True (dst, code, stats): the uint8 codes (n, h, w) and float64 (n, 6):
    pixels of code 0, 1, 2, 3, sum |ref - value| and sum |ref - src| over the code-0 pixels and all channels (STATS).
    A single (h, w, 3) image is told from a batch (n, h, w) by the flow's dimensions.  Asynchronous on the current stream."""
    flow, single, n, h, w = dense_flow(flow)
    src, ref, occ, ch = _images(src, ref, occ, n, h, w, flow.device, single)
    dst, cd, st = _outputs(src, n, h, w, stats)
    fn = lib().fotg_warp if src.dtype == torch.float32 else lib().fotg_warp_u8
    check(fn(flow.device.index or 0, n, _ptr(src), _ptr(flow), w, h, ch, _ptr(ref), _ptr(occ), 0 if fill is None else 1,
             C.c_float(0.0 if fill is None else fill), _ptr(dst), _ptr(cd), _ptr(st), _stream(flow.device)))
    return unbatch((dst, cd, st), single)


def upsample_crop_warp(ofc, flow, src, ref=None, occ=None, fill=None, stats=False, fused=True):
    """OFClass.upsample_crop_warp: the context's coarse flow (n, h_l, w_l, 2) and images (n, h_org, w_org[, c]) -> bit for bit
    warp(src, ofc.upsample_crop(flow), ...), the statistics included.  fused=True evaluates the upsampling inside the warp
    and never writes the full-resolution flow; fused=False runs upsample_crop and the dense warp."""
    n = coarse_flow(ofc, flow, "the warp needs a two-channel flow", "flow")
    if not fused:
        return warp(src, ofc.upsample_crop(flow), ref=ref, occ=occ, fill=fill, stats=stats)
    coarse_shape(ofc, flow, "flow", n)
    h, w = ofc.height_org, ofc.width_org
    src, ref, occ, ch = _images(src, ref, occ, n, h, w, ofc.device, False)
    dst, cd, st = _outputs(src, n, h, w, stats)
    fn = lib().fotg_upsample_crop_warp if src.dtype == torch.float32 else lib().fotg_upsample_crop_warp_u8
    check(fn(ofc._h, n, _ptr(flow), _ptr(src), ch, _ptr(ref), _ptr(occ), 0 if fill is None else 1,
             C.c_float(0.0 if fill is None else fill), _ptr(dst), _ptr(cd), _ptr(st), _stream(ofc.device)))
    return unbatch((dst, cd, st), False)


callable_module(__name__, __name__, "warp")
