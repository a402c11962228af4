"""Warp an image along a flow on the GPU (motion compensation), over fotg_warp / fotg_upsample_crop_warp of libfotg.so: the
reference's image_warp (kroeger/FDF1.0.1/opticalflow_aux.c:18-60) with per-pixel validity codes (the alphabet of
flowonthego_amd.consistency: 0 valid, 1 occluded, 2 the vector leaves the frame, 3 unknown) and photometric residuals.  The
definition, in f32 and in order, is in include/fotg.h and csrc/warp.hip.h.  The warp runs in HIP only; there is no CPU fallback.

The module is callable: flowonthego_amd.warp(src, flow, ...) is flowonthego_amd.warp.warp(src, flow, ...)."""
import ctypes as C

import torch

from ._lib import FotgError, callable_module, check, lib
from .oflow import _dev_f32, _ptr, _stream

STATS = ("valid", "occluded", "outside", "unknown", "sum_abs_warped", "sum_abs_unwarped")


def _images(src, ref, occ, n_flow, h, w, device):
    """src / ref / occ of a batch of n_flow flows of h x w checked: (dtype, channels)"""
    if not isinstance(src, torch.Tensor) or src.dim() not in (3, 4) or src.dtype not in (torch.float32, torch.uint8):
        raise FotgError("src must be a (n, h, w) or (n, h, w, c) float32 or uint8 tensor")
    ch = 1 if src.dim() == 3 else int(src.shape[3])
    if ch not in (1, 3) or tuple(src.shape[:3]) != (n_flow, h, w):
        raise FotgError("src has shape %s, expected (%d, %d, %d) or (%d, %d, %d, 1 | 3)" % (tuple(src.shape), n_flow, h, w, n_flow, h, w))
    _dev_f32(src, "src", device, dtype=src.dtype)
    if ref is not None:
        _dev_f32(ref, "ref", device, tuple(src.shape), dtype=src.dtype)
    if occ is not None:
        _dev_f32(occ, "occ", device, (n_flow, h, w), dtype=torch.uint8)
    return src.dtype, ch


def _outputs(src, n, h, w, stats):
    dst = torch.empty_like(src)
    code = torch.empty((n, h, w), dtype=torch.uint8, device=src.device) if stats else None
    st = torch.empty((n, 6), dtype=torch.float64, device=src.device) if stats else None
    return dst, code, st


def _result(dst, code, st, single, stats):
    if not stats:
        return dst[0] if single else dst
    return (dst[0], code[0], st[0]) if single else (dst, code, st)


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
    if not isinstance(flow, torch.Tensor) or flow.dim() not in (3, 4) or flow.shape[-1] != 2:
        raise FotgError("flow must be a (n, h, w, 2) or (h, w, 2) tensor")
    single = flow.dim() == 3
    if single:
        flow = flow.unsqueeze(0)
        src = src.unsqueeze(0) if isinstance(src, torch.Tensor) else src
        ref = ref.unsqueeze(0) if ref is not None else None
        occ = occ.unsqueeze(0) if occ is not None else None
    n, h, w = (int(v) for v in flow.shape[:3])
    if n < 1 or h < 1 or w < 1:
        raise FotgError("flow has an empty dimension: %s" % (tuple(flow.shape),))
    _dev_f32(flow, "flow")
    dtype, ch = _images(src, ref, occ, n, h, w, flow.device)
    dst, cd, st = _outputs(src, n, h, w, stats)
    fn = lib().fotg_warp if dtype == torch.float32 else lib().fotg_warp_u8
    check(fn(flow.device.index or 0, n, _ptr(src), _ptr(flow), w, h, ch, _ptr(ref), _ptr(occ), 0 if fill is None else 1,
             C.c_float(0.0 if fill is None else fill), _ptr(dst), _ptr(cd), _ptr(st), _stream(flow.device)))
    return _result(dst, cd, st, single, stats)


def upsample_crop_warp(ofc, flow, src, ref=None, occ=None, fill=None, stats=False, fused=True):
    """OFClass.upsample_crop_warp: the context's coarse flow (n, h_l, w_l, 2) and images (n, h_org, w_org[, c]) -> bit for bit
    warp(src, ofc.upsample_crop(flow), ...), the statistics included.  fused=True evaluates the upsampling inside the warp
    and never writes the full-resolution flow; fused=False runs upsample_crop and the dense warp."""
    n = flow.shape[0] if isinstance(flow, torch.Tensor) and flow.dim() == 4 else 0
    if ofc.nch != 2:
        raise FotgError("the warp needs a two-channel flow (this is a depth-mode context)")
    if n < 1 or n > ofc.max_batch:
        raise FotgError("flow must be (n, h_l, w_l, 2) with 1 <= n <= max_batch")
    if not fused:
        return warp(src, ofc.upsample_crop(flow), ref=ref, occ=occ, fill=fill, stats=stats)
    wl, hl = ofc.out_size()
    _dev_f32(flow, "flow", ofc.device, (n, hl, wl, 2))
    h, w = ofc.height_org, ofc.width_org
    dtype, ch = _images(src, ref, occ, n, h, w, ofc.device)
    dst, cd, st = _outputs(src, n, h, w, stats)
    fn = lib().fotg_upsample_crop_warp if dtype == torch.float32 else lib().fotg_upsample_crop_warp_u8
    check(fn(ofc._h, n, _ptr(flow), _ptr(src), ch, _ptr(ref), _ptr(occ), 0 if fill is None else 1,
             C.c_float(0.0 if fill is None else fill), _ptr(dst), _ptr(cd), _ptr(st), _stream(ofc.device)))
    return _result(dst, cd, st, False, stats)


callable_module(__name__, __name__, "warp")
