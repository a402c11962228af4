"""Forward-backward consistency of a flow pair on the GPU (Sundaram, Brox & Keutzer, ECCV 2010), over fotg_fb_check /
fotg_upsample_crop_fb_check of libfotg.so.  Per pixel a uint8 code: 0 consistent, 1 occluded or inconsistent, 2 the vector leaves
the frame, 3 unknown (a non-finite vector).  The definition, in f32 and in order, is in include/fotg.h and csrc/fbcheck.hip.h.
The check runs in HIP only; there is no CPU fallback."""
import ctypes as C

import torch

from ._args import _ptr, _stream, coarse_flow, coarse_shape, dense_flow, flow_form, optional, unbatch
from ._lib import FotgError, check, lib

CODES = ("consistent", "occluded", "outside", "unknown")


def _masks(shape, device, stats):
    m = torch.empty(shape, dtype=torch.uint8, device=device)
    mb = torch.empty(shape, dtype=torch.uint8, device=device)
    cnt = torch.empty((shape[0], 2, 4), dtype=torch.int32, device=device) if stats else None
    return m, mb, cnt


def fb_check(fw, bw, alpha1=0.01, alpha2=0.5, stats=False):
    """fw, bw: device tensors (n, h, w, 2) or (h, w, 2) float32, the flows frame 0 -> 1 and frame 1 -> 0.
    Returns (mask, mask_bw) uint8 (n, h, w) or (h, w): mask over frame 0 (fw checked against bw), mask_bw over frame 1.
    stats=True also returns counts, int32 (n, 2, 4) or (2, 4): per direction the number of pixels of each code.
    Asynchronous on the current stream of the flows' device."""
    flow_form(fw, "fw")
    flow_form(bw, "bw")
    if fw.shape != bw.shape:
        raise FotgError("fw and bw differ in shape: %s and %s" % (tuple(fw.shape), tuple(bw.shape)))
    f, single, n, h, w = dense_flow(fw, "fw")
    b = optional(bw, "bw", f.device, f.shape, single=single)
    m, mb, cnt = _masks((n, h, w), f.device, stats)
    check(lib().fotg_fb_check(f.device.index or 0, n, _ptr(f), _ptr(b), w, h, C.c_float(alpha1), C.c_float(alpha2),
                              _ptr(m), _ptr(mb), _ptr(cnt), _stream(f.device)))
    return unbatch((m, mb, cnt), single, always_tuple=True)


def upsample_crop_fb_check(ofc, fw, bw, alpha1=0.01, alpha2=0.5, stats=False, fused=False):
    """OFClass.upsample_crop_fb_check: the context's coarse flows (n, h_l, w_l, 2) -> masks (n, h_org, w_org), byte for byte
    fb_check(ofc.upsample_crop(fw), ofc.upsample_crop(bw)).  fused=False (the default: measured 8 % faster at 64 x 1080p,
    DESIGN.md section 11) runs the two upsample_crop calls and the dense check; fused=True evaluates the upsampling inside the
    check and never writes either full-resolution flow (2 x 1.06 GB less HBM at 64 x 1080p)."""
    n = coarse_flow(ofc, fw, "the consistency check needs two-channel flows", "flows")
    if not fused:
        return fb_check(ofc.upsample_crop(fw), ofc.upsample_crop(bw), alpha1, alpha2, stats)
    coarse_shape(ofc, fw, "fw", n)
    coarse_shape(ofc, bw, "bw", n)
    m, mb, cnt = _masks((n, ofc.height_org, ofc.width_org), ofc.device, stats)
    check(lib().fotg_upsample_crop_fb_check(ofc._h, n, _ptr(fw), _ptr(bw), C.c_float(alpha1), C.c_float(alpha2),
                                            _ptr(m), _ptr(mb), _ptr(cnt), _stream(ofc.device)))
    return unbatch((m, mb, cnt), False, always_tuple=True)


# palette of the mask image: code 0 white, 1 red, 2 blue, 3 black
PALETTE = ((255, 255, 255), (255, 0, 0), (0, 0, 255), (0, 0, 0))


def mask_to_rgb(mask):
    """(h, w) uint8 codes (numpy or tensor) -> (h, w, 3) uint8 in PALETTE's colours, on the host"""
    import numpy as np
    if hasattr(mask, "detach"):
        mask = mask.detach().cpu().numpy()
    return np.asarray(PALETTE, np.uint8)[np.minimum(np.asarray(mask), 3)]
