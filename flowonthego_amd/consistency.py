"""Forward-backward consistency of a flow pair on the GPU (Sundaram, Brox & Keutzer, ECCV 2010), over fotg_fb_check /
fotg_upsample_crop_fb_check of libfotg.so.  Per pixel a uint8 code: 0 consistent, 1 occluded or inconsistent, 2 the vector leaves
the frame, 3 unknown (a non-finite vector).  The definition, in f32 and in order, is in include/fotg.h and csrc/fbcheck.hip.h.
The check runs in HIP only; there is no CPU fallback."""
import ctypes as C

import torch

from ._lib import FotgError, check, lib
from .oflow import _dev_f32, _ptr, _stream

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
    for t, nm in ((fw, "fw"), (bw, "bw")):
        if not isinstance(t, torch.Tensor) or t.dim() not in (3, 4) or t.shape[-1] != 2:
            raise FotgError("%s must be a (n, h, w, 2) or (h, w, 2) tensor" % nm)
    if fw.shape != bw.shape:
        raise FotgError("fw and bw differ in shape: %s and %s" % (tuple(fw.shape), tuple(bw.shape)))
    single = fw.dim() == 3
    f, b = (fw.unsqueeze(0), bw.unsqueeze(0)) if single else (fw, bw)
    n, h, w = (int(v) for v in f.shape[:3])
    if n < 1 or h < 1 or w < 1:
        raise FotgError("flow has an empty dimension: %s" % (tuple(fw.shape),))
    _dev_f32(f, "fw")
    _dev_f32(b, "bw", f.device)
    m, mb, cnt = _masks((n, h, w), f.device, stats)
    check(lib().fotg_fb_check(f.device.index or 0, n, _ptr(f), _ptr(b), w, h, C.c_float(alpha1), C.c_float(alpha2),
                              _ptr(m), _ptr(mb), _ptr(cnt), _stream(f.device)))
    if single:
        m, mb, cnt = m[0], mb[0], (cnt[0] if stats else None)
    return (m, mb, cnt) if stats else (m, mb)


def upsample_crop_fb_check(ofc, fw, bw, alpha1=0.01, alpha2=0.5, stats=False, fused=False):
    """OFClass.upsample_crop_fb_check: the context's coarse flows (n, h_l, w_l, 2) -> masks (n, h_org, w_org), byte for byte
    fb_check(ofc.upsample_crop(fw), ofc.upsample_crop(bw)).  fused=False (the default: measured 8 % faster at 64 x 1080p,
    DESIGN.md section 11) runs the two upsample_crop calls and the dense check; fused=True evaluates the upsampling inside the
    check and never writes either full-resolution flow (2 x 1.06 GB less HBM at 64 x 1080p)."""
    n = fw.shape[0] if isinstance(fw, torch.Tensor) and fw.dim() == 4 else 0
    if ofc.nch != 2:
        raise FotgError("the consistency check needs two-channel flows (this is a depth-mode context)")
    if n < 1 or n > ofc.max_batch:
        raise FotgError("flows must be (n, h_l, w_l, 2) with 1 <= n <= max_batch")
    if not fused:
        return fb_check(ofc.upsample_crop(fw), ofc.upsample_crop(bw), alpha1, alpha2, stats)
    w, h = ofc.out_size()
    _dev_f32(fw, "fw", ofc.device, (n, h, w, 2))
    _dev_f32(bw, "bw", ofc.device, (n, h, w, 2))
    m, mb, cnt = _masks((n, ofc.height_org, ofc.width_org), ofc.device, stats)
    check(lib().fotg_upsample_crop_fb_check(ofc._h, n, _ptr(fw), _ptr(bw), C.c_float(alpha1), C.c_float(alpha2),
                                            _ptr(m), _ptr(mb), _ptr(cnt), _stream(ofc.device)))
    return (m, mb, cnt) if stats else (m, mb)


# palette of the mask image: code 0 white, 1 red, 2 blue, 3 black
PALETTE = ((255, 255, 255), (255, 0, 0), (0, 0, 255), (0, 0, 0))


def mask_to_rgb(mask):
    """(h, w) uint8 codes (numpy or tensor) -> (h, w, 3) uint8 in PALETTE's colours, on the host"""
    import numpy as np
    if hasattr(mask, "detach"):
        mask = mask.detach().cpu().numpy()
    return np.asarray(PALETTE, np.uint8)[np.minimum(np.asarray(mask), 3)]
