"""Edge- and occlusion-aware filtering of a flow on the GPU, guided by the frame the flow belongs to, over fotg_flow_filter /
fotg_upsample_crop_flow_filter of libfotg.so: a joint (cross) bilateral filter of the vectors.  A vector becomes the mean of the
vectors of nearby pixels of similar colour, which pulls motion boundaries onto image edges; vectors a consistency mask rejects stay
out of the mean, and a rejected pixel is filled from the consistent vectors around it.  Per pixel a uint8 code: 0 filtered, 1 filled
from its neighbours, 3 no support (the vector is passed through).  The definition, in f32 and in order, is in include/fotg.h and
csrc/flowfilter.hip.h.  It runs in HIP only; there is no CPU fallback."""
import ctypes as C
import math

import torch

from ._args import _ptr, _stream, cat_chunks, coarse_flow, coarse_shape, dense_flow, image_stack, optional, two_channel, unbatch
from ._lib import FotgError, check, lib

CODES = ("filtered", "filled", None, "unsupported")
STATS = ("filtered", "filled", "unsupported", "sum_abs_change")
MAX_RADIUS = 7
MAX_ITERS = 4


def spatial_table(radius, sigma):
    """the table s[i] = exp(-i^2 / (2 sigma^2)), i = 0 .. radius, evaluated in float64 and rounded to float32: a list of floats"""
    if not isinstance(radius, int) or not 1 <= radius <= MAX_RADIUS:
        raise FotgError("radius must be 1 .. %d" % MAX_RADIUS)
    sigma = float(sigma)
    if not (sigma > 0 and math.isfinite(sigma)):
        raise FotgError("sigma must be a positive number")
    return [C.c_float(math.exp(-(i * i) / (2.0 * sigma * sigma))).value for i in range(radius + 1)]


def _spatial(radius, sigma, spatial):
    """-> ctypes float array of radius + 1 entries, or None (all ones)"""
    if not isinstance(radius, int) or not 1 <= radius <= MAX_RADIUS:
        raise FotgError("radius must be 1 .. %d" % MAX_RADIUS)
    if sigma is not None and spatial is not None:
        raise FotgError("give sigma or spatial, not both")
    if sigma is not None:
        spatial = spatial_table(radius, sigma)
    if spatial is None:
        return None
    if isinstance(spatial, torch.Tensor):
        if spatial.is_cuda:
            raise FotgError("spatial is a host array (it is validated on the host): pass a list, not a device tensor")
        spatial = spatial.tolist()
    s = [float(v) for v in (spatial.tolist() if hasattr(spatial, "tolist") else spatial)]
    if len(s) != radius + 1:
        raise FotgError("spatial must hold radius + 1 = %d values" % (radius + 1))
    return (C.c_float * len(s))(*s)


def _outputs(n, h, w, device, mask, code, stats, single):
    mask = optional(mask, "mask", device, (n, h, w), torch.uint8, single)
    want_code = code is None and stats or bool(code)
    out = torch.empty((n, h, w, 2), dtype=torch.float32, device=device)
    cd = torch.empty((n, h, w), dtype=torch.uint8, device=device) if want_code else None
    st = torch.empty((n, 4), dtype=torch.float64, device=device) if stats else None
    return mask, out, cd, st


def filter_flow(flow, guide, mask=None, radius=3, sigma=None, spatial=None, tau=20.0, iters=1, code=None, stats=False):
    """flow: device tensor (n, h, w, 2) or (h, w, 2) float32.  guide: the frame(s) the flow belongs to, (n, h, w[, c]) or (h, w[, c])
    with a single flow, c in (1, 3), float32 or uint8.  mask: None or uint8 (n, h, w) / (h, w), a mask of fb_check (only pixels of
    code 0 take part).  radius: 1 .. 7, the window is (2 radius + 1)^2.  sigma: None or the standard deviation of the Gaussian
    spatial weight (spatial_table); spatial: None or radius + 1 weights in [0, 1], the first positive (a host list); neither: a box.
    tau: the mean absolute guide difference per channel at which a neighbour's weight reaches 0.  iters: 1 .. 4 passes; each
    further pass fills the unsupported pixels within radius of a supported one.
    Returns out, the filtered flow; with code=True (out, code), code uint8: 0 filtered, 1 filled from its neighbours, 3 no support;
    with stats=True (out, code, stats), stats float64 (n, 4) / (4,): the pixels of code 0, 1 and 3 and the sum of |change| over the
    components of the code-0 pixels (STATS); stats=True, code=False leaves the code out.  Asynchronous on the current stream."""
    f, single, n, h, w = dense_flow(flow)
    g, ch = image_stack(guide, "guide", n, h, w, f.device, (torch.float32, torch.uint8), single)
    s = _spatial(radius, sigma, spatial)
    mask, out, cd, st = _outputs(n, h, w, f.device, mask, code, stats, single)
    fn = lib().fotg_flow_filter if g.dtype == torch.float32 else lib().fotg_flow_filter_u8
    check(fn(f.device.index or 0, n, _ptr(f), _ptr(g), w, h, ch, _ptr(mask), radius, s, C.c_float(tau), int(iters), _ptr(out),
             _ptr(cd), _ptr(st), _stream(f.device)))
    return unbatch((out, cd, st), single)


def upsample_crop_filter_flow(ofc, coarse, guide, mask=None, radius=3, sigma=None, spatial=None, tau=20.0, iters=1, code=None,
                              stats=False, fused=True):
    """The context's coarse flow (n, h_l, w_l, 2) and the guide (n, h_org, w_org[, c]) -> bit for bit
    filter_flow(ofc.upsample_crop(coarse), guide, ...), the statistics included.  fused=True evaluates the upsampling inside the
    filter and never writes the unfiltered full-resolution flow; fused=False runs upsample_crop and the dense filter."""
    n = coarse_flow(ofc, coarse, "the flow filter needs a two-channel flow")
    if not fused:
        return filter_flow(ofc.upsample_crop(coarse), guide, mask=mask, radius=radius, sigma=sigma, spatial=spatial, tau=tau,
                           iters=iters, code=code, stats=stats)
    coarse_shape(ofc, coarse, "coarse", n)
    h, w = ofc.height_org, ofc.width_org
    g, ch = image_stack(guide, "guide", n, h, w, ofc.device, (torch.float32, torch.uint8))
    s = _spatial(radius, sigma, spatial)
    mask, out, cd, st = _outputs(n, h, w, ofc.device, mask, code, stats, False)
    fn = lib().fotg_upsample_crop_flow_filter if g.dtype == torch.float32 else lib().fotg_upsample_crop_flow_filter_u8
    check(fn(ofc._h, n, _ptr(coarse), _ptr(g), ch, _ptr(mask), radius, s, C.c_float(tau), int(iters), _ptr(out), _ptr(cd), _ptr(st),
             _stream(ofc.device)))
    return unbatch((out, cd, st), False)


def ofc_calc_filtered(ofc, I0, I1, radius=3, sigma=None, spatial=None, tau=20.0, iters=1, occlusion=True, both=False, code=None,
                      stats=False):
    """OFClass.calc_filtered: the flow(s) of n frame pairs I0 -> I1 (n, h, w[, c]) float32 or uint8, filtered at full resolution
    with the frame they belong to as guide, max_batch pairs per chunk.  occlusion=True (a bidir context): both directions are
    computed, masked with upsample_crop_fb_check, and the forward flow is filtered with I0 as guide and its mask; both=True also
    returns the backward flow filtered with I1 as guide and mask_bw.  occlusion=False: the fused filter without a mask, on any
    context (both=True then needs a bidir context too).  Returns what upsample_crop_filter_flow returns; with both=True a pair of
    those, (forward, backward)."""
    two_channel(ofc, "the flow filter needs a two-channel flow")
    if (occlusion or both) and not ofc.op.bidir:
        raise FotgError("calc_filtered(occlusion=True) and (both=True) need a context created with opt_params.bidir = True")
    if not isinstance(I0, torch.Tensor) or not isinstance(I1, torch.Tensor) or I0.shape != I1.shape or I0.dim() < 3:
        raise FotgError("I0 and I1 must be tensors (n, h, w[, c]) of one shape")
    kw = dict(radius=radius, sigma=sigma, spatial=spatial, tau=tau, iters=iters, code=code, stats=stats)
    u8 = I0.dtype == torch.uint8
    parts = []
    for s in range(0, I0.shape[0], ofc.max_batch):
        a, b = I0[s:s + ofc.max_batch], I1[s:s + ofc.max_batch]
        m = mb = None
        if occlusion or both:
            fw, bw = ofc.bidirectional_flows(a, b)
            if occlusion:
                m, mb = ofc.upsample_crop_fb_check(fw, bw)
        else:
            fw = ofc.calc_batch_u8(a, b) if u8 else ofc.calc_batch(a, b)
        r = upsample_crop_filter_flow(ofc, fw, a, mask=m, **kw)
        parts.append((r, upsample_crop_filter_flow(ofc, bw, b, mask=mb, **kw)) if both else r)
    return cat_chunks(parts)
