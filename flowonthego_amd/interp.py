"""The frame at time t between two frames on the GPU (frame-rate up-conversion, slow motion, dropped-frame repair), over
fotg_interp / fotg_upsample_crop_interp of libfotg.so: the interpolation procedure of the Middlebury flow benchmark (Baker et al.,
"A Database and Evaluation Methodology for Optical Flow", section 3.3) on a bidirectional flow and its consistency masks.  The
definition, in f32 and in order, is in include/fotg.h and csrc/interp.hip.h.  It runs in HIP only; there is no CPU fallback.

Code byte per pixel: origin (0 the vector came from the forward flow, 1 from the backward flow, 2 a hole: no vector, plain blend)
+ 4 (only frame 0 was used) + 8 (only frame 1 was used)."""
import ctypes as C

import torch

from ._args import _dev_f32, _ptr, _stream, batched, coarse_flow, coarse_shape, dense_flow, flow_form, image_stack, optional
from ._lib import FotgError, check, lib

STATS = ("from_forward", "from_backward", "holes", "one_sided", "sum_abs_interpolated", "sum_abs_blend")


def _frames(I0, I1, ref, mask_fw, mask_bw, n, h, w, device, single):
    """the frames, ref and masks of a batch of n flows of h x w checked and batched: (I0, I1, ref, mask_fw, mask_bw, channels)"""
    I0, ch = image_stack(I0, "I0", n, h, w, device, (torch.float32, torch.uint8), single)
    I1 = _dev_f32(batched(I1, single), "I1", device, I0.shape, I0.dtype)
    if (mask_fw is None) != (mask_bw is None):
        raise FotgError("give both masks or neither")
    return (I0, I1, optional(ref, "ref", device, I0.shape, I0.dtype, single), optional(mask_fw, "mask_fw", device, (n, h, w), torch.uint8, single),
            optional(mask_bw, "mask_bw", device, (n, h, w), torch.uint8, single), ch)


def _times(t):
    """t or a sequence of t -> (list of floats, whether it was a sequence)"""
    seq = isinstance(t, (list, tuple)) or (isinstance(t, torch.Tensor) and t.dim() > 0) or (hasattr(t, "ndim") and t.ndim > 0)
    ts = [float(v) for v in t] if seq else [float(t)]
    if not ts or any(not (0.0 < v < 1.0) for v in ts):
        raise FotgError("t must lie strictly between 0 and 1")
    return ts, seq


def _run(call, I0, n, h, w, ts, seq, single, stats):
    """call(t, dst, code, st) once per t; the outputs stacked over t when t was a sequence"""
    k = len(ts)
    dst = torch.empty((k,) + tuple(I0.shape), dtype=I0.dtype, device=I0.device)
    code = torch.empty((k, n, h, w), dtype=torch.uint8, device=I0.device) if stats else None
    st = torch.empty((k, n, 6), dtype=torch.float64, device=I0.device) if stats else None
    for i, t in enumerate(ts):
        call(C.c_float(t), dst[i], code[i] if stats else None, st[i] if stats else None)
    outs = [dst, code, st] if stats else [dst]
    if single:
        outs = [o[:, 0] for o in outs]
    if not seq:
        outs = [o[0] for o in outs]
    return tuple(outs) if stats else outs[0]


def interpolate(I0, I1, flow_fw, flow_bw, t, mask_fw=None, mask_bw=None, ref=None, stats=False, alpha1=0.01, alpha2=0.5):
    """I0, I1: device tensors (n, h, w) / (n, h, w, c) or single images (h, w) / (h, w, c), c in (1, 3), float32 or uint8;
    flow_fw (frame 0 -> 1), flow_bw (frame 1 -> 0): (n, h, w, 2) or (h, w, 2) float32, full resolution.
    t: 0 < t < 1, or a sequence of such values: the outputs then gain a leading dimension, one entry per t.
    mask_fw, mask_bw: the masks of fb_check(flow_fw, flow_bw); None: the call runs the check itself (alpha1, alpha2).
    ref: None or the true frame at t (the layout of I0), for the residual sums.
    Returns dst (I0's shape and dtype); with stats=True (dst, code, stats): the uint8 codes (n, h, w) and float64 (n, 6) (STATS):
    pixels whose vector came from the forward flow, from the backward flow, holes, one-sided pixels, sum |ref - dst| and
    sum |ref - ((1 - t) I0 + t I1)| over all pixels and channels (the unrounded values).
    A single (h, w, 3) image is told from a batch (n, h, w) by the flows' dimensions.  Asynchronous on the current stream."""
    flow_form(flow_bw, "flow_bw")
    flow_fw, single, n, h, w = dense_flow(flow_fw, "flow_fw")
    flow_bw = optional(flow_bw, "flow_bw", flow_fw.device, flow_fw.shape, single=single)
    I0, I1, ref, mask_fw, mask_bw, ch = _frames(I0, I1, ref, mask_fw, mask_bw, n, h, w, flow_fw.device, single)
    ts, seq = _times(t)
    fn = lib().fotg_interp if I0.dtype == torch.float32 else lib().fotg_interp_u8
    dev = flow_fw.device

    def call(tc, dst, code, st):
        check(fn(dev.index or 0, n, _ptr(I0), _ptr(I1), _ptr(flow_fw), _ptr(flow_bw), w, h, ch, tc, _ptr(mask_fw), _ptr(mask_bw),
                 C.c_float(alpha1), C.c_float(alpha2), _ptr(ref), _ptr(dst), _ptr(code), _ptr(st), _stream(dev)))
    return _run(call, I0, n, h, w, ts, seq, single, stats)


def upsample_crop_interpolate(ofc, flow_fw, flow_bw, I0, I1, t, mask_fw=None, mask_bw=None, ref=None, stats=False, alpha1=0.01,
                              alpha2=0.5, fused=True):
    """OFClass.upsample_crop_interpolate: the coarse flows of a bidirectional context (n, h_l, w_l, 2) and frames
    (n, h_org, w_org[, c]) -> byte for byte interpolate(I0, I1, ofc.upsample_crop(flow_fw), ofc.upsample_crop(flow_bw), t, ...),
    the statistics included.  fused=True evaluates the upsampling (and, without masks, the consistency check) inside the call and
    never writes a full-resolution flow; fused=False runs upsample_crop and the dense form."""
    n = coarse_flow(ofc, flow_fw, "the interpolation needs two-channel flows", "flows")
    if not fused:
        return interpolate(I0, I1, ofc.upsample_crop(flow_fw), ofc.upsample_crop(flow_bw), t, mask_fw=mask_fw, mask_bw=mask_bw,
                           ref=ref, stats=stats, alpha1=alpha1, alpha2=alpha2)
    coarse_shape(ofc, flow_fw, "flow_fw", n)
    coarse_shape(ofc, flow_bw, "flow_bw", n)
    h, w = ofc.height_org, ofc.width_org
    I0, I1, ref, mask_fw, mask_bw, ch = _frames(I0, I1, ref, mask_fw, mask_bw, n, h, w, ofc.device, False)
    ts, seq = _times(t)
    fn = lib().fotg_upsample_crop_interp if I0.dtype == torch.float32 else lib().fotg_upsample_crop_interp_u8

    def call(tc, dst, code, st):
        check(fn(ofc._h, n, _ptr(flow_fw), _ptr(flow_bw), _ptr(I0), _ptr(I1), ch, tc, _ptr(mask_fw), _ptr(mask_bw), C.c_float(alpha1),
                 C.c_float(alpha2), _ptr(ref), _ptr(dst), _ptr(code), _ptr(st), _stream(ofc.device)))
    return _run(call, I0, n, h, w, ts, seq, False, stats)


def flow_and_interpolate(ofc, I0, I1, t, ref=None, stats=False, alpha1=0.01, alpha2=0.5, fused=True):
    """OFClass.interpolate: calc_bidirectional (or its 8-bit form, by the frames' dtype), the consistency check and the
    interpolation at t, for n pairs (n, h_org, w_org[, c]) or one pair (h_org, w_org[, c])"""
    if not isinstance(I0, torch.Tensor) or not isinstance(I1, torch.Tensor):
        raise FotgError("I0 and I1 must be tensors")
    u8 = I0.dtype == torch.uint8
    frame_dims = 2 + (1 if (ofc._u8_channels() if u8 else ofc.op.channels > 1) else 0)
    single = I0.dim() == frame_dims
    if single:
        I0, I1, ref = I0.unsqueeze(0), I1.unsqueeze(0), (ref.unsqueeze(0) if ref is not None else None)
    fw, bw = ofc.bidirectional_flows(I0, I1)
    out = upsample_crop_interpolate(ofc, fw, bw, I0, I1, t, ref=ref, stats=stats, alpha1=alpha1, alpha2=alpha2, fused=fused)
    if not single:
        return out
    _, seq = _times(t)
    pick = (lambda o: o[:, 0]) if seq else (lambda o: o[0])
    return tuple(pick(o) for o in out) if stats else pick(out)
