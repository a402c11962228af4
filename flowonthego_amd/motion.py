"""Global motion on the GPU: the one camera motion (translation, similarity or affine) that explains a flow field, the pixels that
do not follow it, and video stabilisation on top of it -- over fotg_fit_motion / fotg_upsample_crop_fit_motion / fotg_motion_flow
of libfotg.so.  The fit is a robust least-squares fit from exact 64-bit integer sums (no floating-point atomics: the same bits
every run, whatever the summation order); the definition, in order, is in include/fotg.h and csrc/motion.hip.h.  It runs in HIP
only; there is no CPU fallback."""
import ctypes as C

import torch

from ._args import _dev_f32, _ptr, _stream, coarse_flow, coarse_shape, dense_flow, optional, unbatch
from ._lib import FotgError, check, lib

MODELS = ("translation", "similarity", "affine")
CODES = ("follows", "independent", "masked", "unknown")
STATS = CODES + ("in_fit", "fitted")
SUMS = ("n", "X", "Y", "XX", "XY", "YY", "U", "XU", "YU", "V", "XV", "YV")
MAX_DIM = 16384


def _model(model):
    if model in MODELS:
        return MODELS.index(model)
    if isinstance(model, int) and not isinstance(model, bool) and 0 <= model < len(MODELS):
        return model
    raise FotgError("model must be one of %s" % (MODELS,))


def _fit_args(iters, thresh):
    if not isinstance(iters, int) or isinstance(iters, bool) or iters < 0 or iters > 64:
        raise FotgError("iters must be an integer in 0 .. 64")
    if not thresh >= 0:
        raise FotgError("thresh must be >= 0 (pixels)")


def _fit_outputs(n, h, w, device, code, residual, stats, sums):
    return (torch.empty((n, 6), dtype=torch.float64, device=device),
            torch.empty((n, h, w), dtype=torch.uint8, device=device) if code else None,
            torch.empty((n, h, w, 2), dtype=torch.float32, device=device) if residual else None,
            torch.empty((n, 6), dtype=torch.int64, device=device) if stats else None,
            torch.empty((n, 12), dtype=torch.int64, device=device) if sums else None)


def fit_motion(flow, mask=None, model="affine", iters=3, thresh=1.0, code=False, residual=False, stats=False, sums=False):
    """flow: device tensor (n, h, w, 2) or (h, w, 2) float32; mask: None or uint8 (n, h, w) / (h, w) in the alphabet of fb_check
    (only its code-0 pixels take part).  model: one of MODELS; iters: rounds of re-fitting on the pixels within thresh (pixels) of
    the previous round's motion, after the plain least-squares round 0.
    Returns params, float64 (n, 6) or (6,): [a00 a01 tx a10 a11 ty] of u = a00 x + a01 y + tx, v = a10 x + a11 y + ty in pixel
    coordinates.  With any of code / residual / stats / sums a tuple of params and those asked for, in this order: code uint8
    (n, h, w) (CODES: 0 follows the motion, 1 does not, 2 excluded by mask, 3 unknown: non-finite or beyond +-4096 px), residual
    float32 (n, h, w, 2) (flow minus the motion, == flow - motion_flow(params, w, h)), stats int64 (n, 6) (STATS: pixels of code
    0 .. 3, pixels in the last fit, fitted: 1 unless a round had too few pixels or a singular system), sums int64 (n, 12) (SUMS,
    the last round's).  Asynchronous on the current stream of the flow's device."""
    flow, single, n, h, w = dense_flow(flow, max_dim=MAX_DIM)
    mask = optional(mask, "mask", flow.device, (n, h, w), torch.uint8, single)
    _fit_args(iters, thresh)
    outs = _fit_outputs(n, h, w, flow.device, code, residual, stats, sums)
    check(lib().fotg_fit_motion(flow.device.index or 0, n, _ptr(flow), _ptr(mask), w, h, _model(model), iters, C.c_float(thresh),
                                *(_ptr(o) for o in outs), _stream(flow.device)))
    return unbatch(outs, single)


def motion_flow(params, w, h):
    """params: device tensor (n, 6) or (6,) float64 -> the motion as a dense flow, float32 (n, h, w, 2) or (h, w, 2), with exactly
    the arithmetic of fit_motion's residual.  What turns a fitted or smoothed camera motion into something warp() can apply."""
    if not isinstance(params, torch.Tensor) or params.dim() not in (1, 2) or params.shape[-1] != 6:
        raise FotgError("params must be a (n, 6) or (6,) tensor")
    single = params.dim() == 1
    p = params.unsqueeze(0) if single else params
    n = int(p.shape[0])
    if n < 1 or w < 1 or h < 1:
        raise FotgError("motion_flow needs n, w, h >= 1")
    _dev_f32(p, "params", dtype=torch.float64)
    flow = torch.empty((n, h, w, 2), dtype=torch.float32, device=p.device)
    check(lib().fotg_motion_flow(p.device.index or 0, n, _ptr(p), w, h, _ptr(flow), _stream(p.device)))
    return flow[0] if single else flow


def upsample_crop_fit_motion(ofc, flow, mask=None, model="affine", iters=3, thresh=1.0, code=False, residual=False, stats=False,
                             sums=False, fused=None):
    """OFClass.upsample_crop_fit_motion: the context's coarse flow (n, h_l, w_l, 2) -> byte for byte
    fit_motion(ofc.upsample_crop(flow), mask, ...); mask at the original size.  fused=True evaluates the upsampling inside every
    pass and never writes the full-resolution flow; fused=False runs upsample_crop and the dense fit.  The default, None, is the
    form that measured faster on 64 x 1080p: the fused one for iters == 0 (one pass or two: 0.67 against
    0.73 ms), the unfused one otherwise (every further pass pays the upsampling again: 3.37 against 2.85 ms at iters = 3)."""
    n = coarse_flow(ofc, flow, "the motion fit needs a two-channel flow", "flow")
    if fused is None:
        fused = iters == 0
    if not fused:
        return fit_motion(ofc.upsample_crop(flow), mask, model, iters, thresh, code, residual, stats, sums)
    coarse_shape(ofc, flow, "flow", n)
    h, w = ofc.height_org, ofc.width_org
    optional(mask, "mask", ofc.device, (n, h, w), torch.uint8)
    _fit_args(iters, thresh)
    outs = _fit_outputs(n, h, w, ofc.device, code, residual, stats, sums)
    check(lib().fotg_upsample_crop_fit_motion(ofc._h, n, _ptr(flow), _ptr(mask), _model(model), iters, C.c_float(thresh),
                                              *(_ptr(o) for o in outs), _stream(ofc.device)))
    return unbatch(outs, False)


def _sequence_flows(ofc, frames):
    """the coarse flows of frames (T+1, ...) and, on a bidir context, the forward mask of the consistency check"""
    if ofc.op.bidir:
        fw, bw = ofc.calc_sequence_bidirectional(frames)
        return fw, ofc.upsample_crop_fb_check(fw, bw)[0]
    return ofc.calc_sequence(frames), None


def camera_motion(ofc, frames, model="affine", iters=3, thresh=1.0, fused=None):
    """OFClass.camera_motion: frames (T+1, h, w[, channels]) -> (T, 6) float64, the motion frame k -> k+1 fitted to each flow of the
    sequence; on a context created with opt_params.bidir the occluded pixels (the forward mask of upsample_crop_fb_check) take no
    part"""
    fw, mask = _sequence_flows(ofc, frames)
    return upsample_crop_fit_motion(ofc, fw, mask, model, iters, thresh, fused=fused)


# ---- stabilisation ---------------------------------------------------------------------------------------------------------------
# A 2 x 3 affine map [m00 m01 m02; m10 m11 m12] (third row 0 0 1) is a tuple of six float64 tensors; every product and sum below is
# one element-wise torch operation, in the written order (tests/motion_ref.py follows it in numpy).
def _compose(A, B):
    """A . B"""
    a00, a01, a02, a10, a11, a12 = A
    b00, b01, b02, b10, b11, b12 = B
    return (a00 * b00 + a01 * b10, a00 * b01 + a01 * b11, (a00 * b02 + a01 * b12) + a02,
            a10 * b00 + a11 * b10, a10 * b01 + a11 * b11, (a10 * b02 + a11 * b12) + a12)


def _inverse(S):
    s00, s01, s02, s10, s11, s12 = S
    det = s00 * s11 - s01 * s10
    i00, i01, i10, i11 = s11 / det, -s01 / det, -s10 / det, s00 / det
    return (i00, i01, -(i00 * s02 + i01 * s12), i10, i11, -(i10 * s02 + i11 * s12))


def smoothing_motions(params, radius):
    """params (T, 6) float64, the motions frame k -> k+1 -> (T+1, 6): per frame k the parameters of C_k . S_k^-1 - I, where
    M_k = [I + A_k | t_k], C_0 = I, C_k = M_{k-1} . C_{k-1} and S_k is the entry-wise mean of C over the frames
    k - radius .. k + radius that exist (added in ascending order, then divided by their number)"""
    if not isinstance(params, torch.Tensor) or params.dim() != 2 or params.shape[1] != 6 or params.shape[0] < 1 or params.dtype != torch.float64:
        raise FotgError("params must be a (T, 6) float64 tensor")
    if not isinstance(radius, int) or isinstance(radius, bool) or radius < 0:
        raise FotgError("radius must be an integer >= 0")
    T = int(params.shape[0])
    one = torch.ones((), dtype=torch.float64, device=params.device)
    zero = torch.zeros((), dtype=torch.float64, device=params.device)
    path = [(one, zero, zero, zero, one, zero)]
    for k in range(T):
        p = params[k]
        path.append(_compose((p[0] + 1.0, p[1], p[2], p[3], p[4] + 1.0, p[5]), path[-1]))
    Cs = torch.stack([torch.stack(c) for c in path])                       # (T+1, 6)
    r = min(radius, T)
    pad = torch.zeros((T + 1 + 2 * r, 6), dtype=torch.float64, device=params.device)
    pad[r:r + T + 1] = Cs
    acc = pad[0:T + 1]
    for d in range(1, 2 * r + 1):
        acc = acc + pad[d:d + T + 1]
    cnt = torch.tensor([min(k + r, T) - max(k - r, 0) + 1 for k in range(T + 1)], dtype=torch.float64).to(params.device)
    S = acc / cnt[:, None]
    W = _compose(tuple(Cs[:, i] for i in range(6)), _inverse(tuple(S[:, i] for i in range(6))))
    return torch.stack((W[0] - 1.0, W[1], W[2], W[3], W[4] - 1.0, W[5]), dim=1).contiguous()


def stabilize(frames, flows, model="similarity", radius=15, mask=None, fill=None, stats=False, iters=3, thresh=1.0):
    """frames: device tensor (T+1, h, w) or (T+1, h, w, c), c in (1, 3), float32 or uint8; flows: (T, h, w, 2) float32, flows[k]
    the flow frame k -> k+1; mask: None or uint8 (T, h, w), pixels of each flow to leave out of the fit (fb_check's forward mask).
    The camera motion of every flow is fitted (fit_motion: model, iters, thresh), accumulated into a camera path, the path smoothed
    by a box mean of `radius` frames to either side, and frame k resampled at C_k . S_k^-1 . p (smoothing_motions, motion_flow,
    warp; fill as in warp).
    Returns (stabilised frames, the warp's codes uint8 (T+1, h, w)); with stats=True the warp's statistics (T+1, 6) as well.
    Asynchronous on the current stream."""
    from .warp import warp
    if not isinstance(frames, torch.Tensor) or frames.dim() not in (3, 4) or not isinstance(flows, torch.Tensor) or flows.dim() != 4:
        raise FotgError("frames must be (T+1, h, w[, c]) and flows (T, h, w, 2)")
    if frames.shape[0] != flows.shape[0] + 1 or tuple(frames.shape[1:3]) != tuple(flows.shape[1:3]):
        raise FotgError("frames %s do not go with flows %s" % (tuple(frames.shape), tuple(flows.shape)))
    params = fit_motion(flows, mask, model, iters, thresh)
    h, w = (int(v) for v in flows.shape[1:3])
    out, code, st = warp(frames, motion_flow(smoothing_motions(params, radius), w, h), fill=fill, stats=True)
    return (out, code, st) if stats else (out, code)


def ofc_stabilize(ofc, frames, model="similarity", radius=15, fill=None, stats=False, iters=3, thresh=1.0):
    """OFClass.stabilize: the flows of frames (T+1, ...) first (on a bidir context with the forward consistency mask), then
    stabilize() on them"""
    fw, mask = _sequence_flows(ofc, frames)
    return stabilize(frames, ofc.upsample_crop(fw), model, radius, mask, fill, stats, iters, thresh)
