"""Flow chaining on the GPU: a position followed through the T flows of a sequence (long-range flow, point tracks), over
fotg_flow_chain / fotg_track_points of libfotg.so and their fused forms.  Per chain a uint8 code in the alphabet of
flowonthego_amd.consistency (0 valid to the end, 1 occluded / inconsistent, 2 leaves the frame, 3 unknown) and the number of steps
it was followed.  The definition, in f32 and in order, is in include/fotg.h and csrc/chain.hip.h.  One launch walks all T steps;
the chain runs in HIP only, there is no CPU fallback.

The module is callable: flowonthego_amd.chain(flows, ...) is flowonthego_amd.chain.chain(flows, ...)."""
import ctypes as C

import torch

from ._args import _dev_f32, _ptr, _stream, coarse_flow, coarse_shape, optional, unbatch
from ._lib import FotgError, callable_module, check, lib

STATS = ("valid", "occluded", "outside", "unknown", "sum_steps")


def _sequences(flows, flows_bw):
    """flows (T, h, w, 2) or (n_seq, T, h, w, 2), flows_bw None or alike, checked: (flows5, bw5, single)"""
    if not isinstance(flows, torch.Tensor) or flows.dim() not in (4, 5) or flows.shape[-1] != 2:
        raise FotgError("flows must be a (T, h, w, 2) or (n_seq, T, h, w, 2) tensor")
    single = flows.dim() == 4
    if flows_bw is not None and (not isinstance(flows_bw, torch.Tensor) or flows_bw.shape != flows.shape):
        raise FotgError("flows_bw must have the shape of flows, %s" % (tuple(flows.shape),))
    f = flows.unsqueeze(0) if single else flows
    if min(int(v) for v in f.shape) < 1:
        raise FotgError("flows has an empty dimension: %s" % (tuple(flows.shape),))
    _dev_f32(f, "flows")
    return f, optional(flows_bw, "flows_bw", f.device, f.shape, single=single), single


def _points(points, n_seq, device):
    """points (P, 2) or (n_seq, P, 2) checked -> (n_seq, P, 2); a (P, 2) set is tracked in every sequence"""
    if not isinstance(points, torch.Tensor) or points.dim() not in (2, 3) or points.shape[-1] != 2 or points.shape[-2] < 1:
        raise FotgError("points must be a (P, 2) or (n_seq, P, 2) tensor of (x, y)")
    if points.dim() == 2:
        points = points.unsqueeze(0).expand(n_seq, -1, -1).contiguous()
    return _dev_f32(points, "points", device, (n_seq, points.shape[1], 2))


def _dense_out(n_seq, h, w, device, stats):
    total = torch.empty((n_seq, h, w, 2), dtype=torch.float32, device=device)
    code = torch.empty((n_seq, h, w), dtype=torch.uint8, device=device)
    steps = torch.empty((n_seq, h, w), dtype=torch.int32, device=device)
    st = torch.empty((n_seq, 5), dtype=torch.int64, device=device) if stats else None
    return total, code, steps, st


def _points_out(n_seq, T, P, device, stats):
    traj = torch.empty((n_seq, T + 1, P, 2), dtype=torch.float32, device=device)
    code = torch.empty((n_seq, P), dtype=torch.uint8, device=device)
    steps = torch.empty((n_seq, P), dtype=torch.int32, device=device)
    st = torch.empty((n_seq, 5), dtype=torch.int64, device=device) if stats else None
    return traj, code, steps, st


def chain(flows, flows_bw=None, alpha1=0.01, alpha2=0.5, stats=False):
    """flows: device tensor (T, h, w, 2) or (n_seq, T, h, w, 2) float32, flows[k] the flow frame k -> k+1; flows_bw: None or alike,
    flows_bw[k] the flow frame k+1 -> k (then every step is tested for forward-backward consistency, alpha1 and alpha2 as in
    fb_check).  One chain per pixel of frame 0.
    Returns (total, code, steps): the displacement frame 0 -> T float32 (h, w, 2), the codes uint8 (h, w) and the accepted steps
    int32 (h, w), with a leading n_seq for a batch of sequences; a stopped chain keeps its last accepted displacement.
    stats=True also returns int64 (5,) or (n_seq, 5): chains ending with code 0, 1, 2, 3 and the sum of steps (STATS).
    Asynchronous on the current stream of the flows' device."""
    f, b, single = _sequences(flows, flows_bw)
    n_seq, T, h, w = (int(v) for v in f.shape[:4])
    outs = _dense_out(n_seq, h, w, f.device, stats)
    check(lib().fotg_flow_chain(f.device.index or 0, n_seq, T, _ptr(f), _ptr(b), w, h, C.c_float(alpha1), C.c_float(alpha2),
                                *(_ptr(o) for o in outs), _stream(f.device)))
    return unbatch(outs, single, always_tuple=True)


def track_points(points, flows, flows_bw=None, alpha1=0.01, alpha2=0.5, stats=False):
    """points: device tensor (P, 2) or (n_seq, P, 2) float32, (x, y) in pixels of frame 0, anywhere (a point outside the frame
    gets code 2 at once, a non-finite one code 3); flows, flows_bw as in chain().
    Returns (traj, code, steps): traj float32 (T+1, P, 2), the position in every frame (traj[0] the start; the frozen position
    is repeated once a chain has stopped), code uint8 (P,), steps int32 (P,), with a leading n_seq for a batch of sequences;
    stats=True also returns the five counters of chain().  Asynchronous on the current stream."""
    f, b, single = _sequences(flows, flows_bw)
    n_seq, T, h, w = (int(v) for v in f.shape[:4])
    pts = _points(points, n_seq, f.device)
    P = int(pts.shape[1])
    outs = _points_out(n_seq, T, P, f.device, stats)
    check(lib().fotg_track_points(f.device.index or 0, n_seq, T, _ptr(f), _ptr(b), w, h, C.c_float(alpha1), C.c_float(alpha2), P,
                                  _ptr(pts), *(_ptr(o) for o in outs), _stream(f.device)))
    return unbatch(outs, single, always_tuple=True)


def _coarse(ofc, flows, flows_bw):
    """the context's coarse flows (T, h_l, w_l, 2) of one sequence checked: T"""
    T = coarse_flow(ofc, flows, "the chain needs two-channel flows", "flows", "T")
    coarse_shape(ofc, flows, "flows", T)
    if flows_bw is not None:
        coarse_shape(ofc, flows_bw, "flows_bw", T)
    return T


def upsample_crop_chain(ofc, flows, flows_bw=None, alpha1=0.01, alpha2=0.5, stats=False, fused=None):
    """OFClass.upsample_crop_chain: the T coarse flows of one sequence (the outflow of calc_sequence, and that of
    calc_sequence_bidirectional as flows_bw) -> byte for byte chain(ofc.upsample_crop(flows), ofc.upsample_crop(flows_bw)).
    fused=True evaluates the upsampling at every tap and never writes a full-resolution flow; fused=False runs upsample_crop and
    the dense chain.  The default, None, is the form that measured faster at 1080p, T = 8: the fused one
    with backward flows (1.08 times faster), the unfused one without (1.20 times faster)."""
    T = _coarse(ofc, flows, flows_bw)
    if fused is None:
        fused = flows_bw is not None
    if not fused:
        return chain(ofc.upsample_crop(flows), None if flows_bw is None else ofc.upsample_crop(flows_bw), alpha1, alpha2, stats)
    outs = _dense_out(1, ofc.height_org, ofc.width_org, ofc.device, stats)
    check(lib().fotg_upsample_crop_flow_chain(ofc._h, T, _ptr(flows), _ptr(flows_bw), C.c_float(alpha1), C.c_float(alpha2),
                                              *(_ptr(o) for o in outs), _stream(ofc.device)))
    return unbatch(outs, True, always_tuple=True)


def upsample_crop_track_points(ofc, points, flows, flows_bw=None, alpha1=0.01, alpha2=0.5, stats=False, fused=False):
    """OFClass.upsample_crop_track_points: points (P, 2) in pixels of the original frame 0 along the T coarse flows of one sequence
    -> byte for byte track_points(points, ofc.upsample_crop(flows), ofc.upsample_crop(flows_bw)).  fused=True evaluates the
    upsampling at the taps of the points alone; the two forms of the point tracks have not been timed, so the default is the form
    whose taps are plain loads."""
    T = _coarse(ofc, flows, flows_bw)
    if not fused:
        return track_points(points, ofc.upsample_crop(flows), None if flows_bw is None else ofc.upsample_crop(flows_bw), alpha1, alpha2, stats)
    if not isinstance(points, torch.Tensor) or points.dim() != 2:
        raise FotgError("points must be a (P, 2) tensor of (x, y)")
    pts = _points(points, 1, ofc.device)
    P = int(pts.shape[1])
    outs = _points_out(1, T, P, ofc.device, stats)
    check(lib().fotg_upsample_crop_track_points(ofc._h, T, _ptr(flows), _ptr(flows_bw), C.c_float(alpha1), C.c_float(alpha2), P, _ptr(pts),
                                                *(_ptr(o) for o in outs), _stream(ofc.device)))
    return unbatch(outs, True, always_tuple=True)


def track(ofc, frames, points=None, alpha1=0.01, alpha2=0.5, stats=False, fused=None):
    """OFClass.track: frames (T+1, h, w[, channels]) float32 or uint8 -> the flows of the sequence (both directions on a context
    created with opt_params.bidir, then every step is tested for occlusion; forward only otherwise) and their chain: dense
    (total, code, steps) when points is None, else (traj, code, steps) of the (P, 2) points; fused=None is the default of
    upsample_crop_chain or upsample_crop_track_points"""
    if ofc.op.bidir:
        fw, bw = ofc.calc_sequence_bidirectional(frames)
    else:
        fw, bw = ofc.calc_sequence(frames), None
    if points is None:
        return upsample_crop_chain(ofc, fw, bw, alpha1, alpha2, stats, fused)
    # (None is False here: the point forms have not been timed, so there is no "by measurement" for them)
    return upsample_crop_track_points(ofc, points, fw, bw, alpha1, alpha2, stats, bool(fused))


callable_module(__name__, __name__, "chain")
