"""Motion layers on the GPU: several parametric motions (translation, similarity or affine) fitted to one flow and every pixel given
to the nearest of them -- a camera pan, a vehicle crossing it, a second plane at another depth -- over fotg_motion_layers /
fotg_upsample_crop_motion_layers of libfotg.so.  Layer 0 is fit_motion's camera motion; each further layer grows from the 32 x 32
tile the earlier layers explain least; then all are refined together.  Exact 64-bit integer sums and a written-order f64 solve (no
floating-point atomics: the same bits every run); the definition, in order, is in include/fotg.h and csrc/layers.hip.h.  It runs
in HIP only; there is no CPU fallback.

What the outputs go into, unchanged:
    params, labels = motion_layers(flow, layers=3, labels=True)
    label_components(labels, fg=(1,))                            # the connected pieces of layer 1
    background_plate(frames, motions=..., exclude=(labels != 0).to(torch.uint8))   # a plate of the camera layer alone (layer 0)
    motion_histograms(flow, motion=params[:, 1].contiguous())    # HOF / MBH relative to layer 1's motion
    motion_flow(params[:, k].contiguous(), w, h)                 # layer k as a dense flow, for warp()"""
import ctypes as C

import torch

from ._args import _ptr, _stream, coarse_flow, coarse_shape, dense_flow, optional, unbatch
from ._lib import FotgError, check, lib
from .motion import MAX_DIM, _fit_args, _model

LAYER = ("labelled", "in_fit", "live", "fitted", "seed", "sum_X", "sum_Y", "sum_U")
LAYER_STATS = ("unassigned", "masked", "unknown", "live")
UNASSIGNED, MASKED, UNKNOWN = 253, 254, 255
MAX_LAYERS = 8


def _layer_args(layers, iters, rounds, thresh):
    if not isinstance(layers, int) or isinstance(layers, bool) or layers < 1 or layers > MAX_LAYERS:
        raise FotgError("layers must be an integer in 1 .. %d" % MAX_LAYERS)
    if not isinstance(rounds, int) or isinstance(rounds, bool) or rounds < 0 or rounds > 64:
        raise FotgError("rounds must be an integer in 0 .. 64")
    _fit_args(iters, thresh)


def _layer_outputs(n, K, h, w, device, labels, residual, records, stats, sums):
    return (torch.empty((n, K, 6), dtype=torch.float64, device=device),
            torch.empty((n, h, w), dtype=torch.uint8, device=device) if labels else None,
            torch.empty((n, h, w, 2), dtype=torch.float32, device=device) if residual else None,
            torch.empty((n, K, len(LAYER)), dtype=torch.int64, device=device) if records else None,
            torch.empty((n, len(LAYER_STATS)), dtype=torch.int64, device=device) if stats else None,
            torch.empty((n, K, 12), dtype=torch.int64, device=device) if sums else None)


def motion_layers(flow, mask=None, layers=3, model="affine", iters=3, rounds=3, thresh=1.0, init=None, labels=False, residual=False,
                  records=False, stats=False, sums=False):
    """flow: device tensor (n, h, w, 2) or (h, w, 2) float32; mask: None or uint8 (n, h, w) / (h, w) in the alphabet of fb_check
    (only its code-0 pixels take part).  layers: K in 1 .. 8 motions of one model (MODELS); iters: the re-fitting rounds of each
    layer's seeding, as in fit_motion; rounds: the refinement rounds in which every pixel joins its nearest layer within thresh
    (pixels) and every layer is fitted again; init: None or float64 (n, K, 6) / (K, 6), the layers to start from instead of seeding.
    Returns params, float64 (n, K, 6) or (K, 6), fit_motion's parameters per layer; params[:, 0] without init and with rounds=0 is
    fit_motion's result byte for byte (the refinement then moves it with the others).  A layer for which nothing was left is dead: zeros.  With any of labels / residual / records / stats /
    sums a tuple of params and those asked for, in this order: labels uint8 (n, h, w) (the layer of the pixel; UNASSIGNED 253:
    within thresh of no layer, MASKED 254, UNKNOWN 255: non-finite or beyond +-4096 px), residual float32 (n, h, w, 2) (the flow
    minus its layer's motion), records int64 (n, K, 8) (LAYER: pixels labelled, pixels in the last fit, live, fitted, the seed
    tile or -1 none / -2 init, the sums of X = 2x - (w-1), Y = 2y - (h-1) and rint(256 u) over the labelled pixels:
    layer_summary), stats int64 (n, 4) (LAYER_STATS), sums int64 (n, K, 12) (motion.SUMS of each layer's last fit).
    Asynchronous on the current stream of the flow's device."""
    flow, single, n, h, w = dense_flow(flow, max_dim=MAX_DIM)
    _layer_args(layers, iters, rounds, thresh)
    mask = optional(mask, "mask", flow.device, (n, h, w), torch.uint8, single)
    init = optional(init, "init", flow.device, (n, layers, 6), torch.float64, single)
    outs = _layer_outputs(n, layers, h, w, flow.device, labels, residual, records, stats, sums)
    check(lib().fotg_motion_layers(flow.device.index or 0, n, _ptr(flow), _ptr(mask), w, h, layers, _model(model), iters, rounds,
                                   C.c_float(thresh), _ptr(init), *(_ptr(o) for o in outs), _stream(flow.device)))
    return unbatch(outs, single)


def upsample_crop_motion_layers(ofc, coarse, mask=None, layers=3, model="affine", iters=3, rounds=3, thresh=1.0, init=None, labels=False,
                                residual=False, records=False, stats=False, sums=False, fused=False):
    """OFClass.upsample_crop_motion_layers: the context's coarse flow (n, h_l, w_l, 2) -> byte for byte
    motion_layers(ofc.upsample_crop(coarse), mask, ...); mask at the original size.  fused=True evaluates the upsampling inside
    every pass and never writes the full-resolution flow; fused=False (the default: a call makes many passes, and for fit_motion
    at iters = 3 the unfused form measured faster) runs upsample_crop and the dense form."""
    n = coarse_flow(ofc, coarse, "the motion layers need a two-channel flow")
    if not fused:
        return motion_layers(ofc.upsample_crop(coarse), mask, layers, model, iters, rounds, thresh, init, labels, residual, records, stats,
                             sums)
    coarse_shape(ofc, coarse, "coarse", n)
    h, w = ofc.height_org, ofc.width_org
    _layer_args(layers, iters, rounds, thresh)
    mask = optional(mask, "mask", ofc.device, (n, h, w), torch.uint8)
    init = optional(init, "init", ofc.device, (n, layers, 6), torch.float64)
    outs = _layer_outputs(n, layers, h, w, ofc.device, labels, residual, records, stats, sums)
    check(lib().fotg_upsample_crop_motion_layers(ofc._h, n, _ptr(coarse), _ptr(mask), layers, _model(model), iters, rounds,
                                                 C.c_float(thresh), _ptr(init), *(_ptr(o) for o in outs), _stream(ofc.device)))
    return unbatch(outs, False)


def ofc_motion_layers(ofc, frames, layers=3, model="affine", iters=3, rounds=3, thresh=1.0, labels=False, residual=False, records=False,
                      stats=False, sums=False, fused=False):
    """OFClass.motion_layers: the flows of frames (T+1, ...) first (motion._sequence_flows: on a bidir context the forward
    consistency mask keeps the occluded pixels out), then upsample_crop_motion_layers on them: params (T, K, 6) and what was asked for"""
    from .motion import _sequence_flows
    fw, mask = _sequence_flows(ofc, frames)
    return upsample_crop_motion_layers(ofc, fw, mask, layers, model, iters, rounds, thresh, None, labels, residual, records, stats, sums, fused)


def layer_summary(records, w, h):
    """records (..., 8) int64 of w x h images -> (..., 3) float64: the centroid of the layer's labelled pixels in pixels,
    ((sum_X / labelled) + (w-1)) / 2 and ((sum_Y / labelled) + (h-1)) / 2, and their mean horizontal motion sum_U / (256 labelled).
    (The layer's whole mean motion is its motion at the centroid: a00 cx + a01 cy + tx, a10 cx + a11 cy + ty.)  A layer without
    pixels yields NaN."""
    if not isinstance(records, torch.Tensor) or records.dim() < 1 or records.shape[-1] != len(LAYER):
        raise FotgError("records must be a (..., 8) tensor")
    r = records.to(torch.float64)
    cnt = r[..., 0]
    return torch.stack(((r[..., 5] / cnt + (w - 1.0)) / 2.0, (r[..., 6] / cnt + (h - 1.0)) / 2.0, r[..., 7] / (256.0 * cnt)), -1)
