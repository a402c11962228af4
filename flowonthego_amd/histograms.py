"""Motion histograms on the GPU: a flow turned into features, the histogram of optical flow (HOF) and the motion-boundary histograms
(MBHx, MBHy) of the dense-trajectories family, per cell of a regular grid and/or per object of an `ids` map, over
fotg_motion_histograms / fotg_upsample_crop_motion_histograms of libfotg.so.  The camera motion of fit_motion is subtracted first, the
mask of fb_check says which vectors not to trust, the ids of label_components / moving_objects say which object a pixel belongs to.
Exact integers after the first step (no floating-point atomics: the same bytes every run); the definition, in order, is in
include/fotg.h and csrc/histograms.hip.h.  It runs in HIP only; there is no CPU fallback."""
import torch

from ._args import _ptr, _stream, coarse_flow, coarse_shape, dense_flow, optional, two_channel, unbatch
from ._lib import FotgError, check, lib

# the columns of a record
HIST = tuple("hof%d" % k for k in range(8)) + ("zero",) + tuple("mbhx%d" % k for k in range(8)) + tuple("mbhy%d" % k for k in range(8)) + (
    "n", "n_mbh", "n_bad", "sum_m", "sum_u", "sum_v", "reserved")
HOF, ZERO, MBHX, MBHY = slice(0, 8), 8, slice(9, 17), slice(17, 25)
CELLS = (8, 16, 32)
MAX_ROWS = 1024
MAX_DIM = 16384


def _args(cell, thresh, rows, cells, ids):
    if cell not in CELLS or isinstance(cell, bool):
        raise FotgError("cell must be 8, 16 or 32")
    if not isinstance(thresh, (int, float)) or isinstance(thresh, bool) or not 0 <= thresh <= 8192:
        raise FotgError("thresh must be in 0 .. 8192 pixels")
    if not isinstance(rows, int) or isinstance(rows, bool) or rows < 1 or rows > MAX_ROWS:
        raise FotgError("rows must be an integer in 1 .. %d" % MAX_ROWS)
    if not cells and ids is None:
        raise FotgError("nothing to compute: cells=False and no ids")
    return int(round(thresh * 256))


def _outputs(n, h, w, cell, rows, cells, ids, device):
    return (torch.empty((n, (h + cell - 1) // cell, (w + cell - 1) // cell, len(HIST)), dtype=torch.int64, device=device) if cells else None,
            torch.empty((n, rows, len(HIST)), dtype=torch.int64, device=device) if ids is not None else None)


def motion_histograms(flow, mask=None, motion=None, cell=16, thresh=0.4, ids=None, rows=256, cells=True):
    """flow: device tensor (n, h, w, 2) or (h, w, 2) float32.  mask: None or uint8 (n, h, w) / (h, w), a mask of fb_check (only pixels
    of code 0 take part).  motion: None or float64 (n, 6) / (6,), the parameters fit_motion returns: the camera motion subtracted from
    every vector first.  cell: 8, 16 or 32 pixels.  thresh: the magnitude, in pixels, below which a vector counts in the zero bin
    instead of an orientation bin (round(256 thresh) in the fixed point of the definition).  ids: None or int32 (n, h, w) / (h, w), the
    `ids` of label_components; rows: the rows of the object output, 1 .. 1024.
    Returns the cells, int64 (n, ceil(h / cell), ceil(w / cell), 32) (cells=True), and/or with ids the objects, int64 (n, rows, 32);
    both as a tuple when both.  The 32 columns (HIST): eight HOF bins, the zero-bin pixel count, eight MBHx and eight MBHy bins, then
    the admissible pixels, the pixels in MBH, the inadmissible pixels, the sums of the magnitude, of U and of V in 1/256 pixel, and a
    zero.  A single flow returns them without the batch dimension.  Asynchronous on the current stream."""
    t256 = _args(cell, thresh, rows, cells, ids)
    f, single, n, h, w = dense_flow(flow, max_dim=MAX_DIM)
    m = optional(mask, "mask", f.device, (n, h, w), torch.uint8, single)
    p = optional(motion, "motion", f.device, (n, 6), torch.float64, single)
    i = optional(ids, "ids", f.device, (n, h, w), torch.int32, single)
    outs = _outputs(n, h, w, cell, rows, cells, i, f.device)
    check(lib().fotg_motion_histograms(f.device.index or 0, n, _ptr(f), w, h, _ptr(m), _ptr(p), cell, t256, _ptr(outs[0]), _ptr(i), rows,
                                       _ptr(outs[1]), _stream(f.device)))
    return unbatch(outs, single)


def upsample_crop_motion_histograms(ofc, coarse, mask=None, motion=None, cell=16, thresh=0.4, ids=None, rows=256, cells=True, fused=True):
    """The context's coarse flow (n, h_l, w_l, 2), mask and ids of (n, h_org, w_org) -> bit for bit
    motion_histograms(ofc.upsample_crop(coarse), ...).  fused=True evaluates the upsampling inside the kernel and never writes the
    full-resolution flow; fused=False runs upsample_crop and the dense form."""
    n = coarse_flow(ofc, coarse, "motion histograms need a two-channel flow")
    if not fused:
        return motion_histograms(ofc.upsample_crop(coarse), mask, motion, cell, thresh, ids, rows, cells)
    t256 = _args(cell, thresh, rows, cells, ids)
    coarse_shape(ofc, coarse, "coarse", n)
    h, w = ofc.height_org, ofc.width_org
    optional(mask, "mask", ofc.device, (n, h, w), torch.uint8)
    optional(motion, "motion", ofc.device, (n, 6), torch.float64)
    optional(ids, "ids", ofc.device, (n, h, w), torch.int32)
    outs = _outputs(n, h, w, cell, rows, cells, ids, ofc.device)
    check(lib().fotg_upsample_crop_motion_histograms(ofc._h, n, _ptr(coarse), _ptr(mask), _ptr(motion), cell, t256, _ptr(outs[0]), _ptr(ids),
                                                     rows, _ptr(outs[1]), _stream(ofc.device)))
    return unbatch(outs, False)


def motion_descriptors(hist):
    """hist: int64 (..., 32), records of motion_histograms -> float32 (..., 25): HOF with its ninth bin, the zero-bin pixel count
    scaled by 256 (so that a pixel weighs as a vector of one pixel does), then MBHx, then MBHy; each of the three parts divided by its
    sum (L1) and square-rooted.  A part that is all zero stays zero.  Plain torch on the tensor's device, not a kernel."""
    if not isinstance(hist, torch.Tensor) or hist.dim() < 1 or hist.shape[-1] != len(HIST):
        raise FotgError("hist must be a (..., 32) tensor")
    h = hist.to(torch.float64)
    parts = (torch.cat((h[..., HOF], h[..., ZERO:ZERO + 1] * 256.0), -1), h[..., MBHX], h[..., MBHY])
    out = []
    for p in parts:
        s = p.sum(-1, keepdim=True)
        out.append(torch.sqrt(p / torch.where(s > 0, s, torch.ones_like(s))))
    return torch.cat(out, -1).to(torch.float32)


def ofc_motion_histograms(ofc, frames, cell=16, model="affine", occlusion=False, objects=False, thresh=0.4, iters=3, fit_thresh=1.0,
                          min_area=64, max_objects=256, connectivity=8, cells=True):
    """OFClass.motion_histograms: the flows of frames (T+1, ...); the camera fit of each (model; None skips it and nothing is
    subtracted); with occlusion (a bidir context) the forward consistency mask, which then is the fit's and the histograms' mask;
    with objects the ids of moving_objects (needs a model); then the fused histograms along the coarse flows.
    Returns (params (T, 6) or None, cells (T, ceil(h / cell), ceil(w / cell), 32)) and with objects also (object histograms (T,
    max_objects, 32), the object table (T, max_objects, 11), ids (T, h, w)); cells=False leaves the cells out."""
    from .motion import upsample_crop_fit_motion
    from .objects import label_components
    two_channel(ofc, "motion histograms need a two-channel flow")
    if objects and model is None:
        raise FotgError("objects=True needs a motion model: the objects are the pixels that do not follow it")
    if occlusion and not ofc.op.bidir:
        raise FotgError("occlusion=True needs a context created with opt_params.bidir")
    if not cells and not objects:
        raise FotgError("nothing to compute: cells=False and objects=False")
    mask = None
    if ofc.op.bidir:
        fw, bw = ofc.calc_sequence_bidirectional(frames)
        if occlusion:
            mask = ofc.upsample_crop_fb_check(fw, bw)[0]
    else:
        fw = ofc.calc_sequence(frames)
    params = table = ids = None
    if objects:
        params, code, residual = upsample_crop_fit_motion(ofc, fw, mask, model, iters, fit_thresh, code=True, residual=True)
        table, ids = label_components(code, (1,), connectivity, residual, min_area, max_objects, ids=True)
    elif model is not None:
        params = upsample_crop_fit_motion(ofc, fw, mask, model, iters, fit_thresh)
    out = upsample_crop_motion_histograms(ofc, fw, mask, params, cell, thresh, ids, max_objects, cells)
    out = out if isinstance(out, tuple) else (out,)
    return (params,) + out + ((table, ids) if objects else ())
