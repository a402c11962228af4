"""Motion blur along a flow on the GPU: a shutter simulated per frame, over fotg_motion_blur / fotg_upsample_crop_motion_blur of
libfotg.so.  The tile-max / neighbour-max scatter-as-gather reconstruction filter (McGuire et al. 2012, the direction test of Guertin
et al. 2014, both without depth): a static pixel is untouched unless something within reach moves across it, a moving object smears
over its surroundings by its own half-streak.  Integers after one f32 multiply (the same bytes every run); the definition, in order,
is in include/fotg.h and csrc/motionblur.hip.h.  It runs in HIP only; there is no CPU fallback."""
import torch

from ._args import _ptr, _stream, cat_chunks, coarse_flow, coarse_shape, dense_flow, image_stack, optional, two_channel, unbatch
from ._lib import FotgError, check, lib

STATS = ("code0", "code1", "code2", "code3", "taps", "copy_tiles", "max_len", "reserved")
TILE = 32
MAX_BLUR = 32
MAX_DIM = 16384
_TYPES = {torch.uint8: 0, torch.float32: 1}


def _args(shutter, max_blur):
    if not isinstance(shutter, (int, float)) or isinstance(shutter, bool) or not 0 < shutter <= 2 or int(round(256 * shutter)) < 1:
        raise FotgError("shutter must be in (0, 2] (and at least 1/512)")
    if not isinstance(max_blur, int) or isinstance(max_blur, bool) or max_blur < 1 or max_blur > MAX_BLUR:
        raise FotgError("max_blur must be an integer in 1 .. %d pixels" % MAX_BLUR)
    return int(round(256 * shutter))


def _outputs(src, n, h, w, code, vectors, stats):
    dev = src.device
    return (torch.empty_like(src),
            torch.empty((n, h, w), dtype=torch.uint8, device=dev) if code else None,
            torch.empty((n, h, w, 2), dtype=torch.int16, device=dev) if vectors else None,
            torch.empty((n, len(STATS)), dtype=torch.int64, device=dev) if stats else None)


def motion_blur(frame, flow, mask=None, shutter=0.5, max_blur=32, code=False, vectors=False, stats=False):
    """frame: device tensor (n, h, w) / (n, h, w, c) or a single image (h, w) / (h, w, c), c in (1, 3), uint8 or float32; flow:
    (n, h, w, 2) or (h, w, 2) float32, the flow of that frame.  mask: None or uint8 (n, h, w) / (h, w), a mask of fb_check (a pixel
    of non-zero code has no vector of its own).  shutter: the exposure as a fraction of the frame interval, in (0, 2] (0.5 = a 180
    degree shutter); max_blur: the longest half-streak, 1 .. 32 pixels.
    Returns dst (the frame's shape and dtype) and, as asked for and in this order, code uint8 (n, h, w) (0 untouched, 1 blurred, 2 a
    tap left the frame, 3 unknown vector), vectors int16 (n, h, w, 2) (the half-vectors in 1/16 pixel) and stats int64 (n, 8)
    (STATS).  A single image is told from a batch by the flow's dimensions.  Asynchronous on the current stream."""
    s256 = _args(shutter, max_blur)
    f, single, n, h, w = dense_flow(flow, max_dim=MAX_DIM)
    src, ch = image_stack(frame, "frame", n, h, w, f.device, tuple(_TYPES), single)
    m = optional(mask, "mask", f.device, (n, h, w), torch.uint8, single)
    outs = _outputs(src, n, h, w, code, vectors, stats)
    check(lib().fotg_motion_blur(f.device.index or 0, n, _ptr(src), _TYPES[src.dtype], ch, _ptr(f), w, h, _ptr(m), s256, max_blur,
                                 _ptr(outs[0]), _ptr(outs[1]), _ptr(outs[2]), _ptr(outs[3]), _stream(f.device)))
    return unbatch(outs, single)


def upsample_crop_motion_blur(ofc, coarse, frame, mask=None, shutter=0.5, max_blur=32, code=False, vectors=False, stats=False, fused=True):
    """The context's coarse flow (n, h_l, w_l, 2), frames (n, h_org, w_org[, c]) and mask (n, h_org, w_org) -> bit for bit
    motion_blur(frame, ofc.upsample_crop(coarse), ...).  fused=True evaluates the upsampling inside the first pass and never writes
    the full-resolution flow; fused=False runs upsample_crop and the dense form."""
    n = coarse_flow(ofc, coarse, "the motion blur needs a two-channel flow")
    if not fused:
        return motion_blur(frame, ofc.upsample_crop(coarse), mask, shutter, max_blur, code, vectors, stats)
    s256 = _args(shutter, max_blur)
    coarse_shape(ofc, coarse, "coarse", n)
    h, w = ofc.height_org, ofc.width_org
    src, ch = image_stack(frame, "frame", n, h, w, ofc.device, tuple(_TYPES))
    optional(mask, "mask", ofc.device, (n, h, w), torch.uint8)
    outs = _outputs(src, n, h, w, code, vectors, stats)
    check(lib().fotg_upsample_crop_motion_blur(ofc._h, n, _ptr(src), _TYPES[src.dtype], ch, _ptr(coarse), _ptr(mask), s256, max_blur,
                                               _ptr(outs[0]), _ptr(outs[1]), _ptr(outs[2]), _ptr(outs[3]), _stream(ofc.device)))
    return unbatch(outs, False)


def ofc_motion_blur(ofc, frames, shutter=0.5, max_blur=32, occlusion=False):
    """OFClass.motion_blur: frames (T+1, h, w[, c]) -> frames 0 .. T-1 blurred along their forward flows, (T, h, w[, c]) of the
    frames' dtype.  The flows of the sequence are computed in chunks of max_batch and never written at full resolution (the fused
    form); with occlusion (a context created with opt_params.bidir) the forward mask of the consistency check says which vectors
    are unknown."""
    two_channel(ofc, "the motion blur needs a two-channel flow")
    if occlusion and not ofc.op.bidir:
        raise FotgError("occlusion=True needs a context created with opt_params.bidir")
    _args(shutter, max_blur)
    if not isinstance(frames, torch.Tensor) or frames.dim() not in (3, 4) or frames.shape[0] < 2:
        raise FotgError("frames must be a (T+1, h, w) or (T+1, h, w, c) tensor of at least two frames")
    T, B, parts = frames.shape[0] - 1, ofc.max_batch, []
    for k in range(0, T, B):
        chunk = frames[k:min(k + B, T) + 1]
        mask = None
        if ofc.op.bidir:
            fw, bw = ofc.calc_sequence_bidirectional(chunk)
            if occlusion:
                mask = ofc.upsample_crop_fb_check(fw, bw)[0]
        else:
            fw = ofc.calc_sequence(chunk)
        parts.append(upsample_crop_motion_blur(ofc, fw, chunk[:-1].contiguous(), mask, shutter, max_blur))
    return cat_chunks(parts)
