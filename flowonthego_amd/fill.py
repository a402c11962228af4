"""Hole filling on the GPU by pull-push: the unknown pixels of frames and flows filled from the known ones, at any hole size -- over
fotg_fill / fotg_fill_u8 of libfotg.so.  The definition, in exact integers and f32 and in order, is in include/fotg.h and
csrc/fill.hip.h: a pyramid of sums over the known pixels (pull) is interpolated back down into the holes (push).  Three launches per
call; it runs in HIP only, there is no CPU fallback.  It closes the removal chain (remove_objects leaves holes where the plate knows
nothing) and makes a dense field of a flow with rejected, unknown or missing vectors, which warp, chain, block_motion and
motion_histograms want.
Not built: filling in place, an edge-aware or guided push, weights other than 0 / 1, inpainting from other frames, more than 3
channels."""
import ctypes as C

import torch

from ._args import _ptr, _stream, cat_chunks, dense_flow, optional, two_channel, unbatch
from ._lib import FotgError, check, lib

CODES = FILL_CODES = ("known", "filled", "unfilled")
STATS = FILL_STATS = ("known", "filled", "unfilled", "depth")
MAX_DIM = 16384


def _fg_codes(fg):
    """None: every non-zero byte (0); otherwise label_components' 8-bit set of the codes 0 .. 7"""
    if fg is None:
        return 0
    from .objects import _fg_set
    return _fg_set(fg)


def scratch_bytes(n, w, h, ch):
    """the stream-ordered memory a call on n images of w x h pixels and ch channels takes (fotg_fill_scratch; host only)"""
    b = C.c_longlong(0)
    check(lib().fotg_fill_scratch(n, w, h, ch, C.byref(b)))
    return int(b.value)


def fill_holes(src, hole=None, fg=None, dst=True, code=False, stats=False):
    """src: device float32 or uint8, (n, h, w[, c]) or (h, w[, c]) with c in 1 .. 3 (uint8: 1 or 3); hole: device uint8 (n, h, w) /
    (h, w) or None (float32 only) -- a 2-D hole makes the call single; without a hole a 3-D src is (h, w, c).  fg: None -- every
    non-zero byte of hole is a hole -- or the byte values 0 .. 7 that are holes, as for label_components, so that a code map goes in
    unconverted.  A float32 pixel with a channel that is not finite or beyond +-32768 (the .flo marker 1e9) is a hole as well.
    Returns those asked for, in this order (one alone as itself): dst, src with its holes filled, known pixels bit for bit; code
    uint8 (n, h, w) (CODES: 0 known, 1 filled, 2 nothing known in this image -- kept); stats int64 (n, 4) (STATS: the known, filled
    and unfilled pixels and depth, the log2 scale of the widest hole).  Asynchronous on the current stream."""
    fgc = _fg_codes(fg)
    if not (dst or code or stats):
        raise FotgError("ask for at least one of dst, code and stats")
    if not isinstance(src, torch.Tensor) or not src.is_cuda or src.dtype not in (torch.float32, torch.uint8) or src.dim() not in (2, 3, 4):
        raise FotgError("src must be a device float32 or uint8 tensor (n, h, w[, c]) or (h, w[, c])")
    if hole is not None:
        if not isinstance(hole, torch.Tensor) or hole.dtype != torch.uint8 or hole.dim() not in (2, 3):
            raise FotgError("hole must be a device uint8 tensor (n, h, w) or (h, w)")
        single = hole.dim() == 2
        chan = src.dim() == hole.dim() + 1
        if not chan and src.dim() != hole.dim():
            raise FotgError("src %s does not go with hole %s" % (tuple(src.shape), tuple(hole.shape)))
    else:
        if src.dtype != torch.float32:
            raise FotgError("a uint8 src needs a hole map")
        if src.dim() != 3 and src.dim() != 4:
            raise FotgError("without a hole map src must be (h, w, c) or (n, h, w, c)")
        single, chan = src.dim() == 3, True
    s = src if chan else src.unsqueeze(-1)
    s = (s.unsqueeze(0) if single else s).contiguous()
    n, h, w, ch = (int(v) for v in s.shape)
    if not (1 <= h <= MAX_DIM and 1 <= w <= MAX_DIM and 1 <= n <= 65535):
        raise FotgError("src must have between 1 and %d rows and columns and at most 65535 images" % MAX_DIM)
    if ch not in ((1, 2, 3) if s.dtype == torch.float32 else (1, 3)):
        raise FotgError("src must have 1, 2 or 3 channels (uint8: 1 or 3), not %d" % ch)
    dev = s.device
    ho = optional(hole.contiguous() if isinstance(hole, torch.Tensor) else hole, "hole", dev, (n, h, w), torch.uint8, single=single)
    outs = (torch.empty_like(s) if dst else None,
            torch.empty((n, h, w), dtype=torch.uint8, device=dev) if code else None,
            torch.empty((n, len(STATS)), dtype=torch.int64, device=dev) if stats else None)
    fn = lib().fotg_fill if s.dtype == torch.float32 else lib().fotg_fill_u8
    check(fn(dev.index or 0, n, _ptr(s), w, h, ch, _ptr(ho), fgc, _ptr(outs[0]), _ptr(outs[1]), _ptr(outs[2]), _stream(dev)))
    if outs[0] is not None and not chan:
        outs = (outs[0].squeeze(-1),) + outs[1:]
    return unbatch(outs, single)


def fill_flow(flow, mask=None):
    """flow: device float32 (n, h, w, 2) / (h, w, 2); mask: None or the uint8 map of fb_check (n, h, w) / (h, w), non-zero = this
    vector is rejected.  Returns the dense flow: fill_holes(flow, mask) -- a vector is a hole where its mask byte is non-zero or a
    component is not finite or beyond +-32768 (a .flo file's unknown vectors)."""
    flow, single, n, h, w = dense_flow(flow, "flow", MAX_DIM)
    mask = optional(mask, "mask", flow.device, (n, h, w), torch.uint8, single=single)
    out = fill_holes(flow, mask)
    return out[0] if single else out


def removed_holes(code, alpha):
    """the pixels remove_objects counts as `holes`: code 2 or 3 (no plate there, unknown) and alpha == 256 -> uint8 0 / 1"""
    if not isinstance(code, torch.Tensor) or not isinstance(alpha, torch.Tensor) or code.shape != alpha.shape:
        raise FotgError("code and alpha must be remove_objects' maps of one shape")
    return (((code == 2) | (code == 3)) & (alpha == 256)).to(torch.uint8)


def fill_removed(clean, code, alpha, fill_code=False):
    """clean, code, alpha: remove_objects' outputs.  fill_holes(clean, hole) with hole = (code is 2 or 3) and alpha == 256: exactly
    the pixels remove_objects counts as holes are filled from the frame around them.  fill_code=True: (filled, fill_holes' code)."""
    return fill_holes(clean, removed_holes(code, alpha), code=fill_code)


def upsample_crop_fill_flow(ofc, coarse, mask=None):
    """fill_flow(ofc.upsample_crop(coarse), mask).  The plain composition: the result is a full-resolution flow by definition, so
    a fused kernel would save one read of it, not a buffer."""
    two_channel(ofc, "the flow filling needs a two-channel flow")
    return fill_flow(ofc.upsample_crop(coarse), mask)


def ofc_calc_filled(ofc, I0, I1, both=False, code=False, stats=False):
    """OFClass.calc_filled: the flow of n frame pairs I0 -> I1 (n, h, w[, c]) float32 or uint8 at full resolution, the vectors the
    forward-backward check rejects filled from the consistent ones, max_batch pairs per chunk.  The composition, call for call:
    ofc.bidirectional_flows -> ofc.upsample_crop_fb_check (the masks) -> fill_holes(ofc.upsample_crop(fw), mask_fw, code=, stats=).
    both=True also returns the backward flow filled under mask_bw: a pair (forward, backward).  Needs a bidir context."""
    two_channel(ofc, "the flow filling needs a two-channel flow")
    if not ofc.op.bidir:
        raise FotgError("calc_filled needs a context created with opt_params.bidir = True")
    if not isinstance(I0, torch.Tensor) or not isinstance(I1, torch.Tensor) or I0.shape != I1.shape or I0.dim() < 3:
        raise FotgError("I0 and I1 must be tensors (n, h, w[, c]) of one shape")
    parts = []
    for s in range(0, I0.shape[0], ofc.max_batch):
        fw, bw = ofc.bidirectional_flows(I0[s:s + ofc.max_batch], I1[s:s + ofc.max_batch])
        m, mb = ofc.upsample_crop_fb_check(fw, bw)
        r = fill_holes(ofc.upsample_crop(fw), m, code=code, stats=stats)
        parts.append((r, fill_holes(ofc.upsample_crop(bw), mb, code=code, stats=stats)) if both else r)
    return cat_chunks(parts)


def ofc_remove_objects_filled(ofc, frames, **kw):
    """OFClass.remove_objects_filled: frames (T+1, h, w[, c]) -> (clean, code, mask, plate, fill_code); the keywords are
    OFClass.remove_objects' (and erase.ofc_remove_objects' mask, open, close).  The composition, call for call:
    erase.ofc_remove_objects(ofc, frames, **kw) for the removal, its code, the mask and the plate; then the holes of that removal --
    code 2 or 3 under the grown mask, which is where remove_objects(..., code=True, alpha=True) has alpha == 256:
    grow_mask(mask, grow) is that map without a second removal --; then fill_holes(clean, holes, code=True).  clean: the frames
    without the confirmed objects and without the holes the plate left; code: remove_objects' code map as it was; fill_code:
    fill_holes' code (1 = this pixel was inpainted)."""
    from .erase import grow_mask, ofc_remove_objects
    clean, code, mask, plate = ofc_remove_objects(ofc, frames, **kw)
    holes = (((code == 2) | (code == 3)) & (grow_mask(mask, kw.get("grow", 2)) != 0)).to(torch.uint8)
    filled, fill_code = fill_holes(clean, holes, code=True)
    return filled, code, mask, plate, fill_code
