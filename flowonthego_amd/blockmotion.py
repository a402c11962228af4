"""Block motion vectors from a dense flow on the GPU, for a video encoder, over fotg_block_motion /
fotg_upsample_crop_block_motion of libfotg.so: one quarter-pel vector per 8 x 8, 16 x 16 or 32 x 32 block of the frame, chosen among
the vectors the flow proposes for the block (zero, the block's mean, its centre pixel's, the means of its four quadrants) because it
makes the motion-compensated prediction from ref cheap, optionally refined by full-, half- and quarter-pel steps, with its SAD next
to it.  All arithmetic is integer; the definition is in include/fotg.h and csrc/blockmotion.hip.h.  It runs in HIP only; there is no
CPU fallback."""
import torch

from ._args import _dev_f32, _ptr, _stream, batched, cat_chunks, coarse_flow, coarse_shape, dense_flow, image_stack, optional, two_channel, unbatch
from ._lib import FotgError, check, lib

KINDS = ("zero", "mean", "centre", "top_left", "top_right", "bottom_left", "bottom_right")
MOVED = 8
STATS = ("sad", "sad_zero", "sse", "moved") + tuple("won_" + k for k in KINDS)
BLOCKS = (8, 16, 32)


def _check_params(block, refine):
    if block not in BLOCKS:
        raise FotgError("block must be 8, 16 or 32")
    if not isinstance(refine, int) or not 0 <= refine <= 3:
        raise FotgError("refine must be 0 .. 3")


def _frames(cur, ref, n, h, w, device, single):
    """the frames checked: (cur, ref as (n, h, w[, c]), channels); uint8, the arithmetic is integer"""
    cur, ch = image_stack(cur, "cur", n, h, w, device, (torch.uint8,), single)
    return cur, _dev_f32(batched(ref, single), "ref", device, cur.shape, torch.uint8), ch


def _outputs(n, h, w, block, cur, device, mask, pred, stats, single):
    mask = optional(mask, "mask", device, (n, h, w), torch.uint8, single)
    bw, bh = -(-w // block), -(-h // block)
    mv = torch.empty((n, bh, bw, 2), dtype=torch.int16, device=device)
    cost = torch.empty((n, bh, bw, 2), dtype=torch.int32, device=device)           # returned as uint32
    kind = torch.empty((n, bh, bw), dtype=torch.uint8, device=device)
    pr = torch.empty_like(cur) if pred else None
    st = torch.empty((n, len(STATS)), dtype=torch.int64, device=device) if stats else None
    return mask, mv, cost, kind, pr, st


def block_motion(cur, ref, flow, mask=None, block=16, refine=2, pred=False, stats=False):
    """cur, ref: device tensors (n, h, w[, c]) or (h, w[, c]) uint8, c in (1, 3).  flow: (n, h, w, 2) or (h, w, 2) float32, from cur
    to ref: cur(x) ~ ref(x + flow(x)).  mask: None or uint8 (n, h, w) / (h, w), a mask of fb_check (only pixels of code 0 propose
    vectors).  block: 8, 16 or 32.  refine: 0 .. 3, the last `refine` of the full-, half- and quarter-pel steps.
    Returns (mv, cost, kind): mv int16 (n, bh, bw, 2) in quarter pixels, cost uint32 (n, bh, bw, 2) = [SAD of mv, SAD of the zero
    vector], kind uint8 (n, bh, bw) = the winning candidate (KINDS) | 8 (MOVED) if a refinement step moved it; with pred=True also
    the prediction, uint8 shaped like cur; with stats=True also int64 (n, 11) (STATS).  A single image returns everything without
    the batch dimension.  Asynchronous on the current stream."""
    _check_params(block, refine)
    f, single, n, h, w = dense_flow(flow)
    c, r, ch = _frames(cur, ref, n, h, w, f.device, single)
    mask, mv, cost, kind, pr, st = _outputs(n, h, w, block, c, f.device, mask, pred, stats, single)
    check(lib().fotg_block_motion(f.device.index or 0, n, _ptr(c), _ptr(r), w, h, ch, _ptr(f), _ptr(mask), block, refine, _ptr(mv),
                                  _ptr(cost), _ptr(kind), _ptr(pr), _ptr(st), _stream(f.device)))
    return unbatch((mv, cost.view(torch.uint32), kind, pr, st), single)


def upsample_crop_block_motion(ofc, coarse, cur, ref, mask=None, block=16, refine=2, pred=False, stats=False, fused=True):
    """The context's coarse flow (n, h_l, w_l, 2) and the frames (n, h_org, w_org[, c]) -> bit for bit
    block_motion(cur, ref, ofc.upsample_crop(coarse), ...).  fused=True evaluates the upsampling inside the kernel and never writes
    the full-resolution flow; fused=False runs upsample_crop and the dense form."""
    n = coarse_flow(ofc, coarse, "block motion needs a two-channel flow")
    if not fused:
        return block_motion(cur, ref, ofc.upsample_crop(coarse), mask=mask, block=block, refine=refine, pred=pred, stats=stats)
    _check_params(block, refine)
    coarse_shape(ofc, coarse, "coarse", n)
    h, w = ofc.height_org, ofc.width_org
    c, r, ch = _frames(cur, ref, n, h, w, ofc.device, False)
    mask, mv, cost, kind, pr, st = _outputs(n, h, w, block, c, ofc.device, mask, pred, stats, False)
    check(lib().fotg_upsample_crop_block_motion(ofc._h, n, _ptr(coarse), _ptr(c), _ptr(r), ch, _ptr(mask), block, refine, _ptr(mv),
                                                _ptr(cost), _ptr(kind), _ptr(pr), _ptr(st), _stream(ofc.device)))
    return unbatch((mv, cost.view(torch.uint32), kind, pr, st), False)


def ofc_block_motion(ofc, I0, I1, block=16, refine=2, occlusion=False, pred=False, stats=False):
    """OFClass.block_motion: the flow of n 8-bit frame pairs I0 -> I1 (n, h, w[, c]) and the block vectors that predict I0 from I1,
    max_batch pairs per chunk, the full-resolution flow never written.  occlusion=True (a bidir context): both directions are
    computed and only the vectors upsample_crop_fb_check accepts propose candidates.  Returns (flow, mv, cost, kind[, pred][,
    stats]), flow the coarse flow as calc_batch_u8 returns it."""
    two_channel(ofc, "block motion needs a two-channel flow")
    if occlusion and not ofc.op.bidir:
        raise FotgError("block_motion(occlusion=True) needs a context created with opt_params.bidir = True")
    if not isinstance(I0, torch.Tensor) or not isinstance(I1, torch.Tensor) or I0.shape != I1.shape or I0.dim() < 3:
        raise FotgError("I0 and I1 must be tensors (n, h, w[, c]) of one shape")
    if I0.dtype != torch.uint8 or I1.dtype != torch.uint8:
        raise FotgError("I0 and I1 must be uint8 tensors (the arithmetic is integer)")
    _check_params(block, refine)
    parts = []
    for s in range(0, I0.shape[0], ofc.max_batch):
        a, b = I0[s:s + ofc.max_batch], I1[s:s + ofc.max_batch]
        m = None
        if occlusion:
            fw, bw = ofc.bidirectional_flows(a, b)
            m = ofc.upsample_crop_fb_check(fw, bw)[0]
        else:
            fw = ofc.calc_batch_u8(a, b)
        parts.append((fw,) + upsample_crop_block_motion(ofc, fw, a, b, mask=m, block=block, refine=refine, pred=pred, stats=stats))
    return cat_chunks(parts)
