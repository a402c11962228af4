"""Motion-compensated temporal filtering of a frame sequence on the GPU (temporal denoising, multi-frame fusion), over
fotg_temporal_filter / fotg_upsample_crop_temporal_filter of libfotg.so: the neighbours of a centre frame are pulled onto it along
their flows (the taps and codes of flowonthego_amd.warp) and averaged with it, each with a per-pixel weight that falls with the
photometric difference in a 3 x 3 window.  The definition, in f32 and in order, is in include/fotg.h and csrc/temporal.hip.h.  One
kernel reads each flow, the centre and the neighbour taps once and writes the filtered frame once; it runs in HIP only, there is
no CPU fallback.

The module is callable: flowonthego_amd.temporal(frames, ...) is flowonthego_amd.temporal.temporal_filter(frames, ...)."""
import ctypes as C

import torch

from ._args import _dev_f32, _ptr, _stream, cat_chunks, coarse_shape, image_stack, optional, two_channel
from ._lib import FotgError, callable_module, check, lib

STATS = ("sum_used", "unfiltered", "sum_abs_filtered", "sum_abs_center")
MAX_NEIGHBORS = 8


def _ints(a, name):
    """a host sequence / array / CPU tensor of ints as a list of lists or a list"""
    if isinstance(a, torch.Tensor):
        if a.is_cuda:
            raise FotgError("%s is a host array (it is validated on the host): pass a list, not a device tensor" % name)
        a = a.tolist()
    elif hasattr(a, "tolist"):
        a = a.tolist()
    return a


def _indices(center, neighbors):
    """-> (n, K, ctypes int array of n, ctypes int array of n K)"""
    center, neighbors = _ints(center, "center"), _ints(neighbors, "neighbors")
    try:
        cen = [int(v) for v in center]
        nbr = [[int(v) for v in row] for row in neighbors]
    except TypeError:
        raise FotgError("center must hold n ints and neighbors n rows of K ints")
    n = len(cen)
    K = len(nbr[0]) if nbr else 0
    if n < 1 or len(nbr) != n or any(len(r) != K for r in nbr) or not 1 <= K <= MAX_NEIGHBORS:
        raise FotgError("center must hold n >= 1 ints and neighbors n rows of 1 <= K <= %d ints" % MAX_NEIGHBORS)
    return n, K, (C.c_int * n)(*cen), (C.c_int * (n * K))(*[v for r in nbr for v in r])


def _frames(frames, device=None):
    """the stack checked: (T, h, w, channels, dtype)"""
    frames, ch = image_stack(frames, "frames", None, None, None, device, (torch.float32, torch.uint8))
    return int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2]), ch, frames.dtype


def _gains(gains, K):
    if gains is None:
        return None
    g = [float(v) for v in _ints(gains, "gains")]
    if len(g) != K:
        raise FotgError("gains must hold K = %d values" % K)
    return (C.c_float * K)(*g)


def _rest(frames, n, K, h, w, masks, ref, stats):
    """masks and ref checked, the outputs allocated: (dst, used, st)"""
    optional(masks, "masks", frames.device, (n, K, h, w), torch.uint8)
    shape = (n,) + tuple(frames.shape[1:])
    optional(ref, "ref", frames.device, shape, frames.dtype)
    dst = torch.empty(shape, dtype=frames.dtype, device=frames.device)
    used = torch.empty((n, h, w), dtype=torch.uint8, device=frames.device) if stats else None
    st = torch.empty((n, 4), dtype=torch.float64, device=frames.device) if stats else None
    return dst, used, st


def temporal_filter(frames, center, neighbors, flows, masks=None, tau=30.0, gains=None, ref=None, stats=False):
    """frames: device tensor (T, h, w) or (T, h, w, c), c in (1, 3), float32 or uint8.  center: n frame indices (a host list /
    array); neighbors: n rows of K frame indices, 1 <= K <= 8, -1 = absent.  flows: (n, K, h, w, 2) float32, flows[i, k] the flow
    from frame center[i] to frame neighbors[i][k].  masks: None or uint8 (n, K, h, w) in fb_check's alphabet (only pixels of code 0
    take part).  tau: the mean absolute difference over the 3 x 3 window and the channels at which a neighbour's weight reaches 0.
    gains: None or K weights >= 0, one per neighbour slot.  ref: None or the clean frames (n, h, w[, c]) of frames' type, for the
    residual sums.
    Returns dst (n, h, w[, c]) of frames' type; with stats=True (dst, used, stats): uint8 (n, h, w), the number of neighbours that
    took part in each pixel, and float64 (n, 4): the sum of used, the pixels with used == 0, sum |ref - dst| and sum |ref - centre|
    over all pixels and channels (STATS).  Asynchronous on the current stream."""
    T, h, w, ch, dtype = _frames(frames)
    n, K, cen, nbr = _indices(center, neighbors)
    _dev_f32(flows, "flows", frames.device, (n, K, h, w, 2))
    g = _gains(gains, K)
    dst, used, st = _rest(frames, n, K, h, w, masks, ref, stats)
    fn = lib().fotg_temporal_filter if dtype == torch.float32 else lib().fotg_temporal_filter_u8
    check(fn(frames.device.index or 0, n, K, T, _ptr(frames), w, h, ch, cen, nbr, _ptr(flows), _ptr(masks), C.c_float(tau), g,
             _ptr(ref), _ptr(dst), _ptr(used), _ptr(st), _stream(frames.device)))
    return (dst, used, st) if stats else dst


def upsample_crop_temporal_filter(ofc, coarse_flows, frames, center, neighbors, masks=None, tau=30.0, gains=None, ref=None,
                                  stats=False, fused=True):
    """The context's coarse flows (n K, h_l, w_l, 2) -- a batch calc of the pairs (frames[center[i]], frames[neighbors[i][k]]),
    image-major -- and frames (T, h_org, w_org[, c]) -> bit for bit temporal_filter(frames, center, neighbors,
    ofc.upsample_crop(coarse_flows).view(n, K, h, w, 2), ...), the statistics included.  fused=True evaluates the upsampling inside
    the filter and never writes a full-resolution flow; fused=False runs upsample_crop and the dense filter."""
    two_channel(ofc, "the temporal filter needs a two-channel flow")
    T, h, w, ch, dtype = _frames(frames, ofc.device)
    n, K, cen, nbr = _indices(center, neighbors)
    if n * K > ofc.max_batch:
        raise FotgError("%d images x %d neighbours, context created for max_batch = %d" % (n, K, ofc.max_batch))
    coarse_shape(ofc, coarse_flows, "coarse_flows", n * K)
    if (h, w) != (ofc.height_org, ofc.width_org):
        raise FotgError("frames are %d x %d, the context is %d x %d" % (w, h, ofc.width_org, ofc.height_org))
    if not fused:
        full = ofc.upsample_crop(coarse_flows).view(n, K, h, w, 2)
        return temporal_filter(frames, center, neighbors, full, masks=masks, tau=tau, gains=gains, ref=ref, stats=stats)
    g = _gains(gains, K)
    dst, used, st = _rest(frames, n, K, h, w, masks, ref, stats)
    fn = lib().fotg_upsample_crop_temporal_filter if dtype == torch.float32 else lib().fotg_upsample_crop_temporal_filter_u8
    check(fn(ofc._h, n, K, T, _ptr(coarse_flows), _ptr(frames), ch, cen, nbr, _ptr(masks), C.c_float(tau), g, _ptr(ref), _ptr(dst),
             _ptr(used), _ptr(st), _stream(ofc.device)))
    return (dst, used, st) if stats else dst


def neighbor_table(T, radius):
    """the (center, neighbors) of OFClass.temporal_filter: every frame a centre, its neighbours at distance -1, +1, -2, +2, ..,
    -radius, +radius, -1 beyond the ends of the sequence"""
    offs = [s * r for r in range(1, radius + 1) for s in (-1, 1)]
    return list(range(T)), [[c + o if 0 <= c + o < T else -1 for o in offs] for c in range(T)]


def ofc_temporal_filter(ofc, frames, radius=1, tau=30.0, gains=None, occlusion=False, ref=None, stats=False):
    """OFClass.temporal_filter: every frame of the stack (T, h, w[, c]) filtered with its neighbours at distance +-1 .. +-radius
    (K = 2 radius, neighbor_table's order).  The flows centre -> neighbour are computed directly (not chained), floor(max_batch / K)
    centres per batch, and the fused filter applied.  occlusion=True (a bidir context) also computes the flows neighbour -> centre
    and lets only the pixels the forward-backward check finds consistent take part.  ref: None or the clean stack, for the
    statistics.  Returns dst (T, ...) or (dst, used (T, h, w), stats (T, 4))."""
    two_channel(ofc, "the temporal filter needs a two-channel flow")
    T, h, w, ch, dtype = _frames(frames, ofc.device)
    if not isinstance(radius, int) or not 1 <= 2 * radius <= MAX_NEIGHBORS:
        raise FotgError("radius must be 1 .. %d" % (MAX_NEIGHBORS // 2))
    K = 2 * radius
    if occlusion and not ofc.op.bidir:
        raise FotgError("temporal_filter(occlusion=True) needs a context created with opt_params.bidir = True")
    per = ofc.max_batch // K
    if per < 1:
        raise FotgError("a radius of %d needs a context with max_batch >= %d" % (radius, K))
    optional(ref, "ref", ofc.device, frames.shape, dtype)
    u8 = dtype == torch.uint8
    center, neighbors = neighbor_table(T, radius)
    outs = []
    for s in range(0, T, per):
        cen, nbr = center[s:s + per], neighbors[s:s + per]
        n = len(cen)
        # an absent neighbour still has a slot in the flow batch: the centre itself (its flow is never read)
        i0 = torch.tensor([c for c in cen for _ in range(K)], device=ofc.device)
        i1 = torch.tensor([b if b >= 0 else c for c, row in zip(cen, nbr) for b in row], device=ofc.device)
        I0, I1 = frames.index_select(0, i0), frames.index_select(0, i1)
        masks = None
        if occlusion:
            fw, bw = ofc.bidirectional_flows(I0, I1)
            masks = ofc.upsample_crop_fb_check(fw, bw)[0].view(n, K, h, w)
        else:
            fw = ofc.calc_batch_u8(I0, I1) if u8 else ofc.calc_batch(I0, I1)
        outs.append(upsample_crop_temporal_filter(ofc, fw, frames, cen, nbr, masks=masks, tau=tau, gains=gains,
                                                  ref=None if ref is None else ref[s:s + n], stats=stats))
    return cat_chunks(outs)


callable_module(__name__, __name__, "temporal_filter")
