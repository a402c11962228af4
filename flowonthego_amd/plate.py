"""Background plates and mosaics on the GPU: the frames of a shot pulled into one coordinate system along their motion and reduced
per pixel by a median (or a mean) over the frames that see the pixel -- the scene without its moving objects, and on a canvas larger
than the frame the panorama of a panning shot -- over fotg_plate / fotg_plate_motion / fotg_upsample_crop_plate of libfotg.so.  The
definition, in f32 and in order, is in include/fotg.h and csrc/plate.hip.h.  One kernel gathers the K samples of a canvas pixel,
selects the median on chip and writes the pixel once; it runs in HIP only, there is no CPU fallback.

The module is callable: flowonthego_amd.plate(frames, ...) is flowonthego_amd.plate.background_plate(frames, ...)."""
import ctypes as C
import math

import torch

from ._args import _dev_f32, _ptr, _stream, coarse_shape, image_stack, optional, two_channel
from ._lib import FotgError, callable_module, check, lib
from .temporal import _ints

MODES = ("median", "mean")
CODES = ("estimated", "hidden", "uncovered")
STATS = CODES + ("sum_count", "sum_abs_plate", "sum_abs_first")
MAX_FRAMES = 32
MAX_DIM = 16384


def _mode(mode):
    if mode in MODES:
        return MODES.index(mode)
    raise FotgError("mode must be one of %s" % (MODES,))


def _index(index, T):
    """-> (n, K, ctypes int array of n K); None: one plate of all T frames"""
    if index is None:
        index = [list(range(T))]
    index = _ints(index, "index")
    try:
        if index and not hasattr(index[0], "__len__"):
            index = [index]
        rows = [[int(v) for v in row] for row in index]
    except TypeError:
        raise FotgError("index must hold n rows of K frame indices")
    n = len(rows)
    K = len(rows[0]) if rows else 0
    if n < 1 or n > 65535 or any(len(r) != K for r in rows) or not 1 <= K <= MAX_FRAMES:
        raise FotgError("index must hold 1 <= n <= 65535 rows of 1 <= K <= %d frame indices" % MAX_FRAMES)
    if any(v < -1 or v >= T for r in rows for v in r):
        raise FotgError("a frame index must lie in -1 .. %d (-1 = absent)" % (T - 1))
    return n, K, (C.c_int * (n * K))(*[v for r in rows for v in r])


def _frames(frames, device=None):
    """the stack checked: (T, h, w, channels, dtype)"""
    frames, ch = image_stack(frames, "frames", None, None, None, device, (torch.float32, torch.uint8))
    return int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2]), ch, frames.dtype


def _rest(frames, n, K, T, h, w, W, H, occ, exclude, min_count, ref, count, code, stats):
    """occ, exclude, min_count and ref checked, the outputs allocated: (dst, count, code, stats)"""
    if not isinstance(min_count, int) or isinstance(min_count, bool) or not 1 <= min_count <= K:
        raise FotgError("min_count must be an integer in 1 .. K = %d" % K)
    optional(occ, "occ", frames.device, (n, K, H, W), torch.uint8)
    optional(exclude, "exclude", frames.device, (T, h, w), torch.uint8)
    shape = (n, H, W) + tuple(frames.shape[3:])
    optional(ref, "ref", frames.device, shape, frames.dtype)
    dev = frames.device
    return (torch.empty(shape, dtype=frames.dtype, device=dev),
            torch.empty((n, H, W), dtype=torch.uint8, device=dev) if count else None,
            torch.empty((n, H, W), dtype=torch.uint8, device=dev) if code else None,
            torch.empty((n, 6), dtype=torch.float64, device=dev) if stats else None)


def _result(outs):
    outs = tuple(o for o in outs if o is not None)
    return outs[0] if len(outs) == 1 else outs


def background_plate(frames, index=None, flows=None, motions=None, canvas=None, origin=(0, 0), occ=None, exclude=None, mode="median",
                     min_count=1, fill=0, ref=None, count=False, code=False, stats=False):
    """frames: device tensor (T, h, w) or (T, h, w, c), c in (1, 3), float32 or uint8.  index: n rows of K frame indices (a host
    list / array; one row alone is one plate), 1 <= K <= 32, -1 = absent; None: one plate of all T frames.  Exactly one source of the
    samples' vectors: flows (n, K, H, W, 2) float32 on the canvas, flows[i, k] from the reference to frame index[i][k]; or motions
    (n, K, 6) / (K, 6) float64, the maps reference -> frame in fit_motion's convention (plate_motions).  canvas: (W, H), by default
    the flows' size or the frame grid; origin: (ox, oy), canvas pixel (X, Y) is the reference coordinate (X - ox, Y - oy)
    (mosaic_canvas).  occ: None or uint8 (n, K, H, W), non-zero = the sample is hidden at that canvas pixel; exclude: None or uint8
    (T, h, w), non-zero = that pixel of that frame takes no part (the moving objects).  mode: "median" or "mean"; a pixel with fewer
    than min_count admitted samples gets fill.  ref: None or the clean canvas (n, H, W[, c]) of frames' type, for the residual sums.
    Returns dst (n, H, W[, c]) of frames' type; with any of count / code / stats a tuple of dst and those asked for, in this order:
    count uint8 (n, H, W), the samples admitted; code uint8 (n, H, W) (CODES: 0 estimated, 1 covered but hidden by the masks,
    2 covered by fewer than min_count frames); stats float64 (n, 6) (STATS).  Asynchronous on the current stream."""
    T, h, w, ch, dtype = _frames(frames)
    n, K, ix = _index(index, T)
    if (flows is None) == (motions is None):
        raise FotgError("give the samples' vectors either as flows or as motions")
    try:
        ox, oy = (int(v) for v in origin)
    except (TypeError, ValueError):
        raise FotgError("origin must be (ox, oy)")
    if flows is not None:
        if not isinstance(flows, torch.Tensor) or flows.dim() != 5:
            raise FotgError("flows must be a (n, K, H, W, 2) tensor")
        W, H = int(flows.shape[3]), int(flows.shape[2])
    else:
        W, H = w, h
    if canvas is not None:
        try:
            cw, chh = (int(v) for v in canvas)
        except (TypeError, ValueError):
            raise FotgError("canvas must be (W, H)")
        if flows is not None and (cw, chh) != (W, H):
            raise FotgError("the canvas is %d x %d, the flows are %d x %d" % (cw, chh, W, H))
        W, H = cw, chh
    if not (1 <= W <= MAX_DIM and 1 <= H <= MAX_DIM and 1 <= w <= MAX_DIM and 1 <= h <= MAX_DIM):
        raise FotgError("frames and canvas must have between 1 and %d rows and columns" % MAX_DIM)
    if flows is not None:
        src = _dev_f32(flows, "flows", frames.device, (n, K, H, W, 2))
        fn = lib().fotg_plate if dtype == torch.float32 else lib().fotg_plate_u8
    else:
        if isinstance(motions, torch.Tensor) and motions.dim() == 2:
            motions = motions.unsqueeze(0)
        src = _dev_f32(motions, "motions", frames.device, (n, K, 6), torch.float64)
        fn = lib().fotg_plate_motion if dtype == torch.float32 else lib().fotg_plate_motion_u8
    outs = _rest(frames, n, K, T, h, w, W, H, occ, exclude, min_count, ref, count, code, stats)
    check(fn(frames.device.index or 0, n, K, T, _ptr(frames), w, h, ch, ix, _ptr(src), W, H, ox, oy, _ptr(occ), _ptr(exclude), _mode(mode),
             min_count, C.c_float(fill), _ptr(ref), *(_ptr(o) for o in outs), _stream(frames.device)))
    return _result(outs)


def upsample_crop_background_plate(ofc, coarse_flows, frames, index=None, occ=None, exclude=None, mode="median", min_count=1, fill=0,
                                   ref=None, count=False, code=False, stats=False, fused=True):
    """The context's coarse flows (n K, h_l, w_l, 2) -- a batch calc of the pairs (reference of plate i, frames[index[i][k]]),
    plate-major -- and frames (T, h_org, w_org[, c]) -> bit for bit background_plate(frames, index,
    flows=ofc.upsample_crop(coarse_flows).view(n, K, h, w, 2), ...) on the frame grid, the statistics included.  fused=True evaluates
    the upsampling inside the kernel and never writes a full-resolution flow; fused=False runs upsample_crop and the dense form."""
    two_channel(ofc, "the background plate needs a two-channel flow")
    T, h, w, ch, dtype = _frames(frames, ofc.device)
    n, K, ix = _index(index, T)
    if n * K > ofc.max_batch:
        raise FotgError("%d plates x %d frames, context created for max_batch = %d" % (n, K, ofc.max_batch))
    coarse_shape(ofc, coarse_flows, "coarse_flows", n * K)
    if (h, w) != (ofc.height_org, ofc.width_org):
        raise FotgError("frames are %d x %d, the context is %d x %d" % (w, h, ofc.width_org, ofc.height_org))
    if not fused:
        full = ofc.upsample_crop(coarse_flows).view(n, K, h, w, 2)
        return background_plate(frames, index, flows=full, occ=occ, exclude=exclude, mode=mode, min_count=min_count, fill=fill, ref=ref,
                                count=count, code=code, stats=stats)
    outs = _rest(frames, n, K, T, h, w, w, h, occ, exclude, min_count, ref, count, code, stats)
    fn = lib().fotg_upsample_crop_plate if dtype == torch.float32 else lib().fotg_upsample_crop_plate_u8
    check(fn(ofc._h, n, K, T, _ptr(coarse_flows), _ptr(frames), ch, ix, _ptr(occ), _ptr(exclude), _mode(mode), min_count, C.c_float(fill),
             _ptr(ref), *(_ptr(o) for o in outs), _stream(ofc.device)))
    return _result(outs)


def plate_motions(params, ref=0):
    """params (T, 6) float64, the motions frame k -> k+1 (camera_motion) -> (T+1, 6): per frame k the parameters of
    C_k . C_ref^-1 - I, the map from the reference frame's coordinates to frame k's, where M_k = [I + A_k | t_k], C_0 = I and
    C_k = M_{k-1} . C_{k-1} (the path of smoothing_motions; motion._compose and motion._inverse in their written order)"""
    from .motion import _compose, _inverse
    if not isinstance(params, torch.Tensor) or params.dim() != 2 or params.shape[1] != 6 or params.shape[0] < 1 or params.dtype != torch.float64:
        raise FotgError("params must be a (T, 6) float64 tensor")
    T = int(params.shape[0])
    if not isinstance(ref, int) or isinstance(ref, bool) or not 0 <= ref <= T:
        raise FotgError("ref must be a frame index in 0 .. %d" % T)
    one = torch.ones((), dtype=torch.float64, device=params.device)
    zero = torch.zeros((), dtype=torch.float64, device=params.device)
    path = [(one, zero, zero, zero, one, zero)]
    for k in range(T):
        p = params[k]
        path.append(_compose((p[0] + 1.0, p[1], p[2], p[3], p[4] + 1.0, p[5]), path[-1]))
    Cs = torch.stack([torch.stack(c) for c in path])                       # (T+1, 6)
    W = _compose(tuple(Cs[:, i] for i in range(6)), _inverse(tuple(Cs[ref, i] for i in range(6))))
    return torch.stack((W[0] - 1.0, W[1], W[2], W[3], W[4] - 1.0, W[5]), dim=1).contiguous()


def mosaic_canvas(motions, w, h):
    """motions (K, 6) float64 (plate_motions), the maps reference -> frame of w x h frames -> (W, H, ox, oy): the integer bounding
    box of every frame's four corners in reference coordinates.  A corner c of frame k lies at x = (I + A_k)^-1 (c - t_k); the box is
    floor(min) .. ceil(max) over all of them, W = xmax - xmin + 1, ox = -xmin, rows alike.  Computed on the host in float64; a box
    beyond 16384 pixels, or a motion that cannot be inverted, is a FotgError."""
    if hasattr(motions, "detach"):
        motions = motions.detach().cpu().tolist()
    rows = [[float(v) for v in r] for r in _ints(motions, "motions")]
    if w < 1 or h < 1 or not rows or any(len(r) != 6 for r in rows):
        raise FotgError("motions must be (K, 6) and w, h >= 1")
    xs, ys = [], []
    for a00, a01, tx, a10, a11, ty in rows:
        m00, m11 = a00 + 1.0, a11 + 1.0
        det = m00 * m11 - a01 * a10
        if not (math.isfinite(det) and det != 0.0):
            raise FotgError("a motion cannot be inverted")
        for cx in (0.0, float(w - 1)):
            for cy in (0.0, float(h - 1)):
                dx, dy = cx - tx, cy - ty
                xs.append((m11 * dx - a01 * dy) / det)
                ys.append((m00 * dy - a10 * dx) / det)
    if not all(math.isfinite(v) for v in xs + ys):
        raise FotgError("a frame's corner is not finite in reference coordinates")
    x0, x1, y0, y1 = math.floor(min(xs)), math.ceil(max(xs)), math.floor(min(ys)), math.ceil(max(ys))
    W, H = x1 - x0 + 1, y1 - y0 + 1
    if W > MAX_DIM or H > MAX_DIM:
        raise FotgError("the mosaic would be %d x %d, the largest canvas is %d x %d" % (W, H, MAX_DIM, MAX_DIM))
    return W, H, -x0, -y0


def _ofc_plate(ofc, frames, ref, model, mosaic, mode, exclude_moving, min_count):
    """ofc_background's work: (plate, code, count, motions), motions (T+1, 6) the maps reference -> frame the plate was made with
    (flowonthego_amd.subtract.ofc_foreground inverts them)"""
    from .motion import _sequence_flows, upsample_crop_fit_motion
    two_channel(ofc, "the background plate needs a two-channel flow")
    T1, h, w, ch, dtype = _frames(frames, ofc.device)
    if not 2 <= T1 <= MAX_FRAMES:
        raise FotgError("background takes 2 .. %d frames" % MAX_FRAMES)
    if T1 - 1 > ofc.max_batch:
        raise FotgError("%d frames need a context with max_batch >= %d" % (T1, T1 - 1))
    fw, mask = _sequence_flows(ofc, frames)
    params, moving = upsample_crop_fit_motion(ofc, fw, mask, model, code=True)
    exclude = None
    if exclude_moving:
        exclude = torch.zeros((T1, h, w), dtype=torch.uint8, device=ofc.device)
        exclude[:T1 - 1] = (moving == 1).to(torch.uint8)
    motions = plate_motions(params, ref)
    W, H, ox, oy = mosaic_canvas(motions, w, h) if mosaic else (w, h, 0, 0)
    dst, cnt, code = background_plate(frames, None, motions=motions, canvas=(W, H), origin=(ox, oy), exclude=exclude, mode=mode,
                                      min_count=min_count, count=True, code=True)
    return dst[0], code[0], cnt[0], motions


def ofc_background(ofc, frames, ref=0, model="affine", mosaic=False, mode="median", exclude_moving=True, min_count=1):
    """OFClass.background: frames (T+1, h, w[, c]), 2 <= T+1 <= 32 -> (plate, code, count) of the shot in the coordinates of frame
    `ref`.  The composition, call for call: the sequence flows (on a bidir context with the forward consistency mask),
    upsample_crop_fit_motion with its code, the code-1 pixels (independent motion) of frame k as exclude[k] (exclude_moving; a zero
    map for the last frame, which has no flow), plate_motions(params, ref), the canvas -- the frame grid, or with mosaic
    mosaic_canvas(motions, w, h) -- and background_plate(frames, None, motions=motions, ...) with code and count."""
    return _ofc_plate(ofc, frames, ref, model, mosaic, mode, exclude_moving, min_count)[:3]


callable_module(__name__, __name__, "background_plate")
