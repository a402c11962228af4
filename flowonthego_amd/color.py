"""Middlebury flow colour code on the GPU (flow_code/C/color_flow.cpp MotionToColor + colorcode.cpp computeColor of the reference
tree) over fotg_flow_color / fotg_upsample_crop_color of libfotg.so, and the legend image of colortest.cpp (the PNG writer: _png.py).
The colour code runs in HIP only; there is no CPU fallback.  Output is uint8 R, G, B per pixel, normalised per image."""
import ctypes as C

import numpy as np
import torch

from ._args import _dev_f32, _ptr, _stream, coarse_flow, coarse_shape, dense_flow
from ._lib import check, lib
from ._png import write_png  # noqa: F401  (its place before _png.py; still importable from here)


def _maxmotion(maxmotion):
    return C.c_float(-1.0 if maxmotion is None else float(maxmotion))


def _out_rgb(out, shape, device):
    if out is None:
        return torch.empty(shape, dtype=torch.uint8, device=device)
    return _dev_f32(out, "out", device, shape, dtype=torch.uint8)


def flow_to_color(flow, maxmotion=None, out=None, stats=False):
    """flow: device tensor (n, h, w, 2) or (h, w, 2) float32 -> uint8 (n, h, w, 3) or (h, w, 3), R, G, B.
    maxmotion None (or <= 0): each image normalised by its own largest known |(u, v)|, as color_flow without its argument.
    stats=True also returns an (n, 5) float32 tensor: maxrad, minu, maxu, minv, maxv over the known vectors (what color_flow prints).
    Asynchronous on the current stream of the flow's device."""
    f, single, n, h, w = dense_flow(flow)
    rgb = _out_rgb(out.unsqueeze(0) if (single and out is not None) else out, (n, h, w, 3), f.device)
    st = torch.empty((n, 5), dtype=torch.float32, device=f.device)
    check(lib().fotg_flow_color(f.device.index or 0, n, _ptr(f), w, h, _maxmotion(maxmotion), _ptr(rgb), _ptr(st), _stream(f.device)))
    rgb = rgb[0] if single else rgb
    return (rgb, st) if stats else rgb


def upsample_crop_color(ofc, flow, maxmotion=None, out=None, stats=False):
    """OFClass.upsample_crop_color: the context's coarse flow (n, h_l, w_l, 2) -> uint8 (n, h_org, w_org, 3), byte for byte
    flow_to_color(ofc.upsample_crop(flow)) without the full-resolution flow ever being written."""
    n = coarse_flow(ofc, flow, "the colour code needs a two-channel flow", "flow")
    coarse_shape(ofc, flow, "flow", n)
    rgb = _out_rgb(out, (n, ofc.height_org, ofc.width_org, 3), ofc.device)
    st = torch.empty((n, 5), dtype=torch.float32, device=ofc.device)
    check(lib().fotg_upsample_crop_color(ofc._h, n, _ptr(flow), _maxmotion(maxmotion), _ptr(rgb), _ptr(st), _stream(ofc.device)))
    return (rgb, st) if stats else rgb


def color_wheel(truerange, size=151, device=0):
    """the legend image of the reference's colortest.cpp: (size, size, 3) uint8 on the host.  Flow (fx, fy) per pixel with its
    float expressions, coloured by the kernel with maxmotion = truerange (= computeColor(fx / truerange, fy / truerange)), black
    coordinate axes and tick marks at the integers up to truerange."""
    f32 = np.float32
    truerange, size = f32(truerange), int(size)    # float truerange = atof(...)
    if not truerange > 0 or size < 3:
        raise ValueError("color_wheel needs truerange > 0 and size >= 3")
    rng = f32(1.04 * float(truerange))             # float range = 1.04 * truerange (the product in double)
    s2 = size // 2
    t = np.arange(size, dtype=f32) / f32(s2) * rng - rng
    flow = np.empty((size, size, 2), f32)
    flow[..., 0] = t[None, :]
    flow[..., 1] = t[:, None]
    out = flow_to_color(torch.from_numpy(flow).cuda(device), maxmotion=truerange).cpu().numpy()
    out[s2, :] = 0                                 # x == s2 || y == s2: the axes stay black
    out[:, s2] = 0
    ir, ticksize = int(truerange), (1 if size < 120 else 2)
    for k in range(-ir, ir + 1):
        ik = int(f32(k) / rng * f32(s2)) + s2
        for tt in range(-ticksize, ticksize + 1):
            out[s2 + tt, ik] = 0
            out[ik, s2 + tt] = 0
    return out
