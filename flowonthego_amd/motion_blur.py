"""python -m flowonthego_amd.motion_blur frame.npy flow.flo out.png [--shutter S] [--max-blur R] [--mask m.png] [--code c.png]
   python -m flowonthego_amd.motion_blur frames.npy out.npy [--shutter S] [--max-blur R] [--occlusion] [--op-point K]

Blurs a frame along its flow on the GPU, as a camera with an open shutter would have (flowonthego_amd.motionblur.motion_blur).
frame.npy: an (h, w) or (h, w, 3) uint8 or float32 array; flow.flo: the flow of that frame; --shutter: the exposure as a fraction
of the frame interval, in (0, 2] (default 0.5, a 180 degree shutter); --max-blur: the longest half-streak, 1 .. 32 pixels (default
32); --mask: an 8-bit gray PNG of the flow's size, non-zero = the pixel has no vector of its own (the mask of python -m
flowonthego_amd.fb_check); --code: the per-pixel code as a PNG (untouched: black, blurred: white, a tap left the frame: red, unknown
vector: gray).  Prints the shares of the four codes, the mean number of taps per pixel and the longest half-streak in pixels.
The sequence form: frames.npy holds (T+1, h, w) or (T+1, h, w, 3) frames; their flows are computed (OFClass.motion_blur, --occlusion
with the forward-backward check) and out.npy gets frames 0 .. T-1 blurred, same type.

The module is callable: flowonthego_amd.motion_blur(frame, flow, ...) is flowonthego_amd.motionblur.motion_blur(frame, flow, ...)."""
import argparse
import sys
import zlib

from ._lib import callable_module

CODE_RGB = ((0, 0, 0), (255, 255, 255), (220, 30, 30), (128, 128, 128))


def _sequence(a, np, torch):
    from . import img_params, operating_point
    from .oflow import OFClass
    try:
        frames = np.load(a.files[0])
    except (OSError, ValueError) as e:
        sys.stderr.write("motion_blur: %s\n" % e)
        return 1
    if frames.ndim not in (3, 4) or frames.shape[0] < 2 or frames.dtype not in (np.uint8, np.float32) or (frames.ndim == 4 and frames.shape[3] != 3):
        sys.stderr.write("motion_blur: %s must hold a (T+1, h, w) or (T+1, h, w, 3) uint8 or float32 array of at least two frames\n" % a.files[0])
        return 1
    T, h, w = frames.shape[0] - 1, frames.shape[1], frames.shape[2]
    color = frames.ndim == 4
    u8_rgb = color and frames.dtype == np.uint8          # 8-bit colour frames become gray for the flow; float32 ones are used as RGB
    op = operating_point(a.op_point, w, 3 if color and not u8_rgb else 1)
    op.bidir = bool(a.occlusion)
    if u8_rgb:
        op.u8_color = 2
    ofc = OFClass(op, img_params(width=w, height=h), max_batch=min(T, 8))
    out = ofc.motion_blur(torch.from_numpy(np.ascontiguousarray(frames)).cuda(), a.shutter, a.max_blur, occlusion=a.occlusion)
    np.save(a.files[1], out.cpu().numpy())
    ofc.close()
    print("%d frames of %d x %d blurred, shutter %g" % (T, w, h, a.shutter))
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser(prog="motion_blur", description=__doc__.splitlines()[3])
    ap.add_argument("files", nargs="+", help="frame.npy flow.flo out.png | frames.npy out.npy")
    ap.add_argument("--shutter", type=float, default=0.5)
    ap.add_argument("--max-blur", type=int, default=32)
    ap.add_argument("--mask", default=None)
    ap.add_argument("--code", default=None)
    ap.add_argument("--occlusion", action="store_true")
    ap.add_argument("--op-point", type=int, default=2)
    a = ap.parse_args(sys.argv[1:] if argv is None else argv)
    if len(a.files) not in (2, 3):
        ap.error("expected frame.npy flow.flo out.png, or frames.npy out.npy")
    if not (0 < a.shutter <= 2) or round(256 * a.shutter) < 1:
        ap.error("--shutter must be in (0, 2]")
    if not 1 <= a.max_blur <= 32:
        ap.error("--max-blur must be in 1 .. 32")
    if len(a.files) == 2 and (a.mask or a.code):
        ap.error("--mask and --code belong to the single-frame form")
    if len(a.files) == 3 and a.occlusion:
        ap.error("--occlusion belongs to the sequence form")
    import numpy as np
    import torch
    if len(a.files) == 2:
        return _sequence(a, np, torch)
    from .color import write_png
    from .fit_motion import read_gray_png
    from .flo import read_flo
    from .motionblur import motion_blur
    try:
        frame, flow = np.load(a.files[0]), read_flo(a.files[1])
        mask = read_gray_png(a.mask) if a.mask else None
    except (OSError, ValueError, zlib.error) as e:
        sys.stderr.write("motion_blur: %s\n" % e)
        return 1
    h, w = flow.shape[:2]
    if frame.dtype not in (np.uint8, np.float32) or frame.shape[:2] != (h, w) or frame.shape[2:] not in ((), (1,), (3,)):
        sys.stderr.write("motion_blur: %s must hold a (%d, %d[, 3]) uint8 or float32 array (the flow's size)\n" % (a.files[0], h, w))
        return 1
    if mask is not None and mask.shape != (h, w):
        sys.stderr.write("motion_blur: %s is %d x %d, the flow %d x %d\n" % (a.mask, mask.shape[1], mask.shape[0], w, h))
        return 1
    dev = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()
    dst, code, st = motion_blur(dev(frame), dev(flow), dev(mask), a.shutter, a.max_blur, code=True, stats=True)
    st = st.cpu().numpy()
    img = dst.cpu().numpy().reshape(h, w, -1)
    if img.dtype != np.uint8:
        img = np.clip(np.rint(np.nan_to_num(img)), 0, 255).astype(np.uint8)
    write_png(a.files[2], np.ascontiguousarray(np.broadcast_to(img, (h, w, 3))))
    if a.code:
        write_png(a.code, np.array(CODE_RGB, np.uint8)[code.cpu().numpy()])
    print("untouched %.4f  blurred %.4f  clamped %.4f  unknown %.4f  taps per pixel %.3f  longest half-streak %.4f px" % (
        st[0] / (h * w), st[1] / (h * w), st[2] / (h * w), st[3] / (h * w), st[4] / (h * w), st[6] / 16.0))
    return 0


callable_module(__name__, __package__ + ".motionblur", "motion_blur")

if __name__ == "__main__":
    sys.exit(main())
