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

from ._lib import callable_module

CODE_RGB = ((0, 0, 0), (255, 255, 255), (220, 30, 30), (128, 128, 128))


def _sequence(a):
    import numpy as np
    from ._cli import frame_sequence, refusing, sequence_context, to_device
    with refusing("motion_blur") as inputs:
        frames = frame_sequence(a.files[0], 2, "T+1", c1=False)
    if inputs.refused:
        return 1
    T, h, w = frames.shape[0] - 1, frames.shape[1], frames.shape[2]
    ofc = sequence_context(frames, a.op_point, bidir=a.occlusion, max_batch=min(T, 8))
    out = ofc.motion_blur(to_device(frames), a.shutter, a.max_blur, occlusion=a.occlusion)
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
    if len(a.files) == 2:
        return _sequence(a)
    from ._cli import frame_like_flow, load_array, load_flow, load_mask_png, mask_like_flow, refusing, save_code_png, save_frame_png, to_device
    from .motionblur import motion_blur
    with refusing("motion_blur") as inputs:
        flow = load_flow(a.files[1])
        h, w = flow.shape[:2]
        frame = frame_like_flow(load_array(a.files[0]), a.files[0], h, w)
        mask = mask_like_flow(load_mask_png(a.mask), a.mask, h, w)
    if inputs.refused:
        return 1
    dst, code, st = motion_blur(to_device(frame), to_device(flow), to_device(mask), a.shutter, a.max_blur, code=True, stats=True)
    st = st.cpu().numpy()
    save_frame_png(a.files[2], dst, h, w)
    if a.code:
        save_code_png(a.code, code, CODE_RGB)
    print("untouched %.4f  blurred %.4f  clamped %.4f  unknown %.4f  taps per pixel %.3f  longest half-streak %.4f px" % (
        st[0] / (h * w), st[1] / (h * w), st[2] / (h * w), st[3] / (h * w), st[4] / (h * w), st[6] / 16.0))
    return 0


callable_module(__name__, __package__ + ".motionblur", "motion_blur")

if __name__ == "__main__":
    sys.exit(main())
