"""python -m flowonthego_amd.foreground frames.npy out.npy [--ref K] [--model M] [--low L] [--high H] [--window R] [--min-area N]
                                        [--open R] [--close R] [--keep-moving] [--plate plate.png] [--code code.png] [--op-point K]

What does not belong to the background of a shot, on the GPU: the clean plate of the frames on frame --ref (OFClass.background),
every frame compared with it along the camera motion, and the connected regions of difference that hold at least one strongly
different pixel (OFClass.foreground; flowonthego_amd.subtract).  frames.npy: a (T, h, w) or (T, h, w, 3) uint8 or float32 array of
2 .. 32 frames; out.npy: the (T, h, w) uint8 mask of the confirmed objects.  --ref: the frame whose coordinates the plate has
(default 0); --model: the camera motion fitted to each flow, translation, similarity or affine (default); --low, --high: the two
thresholds in grey levels on the mean difference over the window (defaults 8 and 24): a region above --low counts only if it holds
a pixel above --high; --window: 0, 1 (default) or 2 for 1 x 1, 3 x 3, 5 x 5; --min-area: the smallest object in pixels (default
64); --open, --close: the radii 0 .. 8 of the discs the foreground is opened and closed by before the objects are taken
(flowonthego_amd.morph; default 0 and 0: as it is; 2 and 2 did best on the jittered road crops); --keep-moving: the pixels that move on their own take part in the plate; --plate: the plate as a PNG; --code: frame --ref's
code map as a PNG (background: white, foreground: red, no plate there: gray, unknown: black, strong foreground: dark red).
Prints the confirmed objects and the share of foreground per frame.

The module is callable: flowonthego_amd.foreground(frames, plate, ...) is flowonthego_amd.subtract.subtract_background(frames, plate, ...)."""
import argparse
import sys

from ._lib import callable_module

MODELS = ("translation", "similarity", "affine")
STRONG_RGB = (120, 0, 0)           # code 4, after the four shared colours


def main(argv=None):
    ap = argparse.ArgumentParser(prog="foreground", description=__doc__.splitlines()[3])
    ap.add_argument("files", nargs="+", help="frames.npy out.npy")
    ap.add_argument("--ref", type=int, default=0)
    ap.add_argument("--model", default="affine")
    ap.add_argument("--low", type=float, default=8.0)
    ap.add_argument("--high", type=float, default=24.0)
    ap.add_argument("--window", type=int, default=1)
    ap.add_argument("--min-area", type=int, default=64)
    ap.add_argument("--open", type=int, default=0, help="radius 0 .. 8 the foreground is opened by (default 0: not at all; try 2)")
    ap.add_argument("--close", type=int, default=0, help="radius 0 .. 8 it is then closed by (default 0: not at all; try 2)")
    ap.add_argument("--keep-moving", action="store_true")
    ap.add_argument("--plate", default=None)
    ap.add_argument("--code", default=None)
    ap.add_argument("--op-point", type=int, default=2)
    a = ap.parse_args(sys.argv[1:] if argv is None else argv)
    if len(a.files) != 2:
        ap.error("expected frames.npy out.npy")
    if a.model not in MODELS:
        ap.error("--model must be one of %s" % ", ".join(MODELS))
    if not 0 <= a.low <= a.high <= 2047.9375:            # (a NaN fails the comparison)
        ap.error("--low and --high must satisfy 0 <= low <= high <= 2047.9375")
    if a.window not in (0, 1, 2) or a.ref < 0 or a.min_area < 1:
        ap.error("--window must be 0, 1 or 2, --ref >= 0 and --min-area >= 1")
    if not (0 <= a.open <= 8 and 0 <= a.close <= 8):
        ap.error("--open and --close must lie in 0 .. 8")
    from ._cli import CODE_RGB, Refusal, drop_c1, frame_sequence, refusing, save_code_png, save_frame_png, sequence_context, to_device
    with refusing("foreground") as inputs:
        frames = drop_c1(frame_sequence(a.files[0], 2, "T", c1=True))
        T = frames.shape[0]
        if T > 32:
            raise Refusal("%s holds %d frames, a plate takes at most 32" % (a.files[0], T))
        if a.ref >= T:
            raise Refusal("%s holds %d frames: --ref must be below that" % (a.files[0], T))
    if inputs.refused:
        return 1
    import numpy as np
    ofc = sequence_context(frames, a.op_point, bidir=False, max_batch=T - 1)
    mask, objects, confirmed, plate, code = ofc.foreground(to_device(frames), ref=a.ref, model=a.model, low=a.low, high=a.high,
                                                           window=a.window, min_area=a.min_area, exclude_moving=not a.keep_moving,
                                                           open=a.open, close=a.close)
    mask, confirmed = mask.cpu().numpy(), confirmed.cpu().numpy()
    h, w = mask.shape[1:]
    np.save(a.files[1], mask)
    if a.plate:
        save_frame_png(a.plate, plate, h, w)
    if a.code:
        save_code_png(a.code, code[a.ref], CODE_RGB + (STRONG_RGB,))
    ofc.close()
    print("foreground of %d frames of %d x %d against the plate on frame %d:" % (T, w, h, a.ref))
    for k in range(T):
        print("  frame %d: %d confirmed objects, foreground %.4f" % (k, int(confirmed[k].sum()), float(mask[k].mean())))
    return 0


callable_module(__name__, __package__ + ".subtract", "subtract_background")

if __name__ == "__main__":
    sys.exit(main())
