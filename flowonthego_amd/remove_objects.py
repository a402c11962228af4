"""python -m flowonthego_amd.remove_objects frames.npy out.npy [--mask mask.npy] [--ref K] [--model M] [--low L] [--high H] [--window R]
                                            [--min-area N] [--open R] [--close R] [--grow G] [--feather F] [--plate plate.png] [--code code.npy]
                                            [--op-point K]

A shot without its moving objects, on the GPU: the clean plate of the frames on frame --ref (OFClass.background), what stands out
against it in every frame (OFClass.foreground), and that mask, grown by a disc and feathered, filled from the plate along the camera
motion (OFClass.remove_objects; flowonthego_amd.erase).  frames.npy: a (T, h, w) or (T, h, w, 3) uint8 or float32 array of 2 .. 32
frames; out.npy: the frames of the same shape and type without the objects.  --mask: a (T, h, w) uint8 array, non-zero = take this
pixel out, instead of the objects found.  --ref: the frame whose coordinates the plate has (default 0); --model: the camera motion
fitted to each flow, translation, similarity or affine (default); --low, --high, --window, --min-area: the background subtraction's
thresholds in grey levels (defaults 8 and 24), window 0, 1 (default) or 2 and smallest object in pixels (default 64); --open, --close: the radii 0 .. 8 of the discs the foreground is opened and closed by
before the objects are taken (flowonthego_amd.morph; default 0 and 0: as it is; 2 and 2 did best on the jittered road crops); --grow: the
radius in pixels of the disc the mask is grown by, 0 .. 8 (default 2); --feather: the width in pixels of the ramp beyond it, 0 .. 8
(default 3); --plate: the plate as a PNG; --code: the (T, h, w) uint8 code map (0 untouched, 1 replaced, 2 no plate there, 3
unknown, 4 blended).  Prints per frame the shares of replaced and blended pixels and the number of pixels under the grown mask that
were kept because the plate or the motion knows nothing there: nothing is inpainted.

The module is callable: flowonthego_amd.remove_objects(frames, plate, remove, ...) is flowonthego_amd.erase.remove_objects(frames, plate, remove, ...)."""
import argparse
import sys

from ._lib import callable_module

MODELS = ("translation", "similarity", "affine")


def main(argv=None):
    ap = argparse.ArgumentParser(prog="remove_objects", description=__doc__.splitlines()[4])
    ap.add_argument("files", nargs="+", help="frames.npy out.npy")
    ap.add_argument("--mask", default=None)
    ap.add_argument("--ref", type=int, default=0)
    ap.add_argument("--model", default="affine")
    ap.add_argument("--low", type=float, default=8.0)
    ap.add_argument("--high", type=float, default=24.0)
    ap.add_argument("--window", type=int, default=1)
    ap.add_argument("--min-area", type=int, default=64)
    ap.add_argument("--open", type=int, default=0, help="radius 0 .. 8 the foreground is opened by (default 0: not at all; try 2)")
    ap.add_argument("--close", type=int, default=0, help="radius 0 .. 8 it is then closed by (default 0: not at all; try 2)")
    ap.add_argument("--grow", type=int, default=2)
    ap.add_argument("--feather", type=int, default=3)
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
    if not (0 <= a.grow <= 8 and 0 <= a.feather <= 8):
        ap.error("--grow and --feather must lie in 0 .. 8")
    if not (0 <= a.open <= 8 and 0 <= a.close <= 8):
        ap.error("--open and --close must lie in 0 .. 8")
    from ._cli import Refusal, drop_c1, frame_sequence, load_array, refusing, save_frame_png, sequence_context, to_device
    with refusing("remove_objects") as inputs:
        frames = drop_c1(frame_sequence(a.files[0], 2, "T", c1=True))
        T = frames.shape[0]
        if T > 32:
            raise Refusal("%s holds %d frames, a plate takes at most 32" % (a.files[0], T))
        if a.ref >= T:
            raise Refusal("%s holds %d frames: --ref must be below that" % (a.files[0], T))
        given = load_array(a.mask)
        if given is not None and (given.shape != frames.shape[:3] or str(given.dtype) != "uint8"):
            raise Refusal("%s must hold a %s uint8 array, one value per pixel of %s" % (a.mask, tuple(frames.shape[:3]), a.files[0]))
    if inputs.refused:
        return 1
    import numpy as np
    from .erase import ofc_remove_objects
    ofc = sequence_context(frames, a.op_point, bidir=False, max_batch=T - 1)
    clean, code, mask, plate = ofc_remove_objects(ofc, to_device(frames), ref=a.ref, model=a.model, low=a.low, high=a.high, window=a.window,
                                                  min_area=a.min_area, grow=a.grow, feather=a.feather, mask=to_device(given), open=a.open,
                                                  close=a.close)
    code = code.cpu().numpy()
    h, w = code.shape[1:]
    np.save(a.files[1], clean.cpu().numpy())
    if a.plate:
        save_frame_png(a.plate, plate, h, w)
    if a.code:
        np.save(a.code, code)
    ofc.close()
    print("objects removed from %d frames of %d x %d with the plate on frame %d, grow %d, feather %d:" % (T, w, h, a.ref, a.grow, a.feather))
    for k in range(T):
        print("  frame %d: replaced %.4f, blended %.4f, %d pixels kept for want of a plate or a vector"
              % (k, float((code[k] == 1).mean()), float((code[k] == 4).mean()), int(((code[k] == 2) | (code[k] == 3)).sum())))
    return 0


callable_module(__name__, __package__ + ".erase", "remove_objects")

if __name__ == "__main__":
    sys.exit(main())
