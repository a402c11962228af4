"""python -m flowonthego_amd.background frames.npy out.png [--ref K] [--model M] [--mosaic] [--mode median|mean] [--keep-moving]
                                        [--min-count N] [--code c.png] [--count n.png] [--op-point K]

The clean plate of a shot on the GPU: the scene without its moving objects, the median over the frames pulled onto frame --ref along
the camera motion (OFClass.background; flowonthego_amd.plate).  frames.npy: a (T, h, w) or (T, h, w, 3) uint8 or float32 array of
2 .. 32 frames; --ref: the frame whose coordinates the plate has (default 0); --model: the camera motion fitted to each flow,
translation, similarity or affine (default); --mosaic: the canvas that holds every frame (the panorama of a panning shot) instead of
the frame grid; --mode: median (default) or mean; --keep-moving: the pixels that move on their own take part (by default the fit's
code 1 keeps them out); --min-count: the fewest frames a pixel needs (default 1); --code: the per-pixel code as a PNG (estimated:
white, covered but hidden: red, covered by too few frames: gray); --count: the number of frames used per pixel as a gray PNG,
scaled to 255 for all T.  Prints the canvas and the shares of the three codes.

The module is callable: flowonthego_amd.background(frames, ...) is flowonthego_amd.plate.background_plate(frames, ...)."""
import argparse
import sys

from ._lib import callable_module

MODELS = ("translation", "similarity", "affine")


def main(argv=None):
    ap = argparse.ArgumentParser(prog="background", description=__doc__.splitlines()[3])
    ap.add_argument("files", nargs="+", help="frames.npy out.png")
    ap.add_argument("--ref", type=int, default=0)
    ap.add_argument("--model", default="affine")
    ap.add_argument("--mosaic", action="store_true")
    ap.add_argument("--mode", default="median")
    ap.add_argument("--keep-moving", action="store_true")
    ap.add_argument("--min-count", type=int, default=1)
    ap.add_argument("--code", default=None)
    ap.add_argument("--count", default=None)
    ap.add_argument("--op-point", type=int, default=2)
    a = ap.parse_args(sys.argv[1:] if argv is None else argv)
    if len(a.files) != 2:
        ap.error("expected frames.npy out.png")
    if a.model not in MODELS:
        ap.error("--model must be one of %s" % ", ".join(MODELS))
    if a.mode not in ("median", "mean"):
        ap.error("--mode must be median or mean")
    if a.ref < 0 or not 1 <= a.min_count <= 32:
        ap.error("--ref must be >= 0 and --min-count in 1 .. 32")
    from ._cli import Refusal, drop_c1, frame_sequence, refusing, save_code_png, save_frame_png, sequence_context, to_device
    with refusing("background") as inputs:
        frames = drop_c1(frame_sequence(a.files[0], 2, "T", c1=True))
        T = frames.shape[0]
        if T > 32:
            raise Refusal("%s holds %d frames, a plate takes at most 32" % (a.files[0], T))
        if a.ref >= T or a.min_count > T:
            raise Refusal("%s holds %d frames: --ref must be below and --min-count at most that" % (a.files[0], T))
    if inputs.refused:
        return 1
    import numpy as np
    ofc = sequence_context(frames, a.op_point, bidir=False, max_batch=T - 1)
    plate, code, count = ofc.background(to_device(frames), ref=a.ref, model=a.model, mosaic=a.mosaic, mode=a.mode,
                                        exclude_moving=not a.keep_moving, min_count=a.min_count)
    H, W = code.shape
    save_frame_png(a.files[1], plate, H, W)
    code = code.cpu().numpy()
    if a.code:
        save_code_png(a.code, code)
    if a.count:
        save_frame_png(a.count, (count.cpu().numpy().astype(np.uint32) * 255 // T).astype(np.uint8), H, W)
    ofc.close()
    n = np.bincount(code.ravel(), minlength=3) / float(H * W)
    print("plate %d x %d from %d frames of %d x %d: estimated %.4f  hidden %.4f  uncovered %.4f" % (
        W, H, T, frames.shape[2], frames.shape[1], n[0], n[1], n[2]))
    return 0


callable_module(__name__, __package__ + ".plate", "background_plate")

if __name__ == "__main__":
    sys.exit(main())
