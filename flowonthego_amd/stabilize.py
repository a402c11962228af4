"""python -m flowonthego_amd.stabilize frames.npy out.npy [--model translation|similarity|affine] [--radius N] [--op-point K]
                                       [--fill V]

Stabilises a video on the GPU: frames.npy holds a (T+1, h, w) or (T+1, h, w, 3) uint8 or float32 array.  The flows of the sequence
are computed (both directions, so that occluded pixels stay out of the fit), a camera motion is fitted to each, the camera path is
smoothed over --radius frames to either side and every frame resampled along the smoothed path (OFClass.stabilize).  out.npy gets
the stabilised frames, same shape and type.  --fill V: pixels the resampling cannot fill get V instead of the border's colour.
Prints the share of such pixels per frame.

The module is callable: flowonthego_amd.stabilize(frames, flows, ...) is flowonthego_amd.motion.stabilize(frames, flows, ...)."""
import argparse
import sys

from ._lib import callable_module


def main(argv=None):
    from .motion import MODELS
    ap = argparse.ArgumentParser(prog="stabilize", description=__doc__.splitlines()[0])
    ap.add_argument("frames")
    ap.add_argument("out")
    ap.add_argument("--model", default="similarity", choices=MODELS)
    ap.add_argument("--radius", type=int, default=15)
    ap.add_argument("--op-point", type=int, default=2)
    ap.add_argument("--fill", type=float, default=None)
    a = ap.parse_args(sys.argv[1:] if argv is None else argv)
    if a.radius < 0:
        ap.error("--radius must be >= 0")
    import numpy as np
    from ._cli import drop_c1, frame_sequence, refusing, sequence_context, to_device
    with refusing("stabilize") as inputs:
        frames = drop_c1(frame_sequence(a.frames, 2, "T+1", c1=True))
    if inputs.refused:
        return 1
    ofc = sequence_context(frames, a.op_point, bidir=True, max_batch=frames.shape[0] - 1)
    out, code = ofc.stabilize(to_device(frames), model=a.model, radius=a.radius, fill=a.fill)
    np.save(a.out, out.cpu().numpy())
    holes = (code != 0).float().mean(dim=(1, 2)).cpu().numpy()
    print("unfilled share per frame: " + " ".join("%.4f" % v for v in holes))
    ofc.close()
    return 0


callable_module(__name__, __package__ + ".motion", "stabilize")

if __name__ == "__main__":
    sys.exit(main())
