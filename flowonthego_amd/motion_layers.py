"""python -m flowonthego_amd.motion_layers flow.flo out.png [--layers K] [--model translation|similarity|affine] [--iters I]
                                            [--rounds R] [--thresh PX] [--mask m.png] [--params p.npy]

Splits flow.flo into up to K motion layers on the GPU (flowonthego_amd.layers.motion_layers): layer 0 the camera motion, every
further layer a motion of the same model that explains what the earlier ones do not.  out.png is the label map: one colour per
layer (layer 0 white), unassigned pixels red, masked gray, unknown black.  Prints one line per layer: its six parameters
a00 a01 tx a10 a11 ty and the share of the pixels it holds ("dead" for a layer nothing was left for), then the shares of the
unassigned, masked and unknown pixels.
--mask: an 8-bit gray PNG of the flow's size, 0 = the pixel takes part (the mask of python -m flowonthego_amd.fb_check);
--params: the (K, 6) float64 parameters as an .npy file.

The module is callable: flowonthego_amd.motion_layers(flow, ...) is flowonthego_amd.layers.motion_layers(flow, ...)."""
import argparse
import sys

from ._cli import CODE_RGB
from ._lib import callable_module

# eight layer colours (layer 0 white, as the good case of CODE_RGB); unassigned, masked, unknown at 253 .. 255 take CODE_RGB's last three
LAYER_RGB = ((255, 255, 255), (40, 110, 220), (50, 170, 70), (240, 160, 30), (150, 70, 190), (30, 180, 190), (230, 210, 50), (140, 90, 50))


def palette():
    """the 256 colours of a label map: the layers, then black up to the three codes at 253 .. 255"""
    return LAYER_RGB + ((0, 0, 0),) * (253 - len(LAYER_RGB)) + tuple(CODE_RGB[1:])


def main(argv=None):
    ap = argparse.ArgumentParser(prog="motion_layers", description=__doc__.splitlines()[0])
    ap.add_argument("flow")
    ap.add_argument("out")
    ap.add_argument("--layers", type=int, default=3)
    ap.add_argument("--model", default="affine")
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--thresh", type=float, default=1.0)
    ap.add_argument("--mask", default=None)
    ap.add_argument("--params", default=None)
    a = ap.parse_args(sys.argv[1:] if argv is None else argv)
    if a.layers < 1 or a.layers > 8:
        ap.error("--layers must be in 1 .. 8")
    if a.iters < 0 or a.iters > 64 or a.rounds < 0 or a.rounds > 64 or not a.thresh >= 0:
        ap.error("--iters and --rounds must be in 0 .. 64 and --thresh >= 0")
    from .motion import MODELS                           # (imports torch: after the checks that do not need it)
    if a.model not in MODELS:
        ap.error("--model must be one of " + ", ".join(MODELS))
    import numpy as np
    from ._cli import load_flow, load_mask_png, mask_like_flow, refusing, save_code_png, to_device
    from .layers import LAYER_STATS, motion_layers
    with refusing("motion_layers") as inputs:
        flow = load_flow(a.flow)
        h, w = flow.shape[:2]
        mask = mask_like_flow(load_mask_png(a.mask), a.mask, h, w)
    if inputs.refused:
        return 1
    params, labels, records, st = motion_layers(to_device(flow), to_device(mask), a.layers, a.model, a.iters, a.rounds, a.thresh,
                                                labels=True, records=True, stats=True)
    params, records, st = params.cpu().numpy(), records.cpu().numpy(), st.cpu().numpy()
    for k in range(a.layers):
        print("layer %d: %s  %s" % (k, " ".join("%.9g" % v for v in params[k]),
                                    "share %.4f" % (records[k, 0] / (h * w)) if records[k, 2] else "dead"))
    print("  ".join("%s %.4f" % (nm, c / (h * w)) for nm, c in zip(LAYER_STATS[:3], st[:3])))
    save_code_png(a.out, labels, palette())
    if a.params:
        np.save(a.params, params)
    return 0


callable_module(__name__, __package__ + ".layers", "motion_layers")

if __name__ == "__main__":
    sys.exit(main())
