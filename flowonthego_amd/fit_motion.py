"""python -m flowonthego_amd.fit_motion flow.flo [--mask m.png] [--model translation|similarity|affine] [--iters N] [--thresh PX]
                                        [--code out.png]

Fits the camera motion that explains flow.flo on the GPU (flowonthego_amd.motion.fit_motion) and prints
a00 a01 tx a10 a11 ty, then the shares of the pixels that follow it, move on their own, are masked or unknown.
--mask: an 8-bit gray PNG of the flow's size, 0 = the pixel takes part (the mask of python -m flowonthego_amd.fb_check);
--code: the per-pixel code as a PNG (follows: white, independent: red, masked: gray, unknown: black).

The module is callable: flowonthego_amd.fit_motion(flow, ...) is flowonthego_amd.motion.fit_motion(flow, ...)."""
import argparse
import sys

from ._lib import callable_module
from ._png import read_gray_png  # noqa: F401  (its place before _png.py; still importable from here)


def main(argv=None):
    from .motion import MODELS
    ap = argparse.ArgumentParser(prog="fit_motion", description=__doc__.splitlines()[0])
    ap.add_argument("flow")
    ap.add_argument("--mask", default=None)
    ap.add_argument("--model", default="affine", choices=MODELS)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--thresh", type=float, default=1.0)
    ap.add_argument("--code", default=None)
    a = ap.parse_args(sys.argv[1:] if argv is None else argv)
    if a.iters < 0 or a.iters > 64 or not a.thresh >= 0:
        ap.error("--iters must be in 0 .. 64 and --thresh >= 0")
    from ._cli import load_flow, load_mask_png, mask_like_flow, refusing, save_code_png, to_device
    from .motion import CODES, fit_motion
    with refusing("fit_motion") as inputs:
        flow = load_flow(a.flow)
        h, w = flow.shape[:2]
        mask = mask_like_flow(load_mask_png(a.mask), a.mask, h, w)
    if inputs.refused:
        return 1
    params, code, st = fit_motion(to_device(flow), to_device(mask), a.model, a.iters, a.thresh, code=True, stats=True)
    st = st.cpu().numpy()
    print(" ".join("%.9g" % v for v in params.cpu().numpy()))
    print("  ".join("%s %.4f" % (nm, c / (h * w)) for nm, c in zip(CODES, st[:4])) + ("" if st[5] else "  (not fitted)"))
    if a.code:
        save_code_png(a.code, code)
    return 0


callable_module(__name__, __package__ + ".motion", "fit_motion")

if __name__ == "__main__":
    sys.exit(main())
