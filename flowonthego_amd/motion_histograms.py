"""python -m flowonthego_amd.motion_histograms flow.flo out.npz [--cell 8|16|32] [--thresh PX] [--mask m.png]
                                               [--model none|translation|similarity|affine] [--ids ids.npy --rows K]

Turns flow.flo into motion histograms on the GPU (flowonthego_amd.histograms.motion_histograms): per cell of --cell pixels the
histogram of optical flow (HOF, eight orientation bins and a zero bin for vectors shorter than --thresh pixels) and the two
motion-boundary histograms (MBHx, MBHy).  --model: the camera motion fitted to the flow first and subtracted (default none);
--mask: an 8-bit gray PNG of the flow's size, 0 = the pixel takes part (the mask of python -m flowonthego_amd.fb_check);
--ids: an int32 (h, w) array, per pixel the row of its object or -1 (python -m flowonthego_amd.moving_objects --ids), for one
record per object, --rows of them.  out.npz gets cells (and objects, and params), and descriptors, the 25 normalised values per
cell.  Prints the image's summed HOF and the share of the admissible pixels in the zero bin.

The module is callable: flowonthego_amd.motion_histograms(flow, ...) is flowonthego_amd.histograms.motion_histograms(flow, ...)."""
import argparse
import sys

from ._lib import callable_module


def main(argv=None):
    ap = argparse.ArgumentParser(prog="motion_histograms", description=__doc__.splitlines()[0])
    ap.add_argument("flow")
    ap.add_argument("out")
    ap.add_argument("--cell", type=int, default=16)
    ap.add_argument("--thresh", type=float, default=0.4)
    ap.add_argument("--mask", default=None)
    ap.add_argument("--model", default="none")
    ap.add_argument("--ids", default=None)
    ap.add_argument("--rows", type=int, default=256)
    a = ap.parse_args(sys.argv[1:] if argv is None else argv)
    if a.cell not in (8, 16, 32) or not 0 <= a.thresh <= 8192:
        ap.error("--cell must be 8, 16 or 32 and --thresh in 0 .. 8192")
    if a.rows < 1 or a.rows > 1024:
        ap.error("--rows must be in 1 .. 1024")
    from .motion import MODELS                           # (imports torch: after the checks that do not need it)
    if a.model != "none" and a.model not in MODELS:
        ap.error("--model must be one of none, " + ", ".join(MODELS))
    import numpy as np
    from ._cli import load_array, load_flow, load_mask_png, mask_like_flow, refusing, to_device
    from .histograms import HOF, ZERO, motion_descriptors, motion_histograms
    from .motion import fit_motion
    with refusing("motion_histograms") as inputs:
        flow = load_flow(a.flow)
        h, w = flow.shape[:2]
        mask = mask_like_flow(load_mask_png(a.mask), a.mask, h, w)
        ids = mask_like_flow(load_array(a.ids), a.ids, h, w, "int32")
    if inputs.refused:
        return 1
    f, m = to_device(flow), to_device(mask)
    params = None if a.model == "none" else fit_motion(f, m, a.model)
    out = motion_histograms(f, m, params, a.cell, a.thresh, to_device(ids), a.rows)
    cells = out[0] if ids is not None else out
    save = {"cells": cells.cpu().numpy(), "descriptors": motion_descriptors(cells).cpu().numpy()}
    if ids is not None:
        save["objects"] = out[1].cpu().numpy()
    if params is not None:
        save["params"] = params.cpu().numpy()
    np.savez(a.out, **save)
    total = save["cells"].reshape(-1, 32).sum(0)
    print("HOF " + " ".join("%d" % v for v in total[HOF]))
    print("zero bin %d of %d admissible pixels (%.4f), %d not admissible" % (total[ZERO], total[25], total[ZERO] / max(int(total[25]), 1), total[27]))
    return 0


callable_module(__name__, __package__ + ".histograms", "motion_histograms")

if __name__ == "__main__":
    sys.exit(main())
