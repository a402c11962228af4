"""python -m flowonthego_amd.filter_flow flow.flo guide.npy out.flo [--bw bw.flo] [--radius R] [--sigma S] [--tau T] [--iters K]
                                         [--code out.png]

Filters flow.flo on the GPU, edge- and occlusion-aware (flowonthego_amd.flowfilter.filter_flow): guide.npy holds the frame the
flow belongs to, an (h, w) or (h, w, 3) uint8 or float32 array; every vector becomes the mean of the vectors of nearby pixels of
similar colour.  --radius (default 3, at most 7): the window is (2 R + 1)^2; --sigma: the Gaussian spatial weight (default: R / 2);
--tau (default 20): the mean absolute guide difference per channel at which a neighbour's weight reaches 0; --iters (default 1,
at most 4): passes.  --bw bw.flo (the flow frame 1 -> 0) runs the forward-backward check first: inconsistent vectors stay out of
the means and are filled from their neighbours.  --code: the per-pixel code as a PNG (filtered white, filled red, no support
black).  Prints the shares of the three codes and the mean change of a filtered vector's components.

The module is callable: flowonthego_amd.filter_flow(flow, guide, ...) is flowonthego_amd.flowfilter.filter_flow(flow, guide, ...)."""
import argparse
import sys

from ._lib import callable_module

CODE_RGB = ((255, 255, 255), (220, 30, 30), (128, 128, 128), (0, 0, 0))


def main(argv=None):
    ap = argparse.ArgumentParser(prog="filter_flow", description=__doc__.splitlines()[3])
    ap.add_argument("flow")
    ap.add_argument("guide")
    ap.add_argument("out")
    ap.add_argument("--bw", default=None)
    ap.add_argument("--radius", type=int, default=3)
    ap.add_argument("--sigma", type=float, default=None)
    ap.add_argument("--tau", type=float, default=20.0)
    ap.add_argument("--iters", type=int, default=1)
    ap.add_argument("--code", default=None)
    a = ap.parse_args(sys.argv[1:] if argv is None else argv)
    if not 1 <= a.radius <= 7:
        ap.error("--radius must be 1 .. 7")
    if not 1 <= a.iters <= 4:
        ap.error("--iters must be 1 .. 4")
    if not (a.tau > 0 and a.tau < float("inf")):
        ap.error("--tau must be a positive number")
    sigma = a.radius / 2.0 if a.sigma is None else a.sigma
    if not (sigma > 0 and sigma < float("inf")):
        ap.error("--sigma must be a positive number")
    import numpy as np
    import torch
    from .color import write_png
    from .flo import read_flo, write_flo
    from .flowfilter import filter_flow
    try:
        flow = read_flo(a.flow)
        bw = None if a.bw is None else read_flo(a.bw)
        guide = np.load(a.guide)
    except (OSError, ValueError) as e:
        sys.stderr.write("filter_flow: %s\n" % e)
        return 1
    h, w = flow.shape[:2]
    if guide.dtype not in (np.uint8, np.float32) or guide.shape not in ((h, w), (h, w, 1), (h, w, 3)):
        sys.stderr.write("filter_flow: %s must hold an (%d, %d) or (%d, %d, 3) uint8 or float32 array\n" % (a.guide, h, w, h, w))
        return 1
    if bw is not None and bw.shape != flow.shape:
        sys.stderr.write("filter_flow: %s is %dx%d, %s is %dx%d\n" % (a.flow, w, h, a.bw, bw.shape[1], bw.shape[0]))
        return 1
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    f, mask = dev(flow), None
    if bw is not None:
        from .consistency import fb_check
        mask = fb_check(f, dev(bw))[0]
    out, code, st = filter_flow(f, dev(guide), mask=mask, radius=a.radius, sigma=sigma, tau=a.tau, iters=a.iters, stats=True)
    st = st.cpu().numpy()
    write_flo(a.out, out)
    print("filtered %.4f  filled %.4f  unsupported %.4f  mean change %.4f px"
          % (st[0] / (h * w), st[1] / (h * w), st[2] / (h * w), st[3] / max(2.0 * st[0], 1.0)))
    if a.code:
        write_png(a.code, np.array(CODE_RGB, np.uint8)[code.cpu().numpy()])
    return 0


callable_module(__name__, __package__ + ".flowfilter", "filter_flow")

if __name__ == "__main__":
    sys.exit(main())
