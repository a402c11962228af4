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
    from ._cli import flow_like_flow, frame_like_flow, load_array, load_flow, occlusion_mask, refusing, save_code_png, to_device
    from .flo import write_flo
    from .flowfilter import filter_flow
    with refusing("filter_flow") as inputs:
        flow = load_flow(a.flow)
        h, w = flow.shape[:2]
        bw = flow_like_flow(load_flow(a.bw), a.bw, flow, a.flow)
        guide = frame_like_flow(load_array(a.guide), a.guide, h, w)
    if inputs.refused:
        return 1
    f = to_device(flow)
    mask = occlusion_mask(f, to_device(bw))
    out, code, st = filter_flow(f, to_device(guide), mask=mask, radius=a.radius, sigma=sigma, tau=a.tau, iters=a.iters, stats=True)
    st = st.cpu().numpy()
    write_flo(a.out, out)
    print("filtered %.4f  filled %.4f  unsupported %.4f  mean change %.4f px"
          % (st[0] / (h * w), st[1] / (h * w), st[2] / (h * w), st[3] / max(2.0 * st[0], 1.0)))
    if a.code:
        save_code_png(a.code, code)
    return 0


callable_module(__name__, __package__ + ".flowfilter", "filter_flow")

if __name__ == "__main__":
    sys.exit(main())
