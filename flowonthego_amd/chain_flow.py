"""python -m flowonthego_amd.chain_flow f0.flo f1.flo ... out.flo [--bw b0.flo b1.flo ...] [--points pts.npy traj.npy]

Chains the flows f0.flo (frame 0 -> 1), f1.flo (frame 1 -> 2), ... of one sequence on the GPU (flowonthego_amd.chain) and writes
the displacement frame 0 -> T of every pixel of frame 0 as out.flo.  --bw: as many backward flows (bk.flo: frame k+1 -> k); every
step is then tested for forward-backward consistency.  --points: pts.npy, a (P, 2) float32 array of (x, y), is followed as well
and its trajectory written to traj.npy, (T+1, P, 2).  Prints
valid occluded outside unknown (fractions of the chains by their final code) mean_steps."""
import argparse
import sys


def main(argv=None):
    ap = argparse.ArgumentParser(prog="chain_flow", description=__doc__.splitlines()[0])
    ap.add_argument("flows", nargs="+", help="f0.flo [f1.flo ...] out.flo")
    ap.add_argument("--bw", nargs="+", default=None)
    ap.add_argument("--points", nargs=2, default=None, metavar=("pts.npy", "traj.npy"))
    a = ap.parse_args(sys.argv[1:] if argv is None else argv)
    if len(a.flows) < 2:
        ap.error("at least one flow and the output file are needed")
    paths, out = a.flows[:-1], a.flows[-1]
    if a.bw is not None and len(a.bw) != len(paths):
        ap.error("--bw needs as many flows as the forward sequence (%d)" % len(paths))
    import numpy as np
    from ._cli import Refusal, flow_like_flow, load_array, load_flow, refusing, to_device
    from .chain import STATS, chain, track_points
    from .flo import write_flo
    with refusing("chain_flow") as inputs:
        fw = [load_flow(p) for p in paths]
        bw = [load_flow(p) for p in a.bw] if a.bw else None
        h, w = fw[0].shape[:2]
        for f, p in zip(fw[1:] + (bw or []), paths[1:] + (a.bw or [])):
            flow_like_flow(f, p, fw[0], paths[0])
        pts = load_array(a.points[0]) if a.points else None
        if pts is not None and (pts.ndim != 2 or pts.shape[1] != 2 or pts.shape[0] < 1 or pts.dtype != np.float32):
            raise Refusal("%s must hold a (P, 2) float32 array" % a.points[0])
    if inputs.refused:
        return 1
    F, B = to_device(np.stack(fw)), None if bw is None else to_device(np.stack(bw))
    total, _, _, st = chain(F, B, stats=True)
    st = st.cpu().numpy()
    print("  ".join("%s %.4f" % (nm, c / (h * w)) for nm, c in zip(STATS[:4], st[:4])) + "  mean_steps %.4f" % (st[4] / (h * w)))
    write_flo(out, total.cpu().numpy())
    if pts is not None:
        traj, _, _ = track_points(to_device(pts), F, B)
        np.save(a.points[1], traj.cpu().numpy())
    return 0


if __name__ == "__main__":
    sys.exit(main())
