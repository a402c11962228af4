"""python -m flowonthego_amd.block_motion cur.npy ref.npy flow.flo out.npz [--block B] [--refine R] [--bw bw.flo] [--pred pred.png]

Block motion vectors for a video encoder on the GPU (flowonthego_amd.blockmotion.block_motion): cur.npy and ref.npy hold the frame
to predict and the frame to predict it from, (h, w) or (h, w, 3) uint8 arrays; flow.flo is the flow from cur to ref.  Per --block x
--block pixels (8, 16 or 32, default 16) one quarter-pel vector, chosen among the vectors the flow proposes for the block by its SAD
and refined by the last --refine (0 .. 3, default 2) of the full-, half- and quarter-pel steps.  --bw bw.flo (the flow ref -> cur)
runs the forward-backward check first: inconsistent vectors propose nothing.  Writes mv (bh, bw, 2) int16 in quarter pixels, cost
(bh, bw, 2) uint32 = [SAD, SAD of the zero vector] and kind (bh, bw) uint8 into out.npz; --pred: the prediction as a PNG.  Prints
the sum of the SADs, that of the zero vector and the PSNR of the prediction.

The module is callable: flowonthego_amd.block_motion(cur, ref, flow, ...) is flowonthego_amd.blockmotion.block_motion(...)."""
import argparse
import math
import sys

from ._lib import callable_module


def main(argv=None):
    ap = argparse.ArgumentParser(prog="block_motion", description=__doc__.splitlines()[2])
    ap.add_argument("cur")
    ap.add_argument("ref")
    ap.add_argument("flow")
    ap.add_argument("out")
    ap.add_argument("--block", type=int, default=16)
    ap.add_argument("--refine", type=int, default=2)
    ap.add_argument("--bw", default=None)
    ap.add_argument("--pred", default=None)
    a = ap.parse_args(sys.argv[1:] if argv is None else argv)
    if a.block not in (8, 16, 32):
        ap.error("--block must be 8, 16 or 32")
    if not 0 <= a.refine <= 3:
        ap.error("--refine must be 0 .. 3")
    import numpy as np
    import torch
    from .blockmotion import block_motion
    from .color import write_png
    from .flo import read_flo
    try:
        flow = read_flo(a.flow)
        bw = None if a.bw is None else read_flo(a.bw)
        cur, ref = np.load(a.cur), np.load(a.ref)
    except (OSError, ValueError) as e:
        sys.stderr.write("block_motion: %s\n" % e)
        return 1
    h, w = flow.shape[:2]
    for nm, f in ((a.cur, cur), (a.ref, ref)):
        if f.dtype != np.uint8 or f.shape not in ((h, w), (h, w, 1), (h, w, 3)) or f.shape != cur.shape:
            sys.stderr.write("block_motion: %s must hold an (%d, %d) or (%d, %d, 3) uint8 array, the same for both frames\n"
                             % (nm, h, w, h, w))
            return 1
    if bw is not None and bw.shape != flow.shape:
        sys.stderr.write("block_motion: %s is %dx%d, %s is %dx%d\n" % (a.flow, w, h, a.bw, bw.shape[1], bw.shape[0]))
        return 1
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    f, mask = dev(flow), None
    if bw is not None:
        from .consistency import fb_check
        mask = fb_check(f, dev(bw))[0]
    mv, cost, kind, pred, st = block_motion(dev(cur), dev(ref), f, mask=mask, block=a.block, refine=a.refine, pred=True, stats=True)
    st = st.cpu().numpy()
    np.savez(a.out, mv=mv.cpu().numpy(), cost=cost.cpu().numpy(), kind=kind.cpu().numpy())
    psnr = float("inf") if st[2] == 0 else 10.0 * math.log10(255.0 ** 2 * cur.size / float(st[2]))
    print("SAD %d  zero-vector SAD %d  prediction PSNR %.2f dB" % (st[0], st[1], psnr))
    if a.pred:
        p = pred.cpu().numpy().reshape(h, w, -1)
        write_png(a.pred, np.repeat(p, 3, axis=2) if p.shape[2] == 1 else p)
    return 0


callable_module(__name__, __package__ + ".blockmotion", "block_motion")

if __name__ == "__main__":
    sys.exit(main())
