"""python -m flowonthego_amd.warp_frame f0.npy f1.npy flow.flo out.png [--occ mask.npy] [--fill V]

Pulls frame 1 back onto frame 0's grid along flow.flo (the flow frame 0 -> 1) on the GPU (flowonthego_amd.warp).  f0.npy, f1.npy:
(h, w) or (h, w, 3) arrays, uint8 or float32; mask.npy: (h, w) uint8 codes of fb_check.  Writes the warped frame as a PNG (with
--fill V every pixel that is not valid gets V, otherwise the reference's clamped taps) and prints
valid occluded outside unknown (fractions of the pixels) mad_warped mad_unwarped (mean |f0 - warp(f1)| and mean |f0 - f1| over the
valid pixels and all channels)."""
import argparse
import sys


def main(argv=None):
    ap = argparse.ArgumentParser(prog="warp_frame", description=__doc__.splitlines()[0])
    ap.add_argument("f0")
    ap.add_argument("f1")
    ap.add_argument("flow")
    ap.add_argument("out")
    ap.add_argument("--occ", default=None)
    ap.add_argument("--fill", type=float, default=None)
    a = ap.parse_args(sys.argv[1:] if argv is None else argv)
    import numpy as np
    import torch
    from .color import write_png
    from .flo import read_flo
    from .warp import STATS, warp
    try:
        f0, f1, flow = np.load(a.f0), np.load(a.f1), read_flo(a.flow)
        occ = np.load(a.occ) if a.occ else None
    except (OSError, ValueError) as e:
        sys.stderr.write("warp_frame: %s\n" % e)
        return 1
    h, w = flow.shape[:2]
    if f0.shape != f1.shape or f0.dtype != f1.dtype or f0.dtype not in (np.uint8, np.float32) or f0.shape[:2] != (h, w) \
            or f0.shape[2:] not in ((), (1,), (3,)) or (occ is not None and (occ.shape != (h, w) or occ.dtype != np.uint8)):
        sys.stderr.write("warp_frame: the frames must be two alike (%d, %d[, 3]) uint8 or float32 arrays (the flow's size), "
                         "the mask (%d, %d) uint8\n" % (h, w, h, w))
        return 1
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    dst, _, st = warp(dev(f1), dev(flow), ref=dev(f0), occ=None if occ is None else dev(occ), fill=a.fill, stats=True)
    st = st.cpu().numpy()
    terms = max(st[0], 1.0) * (3 if f0.shape[2:] == (3,) else 1)
    print("  ".join("%s %.4f" % (nm, c / (h * w)) for nm, c in zip(STATS[:4], st[:4])) +
          "  mad_warped %.4f  mad_unwarped %.4f" % (st[4] / terms, st[5] / terms))
    img = dst.cpu().numpy().reshape(h, w, -1)
    if img.dtype != np.uint8:
        img = np.clip(np.rint(np.nan_to_num(img)), 0, 255).astype(np.uint8)
    write_png(a.out, np.ascontiguousarray(np.broadcast_to(img, (h, w, 3))))
    return 0


if __name__ == "__main__":
    sys.exit(main())
