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
    from ._cli import array_like_array, frame_like_flow, load_array, load_flow, mask_like_flow, refusing, save_frame_png, to_device
    from .warp import STATS, warp
    with refusing("warp_frame") as inputs:
        flow = load_flow(a.flow)
        h, w = flow.shape[:2]
        f0 = frame_like_flow(load_array(a.f0), a.f0, h, w)
        f1 = array_like_array(frame_like_flow(load_array(a.f1), a.f1, h, w), a.f1, f0, a.f0)
        occ = mask_like_flow(load_array(a.occ), a.occ, h, w)
    if inputs.refused:
        return 1
    dst, _, st = warp(to_device(f1), to_device(flow), ref=to_device(f0), occ=to_device(occ), fill=a.fill, stats=True)
    st = st.cpu().numpy()
    terms = max(st[0], 1.0) * (3 if f0.shape[2:] == (3,) else 1)
    print("  ".join("%s %.4f" % (nm, c / (h * w)) for nm, c in zip(STATS[:4], st[:4])) +
          "  mad_warped %.4f  mad_unwarped %.4f" % (st[4] / terms, st[5] / terms))
    save_frame_png(a.out, dst, h, w)
    return 0


if __name__ == "__main__":
    sys.exit(main())
