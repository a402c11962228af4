"""python -m flowonthego_amd.fb_check fw.flo bw.flo out.png [--alpha1 A1] [--alpha2 A2]

Forward-backward consistency of two .flo files on the GPU (flowonthego_amd.consistency): fw.flo holds the flow frame 0 -> 1,
bw.flo the flow frame 1 -> 0.  Writes the mask of frame 0 as a PNG (code 0 consistent white, 1 occluded red, 2 outside the
frame blue, 3 unknown black) and prints the fraction of frame 0's pixels of each code."""
import argparse
import sys


def main(argv=None):
    ap = argparse.ArgumentParser(prog="fb_check", description=__doc__.splitlines()[0])
    ap.add_argument("fw")
    ap.add_argument("bw")
    ap.add_argument("out")
    ap.add_argument("--alpha1", type=float, default=0.01)
    ap.add_argument("--alpha2", type=float, default=0.5)
    a = ap.parse_args(sys.argv[1:] if argv is None else argv)
    from ._cli import flow_like_flow, load_flow, refusing, to_device
    from ._png import write_png
    from .consistency import CODES, fb_check, mask_to_rgb
    with refusing("fb_check") as inputs:
        fw = load_flow(a.fw)
        bw = flow_like_flow(load_flow(a.bw), a.bw, fw, a.fw)
    if inputs.refused:
        return 1
    mask, _, cnt = fb_check(to_device(fw), to_device(bw), a.alpha1, a.alpha2, stats=True)
    cnt = cnt.cpu().numpy()[0]
    npix = fw.shape[0] * fw.shape[1]
    print("  ".join("%s %.4f" % (nm, float(c) / npix) for nm, c in zip(CODES, cnt)))
    write_png(a.out, mask_to_rgb(mask))
    return 0


if __name__ == "__main__":
    sys.exit(main())
