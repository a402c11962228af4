"""python -m flowonthego_amd.interp_frame f0.npy f1.npy t out.png [--ref mid.npy] [--op N]

Writes the frame at time t (0 < t < 1) between two frames: both flows from one bidirectional call at operating point N (default
2), the consistency check and the interpolation on the GPU (OFClass.interpolate).  f0.npy, f1.npy: (h, w) arrays, uint8 or
float32 (gray).  Prints
from_forward from_backward holes one_sided (fractions of the pixels) and, with --ref (the true frame at t), mad_interpolated
mad_blend (mean |ref - frame| and mean |ref - ((1 - t) f0 + t f1)| over all pixels)."""
import argparse
import sys


def main(argv=None):
    ap = argparse.ArgumentParser(prog="interp_frame", description=__doc__.splitlines()[0])
    ap.add_argument("f0")
    ap.add_argument("f1")
    ap.add_argument("t", type=float)
    ap.add_argument("out")
    ap.add_argument("--ref", default=None)
    ap.add_argument("--op", type=int, default=2)
    a = ap.parse_args(sys.argv[1:] if argv is None else argv)
    if not 0.0 < a.t < 1.0:
        ap.error("t must lie strictly between 0 and 1")
    from . import img_params, operating_point
    from ._cli import Refusal, array_like_array, load_array, refusing, save_frame_png, to_device
    from .interp import STATS
    from .oflow import OFClass
    with refusing("interp_frame") as inputs:
        f0 = load_array(a.f0)
        if f0.ndim != 2 or str(f0.dtype) not in ("uint8", "float32"):
            raise Refusal("%s must hold an (h, w) uint8 or float32 array" % a.f0)
        f1 = array_like_array(load_array(a.f1), a.f1, f0, a.f0)
        ref = array_like_array(load_array(a.ref), a.ref, f0, a.f0)
    if inputs.refused:
        return 1
    h, w = f0.shape
    op = operating_point(a.op, w, 1)
    op.bidir = True
    ofc = OFClass(op, img_params(width=w, height=h))
    dst, _, st = ofc.interpolate(to_device(f0), to_device(f1), a.t, ref=to_device(ref), stats=True)
    st = st.cpu().numpy()
    line = "  ".join("%s %.4f" % (nm, c / (h * w)) for nm, c in zip(STATS[:4], st[:4]))
    if ref is not None:
        line += "  mad_interpolated %.4f  mad_blend %.4f" % (st[4] / (h * w), st[5] / (h * w))
    print(line)
    save_frame_png(a.out, dst, h, w)
    ofc.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
