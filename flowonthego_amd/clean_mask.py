"""python -m flowonthego_amd.clean_mask in.npy|in.png out.png [--open R] [--close R] [--fg a,b,...] [--op OP --radius R]

A mask or a code map cleaned by binary morphology on the GPU (flowonthego_amd.morph): an opening by a disc of radius --open deletes
the speckle the disc does not fit into, a closing by a disc of radius --close then fills the pin-holes and gaps (defaults 1 and 2,
each 0 .. 8, 0 = leave that part out).  in.npy: an (h, w) uint8 array; in.png: an 8-bit gray PNG.  A pixel is set if its byte is
non-zero, or with --fg if it is one of the listed byte values 0 .. 7 (--fg 1,4 takes the foreground of a background subtraction's
code map as it is).  --op erode | dilate | open | close with --radius R runs that one operation instead.  out.png: the result,
set pixels white.  Prints the set pixels before and after and the pixels added and removed.

The module is callable: flowonthego_amd.clean_mask(mask, open=1, close=2, ...) is flowonthego_amd.morph.clean_mask(mask, ...)."""
import argparse
import sys

from ._lib import callable_module

OPS = ("erode", "dilate", "open", "close")


def main(argv=None):
    ap = argparse.ArgumentParser(prog="clean_mask", description=__doc__.splitlines()[2])
    ap.add_argument("files", nargs="+", help="in.npy|in.png out.png")
    ap.add_argument("--open", type=int, default=None)
    ap.add_argument("--close", type=int, default=None)
    ap.add_argument("--fg", default=None)
    ap.add_argument("--op", default=None)
    ap.add_argument("--radius", type=int, default=None)
    a = ap.parse_args(sys.argv[1:] if argv is None else argv)
    if len(a.files) != 2:
        ap.error("expected in.npy|in.png out.png")
    if (a.op is None) != (a.radius is None):
        ap.error("--op and --radius go together")
    if a.op is not None and (a.open is not None or a.close is not None):
        ap.error("--op stands instead of --open and --close")
    if a.op is not None and a.op not in OPS:
        ap.error("--op must be one of %s" % ", ".join(OPS))
    rad = dict(radius=a.radius) if a.op is not None else dict(open=1 if a.open is None else a.open, close=2 if a.close is None else a.close)
    for name, r in rad.items():
        if not 0 <= r <= 8:
            ap.error("--%s must lie in 0 .. 8" % name)
    fg = None
    if a.fg is not None:
        try:
            fg = tuple(int(v) for v in a.fg.split(","))
        except ValueError:
            ap.error("--fg must be a list of byte values, as in 1,4")
        if not fg or any(v < 0 or v > 7 for v in fg):
            ap.error("--fg takes the byte values 0 .. 7")
    from ._cli import Refusal, load_array, load_mask_png, refusing, to_device
    with refusing("clean_mask") as inputs:
        path = a.files[0]
        mask = load_array(path) if path.endswith(".npy") else load_mask_png(path)
        if mask.ndim != 2 or str(mask.dtype) != "uint8" or min(mask.shape) < 1 or max(mask.shape) > 16384:
            raise Refusal("%s must hold an (h, w) uint8 array of at most 16384 rows and columns" % path)
    if inputs.refused:
        return 1
    import numpy as np
    from ._png import write_png
    from . import morph
    if a.op is not None:
        out, stats = morph.morphology(to_device(mask), a.op, a.radius, fg=fg, stats=True)
        rows = [(a.op, a.radius, stats.cpu().numpy())]
    else:
        out, stats = morph.clean_mask(to_device(mask), open=rad["open"], close=rad["close"], fg=fg, stats=True)
        stats = stats.cpu().numpy()
        rows = [("open", rad["open"], stats[0]), ("close", rad["close"], stats[1])]
    out = out.cpu().numpy()
    h, w = out.shape
    write_png(a.files[1], np.ascontiguousarray(np.broadcast_to((out * np.uint8(255))[..., None], (h, w, 3))))
    print("mask of %d x %d:" % (w, h))
    for name, r, s in rows:
        print("  %s by radius %d: %d set pixels before, %d after, %d added, %d removed" % (name, r, s[0], s[1], s[2], s[3]))
    return 0


callable_module(__name__, __package__ + ".morph", "clean_mask")

if __name__ == "__main__":
    sys.exit(main())
