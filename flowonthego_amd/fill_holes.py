"""python -m flowonthego_amd.fill_holes in.npy|in.png|in.flo out.npy|out.png|out.flo [--hole m.npy|m.png] [--fg a,b,...] [--code c.png]

The holes of a frame or a flow filled from its known pixels by pull-push on the GPU (flowonthego_amd.fill): any hole size, known
pixels kept bit for bit.  in.npy: an (h, w) or (h, w, c) array, float32 with c in 1 .. 3 or uint8 with c 1 or 3; in.png: an 8-bit
gray PNG; in.flo: a flow, whose unknown vectors (1e9) are holes without a map.  --hole: an (h, w) uint8 array or an 8-bit gray PNG,
non-zero = hole, or with --fg the listed byte values 0 .. 7 (--fg 2,3 takes the pixels a removal's code map leaves without a plate);
8-bit input needs it, in float32 a pixel that is not finite or beyond +-32768 is a hole as well.  out: .npy the array as it came,
.flo a two-channel result, .png the frame.  --code: the PNG of the code map (white known, red filled, gray nothing known).
Prints one line per image: known, filled, unfilled, depth.

The module is callable: flowonthego_amd.fill_holes(src, hole, ...) is flowonthego_amd.fill.fill_holes(src, hole, ...)."""
import argparse
import sys

from ._lib import callable_module


def main(argv=None):
    ap = argparse.ArgumentParser(prog="fill_holes", description=__doc__.splitlines()[2])
    ap.add_argument("files", nargs="+", help="in.npy|in.png|in.flo out.npy|out.png|out.flo")
    ap.add_argument("--hole", default=None)
    ap.add_argument("--fg", default=None)
    ap.add_argument("--code", default=None)
    a = ap.parse_args(sys.argv[1:] if argv is None else argv)
    if len(a.files) != 2:
        ap.error("expected in.npy|in.png|in.flo out.npy|out.png|out.flo")
    src_path, out_path = a.files
    if not src_path.endswith((".npy", ".png", ".flo")) or not out_path.endswith((".npy", ".png", ".flo")):
        ap.error("the input and the output must be .npy, .png or .flo files")
    if src_path.endswith(".png") and a.hole is None:
        ap.error("an 8-bit frame needs --hole")
    if a.hole is not None and not a.hole.endswith((".npy", ".png")):
        ap.error("--hole must be an .npy or a .png file")
    if a.code is not None and not a.code.endswith(".png"):
        ap.error("--code must be a .png file")
    if a.fg is not None and a.hole is None:
        ap.error("--fg goes with --hole")
    fg = None
    if a.fg is not None:
        try:
            fg = tuple(int(v) for v in a.fg.split(","))
        except ValueError:
            ap.error("--fg must be a list of byte values, as in 2,3")
        if not fg or any(v < 0 or v > 7 for v in fg):
            ap.error("--fg takes the byte values 0 .. 7")
    from ._cli import Refusal, load_array, load_flow, load_mask_png, refusing, to_device
    with refusing("fill_holes") as inputs:
        src = load_flow(src_path) if src_path.endswith(".flo") else load_array(src_path) if src_path.endswith(".npy") else load_mask_png(src_path)
        kind = str(src.dtype)
        if src.ndim not in (2, 3) or kind not in ("float32", "uint8") or min(src.shape[:2]) < 1 or max(src.shape[:2]) > 16384 \
                or (src.ndim == 3 and src.shape[2] not in ((1, 2, 3) if kind == "float32" else (1, 3))):
            raise Refusal("%s must hold an (h, w) or (h, w, c) array of at most 16384 rows and columns, float32 with c in 1 .. 3 or uint8 "
                          "with c 1 or 3" % src_path)
        if kind == "uint8" and a.hole is None:
            raise Refusal("%s is 8-bit: it needs --hole" % src_path)
        hole = None if a.hole is None else load_array(a.hole) if a.hole.endswith(".npy") else load_mask_png(a.hole)
        if hole is not None and (hole.shape != src.shape[:2] or str(hole.dtype) != "uint8"):
            raise Refusal("%s must hold an (h, w) uint8 array of the size of %s" % (a.hole, src_path))
        if out_path.endswith(".flo") and (kind != "float32" or src.ndim != 3 or src.shape[2] != 2):
            raise Refusal("%s: only a two-channel float32 result is written as a .flo file" % out_path)
        if out_path.endswith(".png") and src.ndim == 3 and src.shape[2] == 2:
            raise Refusal("%s: a two-channel result is no picture" % out_path)
    if inputs.refused:
        return 1
    import numpy as np
    from . import fill
    from ._cli import save_code_png, save_frame_png
    h, w = src.shape[:2]
    s = to_device(src if src.ndim == 3 else src[..., None])
    dst, code, stats = fill.fill_holes(s, to_device(hole), fg=fg, dst=True, code=True, stats=True)
    out = dst.cpu().numpy().reshape(src.shape)
    if out_path.endswith(".npy"):
        np.save(out_path, out)
    elif out_path.endswith(".flo"):
        from .flo import write_flo
        write_flo(out_path, out)
    else:
        save_frame_png(out_path, out, h, w)
    if a.code is not None:
        save_code_png(a.code, code)
    for k, row in enumerate(stats.cpu().numpy().reshape(-1, 4)):
        print("image %d of %d x %d: %d known, %d filled, %d unfilled, depth %d" % (k, w, h, row[0], row[1], row[2], row[3]))
    return 0


callable_module(__name__, __package__ + ".fill", "fill_holes")

if __name__ == "__main__":
    sys.exit(main())
