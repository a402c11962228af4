"""python -m flowonthego_amd.fit_motion flow.flo [--mask m.png] [--model translation|similarity|affine] [--iters N] [--thresh PX]
                                        [--code out.png]

Fits the camera motion that explains flow.flo on the GPU (flowonthego_amd.motion.fit_motion) and prints
a00 a01 tx a10 a11 ty, then the shares of the pixels that follow it, move on their own, are masked or unknown.
--mask: an 8-bit gray PNG of the flow's size, 0 = the pixel takes part (the mask of python -m flowonthego_amd.fb_check);
--code: the per-pixel code as a PNG (follows: white, independent: red, masked: gray, unknown: black).

The module is callable: flowonthego_amd.fit_motion(flow, ...) is flowonthego_amd.motion.fit_motion(flow, ...)."""
import argparse
import struct
import sys
import zlib

from ._lib import callable_module

CODE_RGB = ((255, 255, 255), (220, 30, 30), (128, 128, 128), (0, 0, 0))


def read_gray_png(path):
    """an 8-bit gray, non-interlaced PNG -> (h, w) uint8 (zlib + struct only)"""
    import numpy as np
    data = open(path, "rb").read()
    if data[:8] != b"\x89PNG\r\n\x1a\n":
        raise ValueError("%s is not a PNG file" % path)
    pos, idat, head = 8, b"", None
    while pos + 8 <= len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        pos += 12 + n
        if tag == b"IHDR":
            head = struct.unpack(">IIBBBBB", body)
        elif tag == b"IDAT":
            idat += body
        elif tag == b"IEND":
            break
    if head is None or head[2:] != (8, 0, 0, 0, 0):
        raise ValueError("%s must be an 8-bit gray PNG without interlacing" % path)
    w, h = head[:2]
    raw = np.frombuffer(zlib.decompress(idat), np.uint8)
    if raw.size != h * (w + 1):
        raise ValueError("%s is truncated" % path)
    rows = raw.reshape(h, w + 1)
    out = np.zeros((h, w), np.uint8)
    prev = np.zeros(w, np.int32)
    for y in range(h):
        ft, line = int(rows[y, 0]), rows[y, 1:].astype(np.int32)
        if ft == 0:
            cur = line
        elif ft == 2:
            cur = (line + prev) & 255
        elif ft in (1, 3, 4):                   # the filters that look to the left: byte by byte
            cur = np.zeros(w, np.int32)
            for x in range(w):
                a, b, c = (cur[x - 1] if x else 0), prev[x], (prev[x - 1] if x else 0)
                if ft == 1:
                    p = a
                elif ft == 3:
                    p = (a + b) // 2
                else:
                    pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
                    p = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
                cur[x] = (line[x] + p) & 255
        else:
            raise ValueError("%s: bad filter type %d" % (path, ft))
        out[y] = cur
        prev = cur
    return out


def main(argv=None):
    from .motion import MODELS
    ap = argparse.ArgumentParser(prog="fit_motion", description=__doc__.splitlines()[0])
    ap.add_argument("flow")
    ap.add_argument("--mask", default=None)
    ap.add_argument("--model", default="affine", choices=MODELS)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--thresh", type=float, default=1.0)
    ap.add_argument("--code", default=None)
    a = ap.parse_args(sys.argv[1:] if argv is None else argv)
    if a.iters < 0 or a.iters > 64 or not a.thresh >= 0:
        ap.error("--iters must be in 0 .. 64 and --thresh >= 0")
    import numpy as np
    import torch
    from .color import write_png
    from .flo import read_flo
    from .motion import CODES, fit_motion
    try:
        flow = read_flo(a.flow)
        mask = read_gray_png(a.mask) if a.mask else None
    except (OSError, ValueError, zlib.error) as e:
        sys.stderr.write("fit_motion: %s\n" % e)
        return 1
    h, w = flow.shape[:2]
    if mask is not None and mask.shape != (h, w):
        sys.stderr.write("fit_motion: %s is %d x %d, the flow %d x %d\n" % (a.mask, mask.shape[1], mask.shape[0], w, h))
        return 1
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    params, code, st = fit_motion(dev(flow), None if mask is None else dev(mask), a.model, a.iters, a.thresh, code=True, stats=True)
    st = st.cpu().numpy()
    print(" ".join("%.9g" % v for v in params.cpu().numpy()))
    print("  ".join("%s %.4f" % (nm, c / (h * w)) for nm, c in zip(CODES, st[:4])) + ("" if st[5] else "  (not fitted)"))
    if a.code:
        write_png(a.code, np.array(CODE_RGB, np.uint8)[code.cpu().numpy()])
    return 0


callable_module(__name__, __package__ + ".motion", "fit_motion")

if __name__ == "__main__":
    sys.exit(main())
