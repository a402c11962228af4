"""python -m flowonthego_amd.moving_objects flow.flo [--mask m.png] [--model translation|similarity|affine] [--iters N] [--thresh PX]
                                             [--min-area N] [--max-objects N] [--connectivity 4|8] [--ids out.png]

Fits the camera motion that explains flow.flo on the GPU, groups the pixels that do not follow it into objects
(flowonthego_amd.objects.moving_objects) and prints a00 a01 tx a10 a11 ty, then one line per object:
xmin ymin xmax ymax  area  centroid x y  mean motion u v (pixels, relative to the camera).
--mask: an 8-bit gray PNG of the flow's size, 0 = the pixel takes part in the fit (the mask of python -m flowonthego_amd.fb_check);
--ids: the objects as a PNG, a colour per object, background black.

The module is callable: flowonthego_amd.moving_objects(flow, ...) is flowonthego_amd.objects.moving_objects(flow, ...)."""
import argparse
import sys

from ._lib import callable_module


def main(argv=None):
    from .motion import MODELS
    ap = argparse.ArgumentParser(prog="moving_objects", description=__doc__.splitlines()[0])
    ap.add_argument("flow")
    ap.add_argument("--mask", default=None)
    ap.add_argument("--model", default="affine", choices=MODELS)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--thresh", type=float, default=1.0)
    ap.add_argument("--min-area", type=int, default=64)
    ap.add_argument("--max-objects", type=int, default=256)
    ap.add_argument("--connectivity", type=int, default=8, choices=(4, 8))
    ap.add_argument("--ids", default=None)
    a = ap.parse_args(sys.argv[1:] if argv is None else argv)
    if a.iters < 0 or a.iters > 64 or not a.thresh >= 0:
        ap.error("--iters must be in 0 .. 64 and --thresh >= 0")
    if a.min_area < 1 or a.max_objects < 1 or a.max_objects > 65536:
        ap.error("--min-area must be >= 1 and --max-objects in 1 .. 65536")
    import numpy as np
    from ._cli import load_flow, load_mask_png, mask_like_flow, refusing, save_code_png, to_device
    from .objects import moving_objects, object_summary
    with refusing("moving_objects") as inputs:
        flow = load_flow(a.flow)
        h, w = flow.shape[:2]
        mask = mask_like_flow(load_mask_png(a.mask), a.mask, h, w)
    if inputs.refused:
        return 1
    params, objects, ids, st = moving_objects(to_device(flow), to_device(mask), a.model, a.iters, a.thresh, a.min_area, a.max_objects,
                                              a.connectivity, ids=True, stats=True)
    st = st.cpu().numpy()
    print(" ".join("%.9g" % v for v in params.cpu().numpy()))
    rows = objects[:int(st[3])]
    for o, s in zip(rows.cpu().numpy(), object_summary(rows).cpu().numpy()):
        print("%d %d %d %d  area %d  centroid %.2f %.2f  motion %.3f %.3f" % (o[2], o[3], o[4], o[5], o[1], s[0], s[1], s[2], s[3]))
    print("%d objects of at least %d pixels (%d components, %d pixels)%s" % (st[2], a.min_area, st[1], st[0],
                                                                             "" if st[2] == st[3] else ", the first %d listed" % st[3]))
    if a.ids:
        pal = np.zeros((a.max_objects + 1, 3), np.uint8)
        j = np.arange(1, a.max_objects + 1)
        pal[1:] = np.stack([64 + (j * 97) % 192, 64 + (j * 57) % 192, 64 + (j * 151) % 192], -1)
        save_code_png(a.ids, ids + 1, pal)
    return 0


callable_module(__name__, __package__ + ".objects", "moving_objects")

if __name__ == "__main__":
    sys.exit(main())
