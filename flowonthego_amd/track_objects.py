"""python -m flowonthego_amd.track_objects frames.npy out.npz [--model translation|similarity|affine] [--iters N] [--thresh PX]
                                            [--min-area N] [--max-objects N] [--min-votes N] [--min-frac F] [--max-tracks N]
                                            [--op-point K] [--ids out.npy]

Tracks the moving objects of a video on the GPU: frames.npy holds a (T+1, h, w) or (T+1, h, w, 3) uint8 or float32 array, T >= 2.
The flows of the sequence are computed (both directions, so that occluded pixels neither fit nor vote), the camera motion is fitted
to each, the pixels that do not follow it are grouped into objects and the objects of consecutive frames are linked by the flow
(OFClass.track_objects).  out.npz gets params (T, 6), objects (T, max_objects, 11), track (T, max_objects), tracks (max_tracks, 8)
and stats (4); --ids: the track id of every pixel, int32 (T, h, w), -1 for background.  Prints one line per track:
id  frames first .. last  rows first last  mean area  largest area  votes  how it ended.

The module is callable: flowonthego_amd.track_objects(ids, objects, flows, ...) is flowonthego_amd.tracks.track_objects(...)."""
import argparse
import sys

from ._lib import callable_module


def main(argv=None):
    ap = argparse.ArgumentParser(prog="track_objects", description=__doc__.splitlines()[0])
    ap.add_argument("frames")
    ap.add_argument("out")
    ap.add_argument("--model", default="affine")
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--thresh", type=float, default=1.0)
    ap.add_argument("--min-area", type=int, default=64)
    ap.add_argument("--max-objects", type=int, default=256)
    ap.add_argument("--min-votes", type=int, default=16)
    ap.add_argument("--min-frac", type=float, default=0.25)
    ap.add_argument("--max-tracks", type=int, default=1024)
    ap.add_argument("--op-point", type=int, default=2)
    ap.add_argument("--ids", default=None)
    a = ap.parse_args(sys.argv[1:] if argv is None else argv)
    if a.iters < 0 or a.iters > 64 or not a.thresh >= 0:
        ap.error("--iters must be in 0 .. 64 and --thresh >= 0")
    if a.min_area < 1 or a.max_objects < 1 or a.max_objects > 1024:
        ap.error("--min-area must be >= 1 and --max-objects in 1 .. 1024")
    if a.min_votes < 1 or not 0 <= a.min_frac <= 1 or a.max_tracks < 1 or a.max_tracks > 65536:
        ap.error("--min-votes must be >= 1, --min-frac in 0 .. 1 and --max-tracks in 1 .. 65536")
    from .motion import MODELS                           # (imports torch: after the checks that do not need it)
    if a.model not in MODELS:
        ap.error("--model must be one of " + ", ".join(MODELS))
    import numpy as np
    from ._cli import drop_c1, frame_sequence, refusing, sequence_context, to_device
    from .tracks import ENDS
    with refusing("track_objects") as inputs:
        frames = drop_c1(frame_sequence(a.frames, 3, "T+1", c1=True))
    if inputs.refused:
        return 1
    T = frames.shape[0] - 1
    ofc = sequence_context(frames, a.op_point, bidir=True, max_batch=T)
    params, objects, track, tracks, ids, st = ofc.track_objects(
        to_device(frames), model=a.model, iters=a.iters, thresh=a.thresh, min_area=a.min_area, max_objects=a.max_objects,
        min_votes=a.min_votes, min_frac=a.min_frac, max_tracks=a.max_tracks, track_ids=True, stats=True)
    st, table = st.cpu().numpy(), tracks.cpu().numpy()
    np.savez(a.out, params=params.cpu().numpy(), objects=objects.cpu().numpy(), track=track.cpu().numpy(), tracks=table, stats=st)
    if a.ids:
        np.save(a.ids, ids.cpu().numpy())
    for k, r in enumerate(table[:int(st[1])]):
        print("%d  frames %d .. %d  rows %d %d  mean area %.1f  largest %d  votes %d  %s" % (k, r[0], r[1], r[2], r[3], r[4] / (r[1] - r[0] + 1), r[5],
                                                                                           r[6], ENDS[int(r[7])]))
    print("%d tracks over %d object maps (%d links, %d alive at the end)%s" % (st[0], T, st[2], st[3],
                                                                              "" if st[0] == st[1] else ", the first %d listed" % st[1]))
    ofc.close()
    return 0


callable_module(__name__, __package__ + ".tracks", "track_objects")

if __name__ == "__main__":
    sys.exit(main())
