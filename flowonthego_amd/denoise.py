"""python -m flowonthego_amd.denoise frames.npy out.npy [--radius R] [--tau T] [--occlusion] [--ref clean.npy] [--op-point K]

Denoises a video on the GPU by motion-compensated temporal filtering: frames.npy holds a (T, h, w) or (T, h, w, 3) uint8 or float32
array.  Every frame is averaged with its neighbours at distance +-1 .. +-R (default 1, at most 4), each pulled onto it along its own
flow and weighted per pixel by the photometric difference in a 3 x 3 window: a neighbour's weight reaches 0 where that difference
averages --tau (default 30) per pixel and channel (OFClass.temporal_filter).  --occlusion also computes the backward flows and leaves
out the pixels the forward-backward check finds inconsistent.  out.npy gets the filtered frames, same shape and type.  With --ref
(the clean frames, same shape and type) it prints the PSNR before and after; it always prints the mean number of neighbours used."""
import argparse
import sys


def _psnr(a, clean):
    import numpy as np
    mse = float(np.mean((a.astype(np.float64) - clean.astype(np.float64)) ** 2))
    return float("inf") if mse == 0 else 10.0 * np.log10(255.0 ** 2 / mse)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="denoise", description=__doc__.splitlines()[2])
    ap.add_argument("frames")
    ap.add_argument("out")
    ap.add_argument("--radius", type=int, default=1)
    ap.add_argument("--tau", type=float, default=30.0)
    ap.add_argument("--occlusion", action="store_true")
    ap.add_argument("--ref", default=None)
    ap.add_argument("--op-point", type=int, default=2)
    a = ap.parse_args(sys.argv[1:] if argv is None else argv)
    if not 1 <= a.radius <= 4:
        ap.error("--radius must be 1 .. 4")
    if not (a.tau > 0 and a.tau < float("inf")):
        ap.error("--tau must be a positive number")
    import numpy as np
    from ._cli import array_like_array, drop_c1, frame_sequence, load_array, refusing, sequence_context, to_device
    with refusing("denoise") as inputs:
        loaded = frame_sequence(a.frames, 1, "T", c1=True)
        ref = drop_c1(array_like_array(load_array(a.ref), a.ref, loaded, a.frames))
    if inputs.refused:
        return 1
    frames = drop_c1(loaded)
    T, h, w = frames.shape[:3]
    K = 2 * a.radius
    ofc = sequence_context(frames, a.op_point, bidir=a.occlusion, max_batch=K * min(T, 8))
    dst, used, st = ofc.temporal_filter(to_device(frames), radius=a.radius, tau=a.tau, occlusion=a.occlusion, ref=to_device(ref), stats=True)
    out = dst.cpu().numpy()
    np.save(a.out, out.reshape(loaded.shape))
    if ref is not None:
        print("PSNR before %.3f dB  after %.3f dB" % (_psnr(frames, ref), _psnr(out, ref)))
    print("mean used %.4f of %d neighbours" % (float(st[:, 0].sum().item()) / (T * h * w), K))
    ofc.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
