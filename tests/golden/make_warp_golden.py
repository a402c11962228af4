#!/usr/bin/env python3
"""Generates tests/golden/image_warp_ref.npz: the outputs of the reference's OWN image_warp (kroeger/FDF1.0.1/opticalflow_aux.c:18-60,
compiled unmodified into oracle/_ref/libfdf_ref_{gray,rgb}.so and driven through oracle/fdf_ref.py) on the inputs of
tests/warp_ref.py cases().  Runs only where oracle/_ref has been built; the fixture is plain data.

The inputs are made again from their seeds by the tests, so only outputs are stored, per case <name>:
  <name>/dst     every ROW_STEP-th row of the warped image, (rows, w) or (rows, w, 3) float32 (ROW_STEP = 1 below 64 rows, 16 from there)
  <name>/mask    the whole mask, (h, w) uint8
  <name>/sha     sha256 of the whole dst (C order float32 bytes), as 32 uint8
"""
import hashlib
import os
import sys

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(OUT))


def row_step(h):
    return 1 if h < 64 else 16


def digest(dst):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(dst, np.float32).tobytes()).digest(), np.uint8)


def live_image_warp(refs, img, flow):
    """the reference's image_warp on an (h, w) or (h, w, 3) image: (dst of img's shape, mask (h, w) float32)"""
    noc = 1 if img.ndim == 2 else 3
    R = refs[noc]
    h, w = flow.shape[:2]
    planar = np.ascontiguousarray(img[None] if noc == 1 else img.transpose(2, 0, 1), np.float32)
    I2 = R.from_planar(planar)
    WX, WY = R.from_plane(np.ascontiguousarray(flow[..., 0])), R.from_plane(np.ascontiguousarray(flow[..., 1]))
    w2, mask = R.newc(w, h), R.new(w, h)
    R.L.image_warp(w2, mask, I2, WX, WY)
    d = R.viewc(w2)[:, :, :w].copy()
    m = R.view(mask)[:, :w].copy()
    R.free(I2, WX, WY, w2, mask)
    return (d[0] if noc == 1 else np.ascontiguousarray(d.transpose(1, 2, 0))), m


def live_refs():
    from oracle import fdf_ref
    if not (fdf_ref.available(1) and fdf_ref.available(3)):
        return None
    return {1: fdf_ref.FdfRef(1), 3: fdf_ref.FdfRef(3)}


def main():
    import warp_ref as W
    refs = live_refs()
    if refs is None:
        sys.exit("make_warp_golden.py: oracle/_ref is not built (make -C oracle ref, where the reference tree exists)")
    rec = {}
    for name, noc, h, w, kind, seed in W.cases():
        img, flow = W.case_image(h, w, noc, seed), W.case_flow(kind, h, w, seed)
        dst, mask = live_image_warp(refs, img, flow)
        assert set(np.unique(mask)) <= {0.0, 1.0}
        rec[name + "/dst"] = dst[::row_step(h)]
        rec[name + "/mask"] = mask.astype(np.uint8)
        rec[name + "/sha"] = digest(dst)
    path = os.path.join(OUT, "image_warp_ref.npz")
    np.savez_compressed(path, **rec)
    print("wrote %s (%d bytes, %d cases)" % (path, os.path.getsize(path), len(W.cases())))


if __name__ == "__main__":
    main()
