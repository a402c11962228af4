"""Writes tests/golden/alley_1_more.npz: frames 0003, 0020, 0021 and 0022 of the reference's images/alley_1 as 8-bit gray, with
make_golden.py's gray_cv (frames 0001 and 0002 are in alley_1_gray.npz) -- the triplets (1, 2, 3) and (20, 21, 22) of the frame
interpolation's quality check (tests/test_interp.py, tests/test_gpu_interp.py).  The conversion is integer valued: 8-bit storage
loses nothing.  The archive is an .npz whose members are bzip2-compressed (numpy.load reads it like any other): deflate, what
numpy.savez_compressed writes, leaves the four frames above 1 MiB.

    python tests/golden/make_interp_golden.py"""
import io
import os
import zipfile

import numpy as np

from make_golden import OUT, REF, gray_cv, rgb

FRAMES = (3, 20, 21, 22)


def main():
    path = os.path.join(OUT, "alley_1_more.npz")
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_BZIP2) as zf:
        for k in FRAMES:
            buf = io.BytesIO()
            np.save(buf, gray_cv(rgb(REF + "/images/alley_1/frame_%04d.png" % k)))
            zf.writestr("frame_%04d.npy" % k, buf.getvalue())
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
