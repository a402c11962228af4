#!/usr/bin/env python3
"""Records tests/golden/kroeger_ref_live.npz: the input and output digests of every call tests/test_kroeger_pin.py makes into the
reference's own LK code (oracle/_ref/libkroeger_*.so, built by `make -C oracle ref` where the reference tree exists).  Runs those
tests with the live build and stores what they recorded; the tests replay the digests where oracle/_ref cannot be built.

    python tests/golden/make_kroeger_golden.py
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    from oracle import kroeger_ref as K
    assert all(K.available(d, c) for d in (0, 1) for c in (1, 3)), "build oracle/_ref first (make -C oracle ref)"
    import test_kroeger_pin as T
    path = T.KroegerCalls.PATH
    if os.path.exists(path):
        os.remove(path)                       # record afresh: the live build must not be checked against an older file
    T.KREF.stored = None
    rc = pytest.main(["-q", "-p", "no:cacheprovider", os.path.join(ROOT, "tests", "test_kroeger_pin.py")])
    assert rc == 0, "the pin tests must pass before their outputs are recorded"
    T.KREF.save(path)
    print("wrote %s: %d entries, %d bytes" % (path, len(T.KREF.recorded), os.path.getsize(path)))


if __name__ == "__main__":
    main()
