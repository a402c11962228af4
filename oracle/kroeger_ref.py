"""ctypes driver of oracle/_ref/libkroeger_{of,de}_{gray,rgb}.so -- the reference's OWN LK / densification / scale-loop code
(kroeger/{oflow,patch,patchgrid,refine_variational}.cpp + FDF1.0.1) compiled unmodified by `make -C oracle ref` against the
project-written minimal Eigen headers oracle/eigen_min/, with oracle/kroeger_drv.cpp as the entry point.

TEST INFRASTRUCTURE ONLY.  Used to pin oracle/dis_oracle.c's LK half bit for bit (tests/test_kroeger_pin.py) and to record the
stored outputs tests/golden/kroeger_ref_live.npz (tests/golden/make_kroeger_golden.py) for machines without the build.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from . import oracle as O

_HERE = os.path.dirname(os.path.abspath(__file__))
f32p = C.POINTER(C.c_float)
_LIBS = {}


def _name(depth, noc):
    return "libkroeger_%s_%s.so" % ("de" if depth else "of", "gray" if noc == 1 else "rgb")


def available(depth=0, noc=1):
    return os.path.exists(os.path.join(_HERE, "_ref", _name(depth, noc)))


def lib(depth=0, noc=1):
    key = (int(bool(depth)), int(noc))
    if key not in _LIBS:
        L = C.CDLL(os.path.join(_HERE, "_ref", _name(*key)))
        L.kroeger_flow_pyr.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(O.DisParams), f32p, f32p, f32p]
        assert L.kroeger_build_mode() == (20 if depth else 10) + noc
        _LIBS[key] = L
    return _LIBS[key]


def flow_pyr(P0, P1, params, dump=False, initflow=None):
    """OFClass on the oracle's pyramids (O.Pyramid) -> finest-level flow (h_l, w_l, nch) [+ {level: (pre, post)}], the layout of
    O.flow_pyr.  pre is None where the driver cannot reproduce it (usefbcon and usetvref both on, see kroeger_drv.cpp)."""
    L = lib(params.depth, params.noc)
    w, h = P0.level_wh(params.sc_l)
    nch = 1 if params.depth else 2
    out = np.zeros((h, w, nch), np.float32)
    fi = O.f32(initflow) if initflow is not None else None
    d = None
    if dump:
        d = np.zeros(sum(2 * nch * (P0.w0 >> l) * (P0.h0 >> l) for l in range(params.sc_l, params.sc_f + 1)), np.float32)
    rc = L.kroeger_flow_pyr(C.cast(P0.ptr, C.c_void_p), C.cast(P1.ptr, C.c_void_p), C.byref(params),
                            O.P(fi) if fi is not None else None, O.P(out), O.P(d) if dump else None)
    assert rc == 0, "parameters do not match the kroeger build (depth / noc / normoutlier)"
    if not dump:
        return out
    lv, off = {}, 0
    for l in range(params.sc_f, params.sc_l - 1, -1):
        n = nch * (P0.w0 >> l) * (P0.h0 >> l)
        shp = (P0.h0 >> l, P0.w0 >> l, nch)
        pre = d[off:off + n].reshape(shp).copy()
        lv[l] = (None if np.isnan(pre).all() else pre, d[off + n:off + 2 * n].reshape(shp).copy())
        off += 2 * n
    return out, lv


def eigen_lib():
    """oracle/libeigen_min_test.so: the eigen_min operations on caller data (built from this project's sources alone)"""
    if "eigen_min" not in _LIBS:
        so = os.path.join(_HERE, "libeigen_min_test.so")
        if not os.path.exists(so):
            subprocess.check_call(["make", "-C", _HERE, "libeigen_min_test.so"], stdout=subprocess.DEVNULL)
        L = C.CDLL(so)
        L.kroeger_eigen_redux.argtypes = [f32p, f32p, C.c_int, f32p]
        L.kroeger_eigen_fixed.argtypes = [f32p, f32p, f32p]
        L.kroeger_eigen_llt.argtypes = [C.c_int, f32p, f32p, f32p, f32p]
        _LIBS["eigen_min"] = L
    return _LIBS["eigen_min"]


def eigen_redux(v, w):
    """(v.sum(), (v.array() * w.array()).sum(), v.lpNorm<1>()) of eigen_min's dynamic vector"""
    v, w = O.f32(v), O.f32(w)
    out = np.zeros(3, np.float32)
    eigen_lib().kroeger_eigen_redux(O.P(v), O.P(w), v.size, O.P(out))
    return out


def eigen_fixed(u, H):
    """(u.squaredNorm(), u.norm(), H.determinant()) for a Vector2f u and a 2x2 H"""
    u, H = O.f32(u), O.f32(H)
    out = np.zeros(3, np.float32)
    eigen_lib().kroeger_eigen_fixed(O.P(u), O.P(H), O.P(out))
    return out


def eigen_llt(H, b):
    """H.llt() and .solve(b) for a 1x1 or 2x2 H -> (factor matrix as stored, x, index where the factorisation stopped or -1)"""
    H, b = O.f32(H), O.f32(b)
    n = H.shape[0]
    l = np.zeros((n, n), np.float32)
    x = np.zeros(n, np.float32)
    k = eigen_lib().kroeger_eigen_llt(n, O.P(H), O.P(b), O.P(l), O.P(x))
    return l, x, k
