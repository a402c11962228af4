#!/usr/bin/env python3
"""Generates tests/golden/colorcode_ref.npz: inputs and outputs of the reference's OWN Middlebury colour code.  Runs only where the
reference tree exists; the fixture is plain data.

The reference's flow_code/C/color_flow.cpp (its main renamed), colorcode.cpp, flowIO.cpp and imageLib/{Image,RefCntMem,ImageIO,
Convert}.cpp are compiled with g++ into a temporary directory, together with a small driver (written below) that stubs the PNG
reader / writer (libpng is not needed: nothing is written) and captures the values MotionToColor prints.  Recorded:

  cc_named_{in,out,kind}   computeColor(fx, fy) of the named vectors: axis-aligned vectors with +-0 components and |v| == 1 (kind 1),
                           the 55 wheel boundaries at three radii and their f32 neighbours (kind 2: where a 1-ulp difference of the
                           angle moves k0, so where the atan2 deviation shows).  Outputs are R, G, B (the reference's CByteImage holds
                           B, G, R; its PNG writer swaps).
  cc_grid_out              computeColor of the 160 000 vectors of tests/colorcode_ref.py grid_vectors() (integer arithmetic, so the
                           inputs are made again by the tests rather than stored)
  field/<name>             the small stored flow fields (the alley field is the existing fixture alley_0001_flo.npz)
  mtc/<run>/{field,maxmotion,rows,rgb,stats}
                           MotionToColor of a field; rgb keeps every rows-th row (the alley runs: every 8th / 16th row) to keep the
                           file small; stats = the five values it prints (maxrad, minu, maxu, minv, maxv).  mtc_runs: the run names.
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

REF = os.environ.get("FOTG_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))

DRIVER = r'''
#include <stdarg.h>
#include "imageLib.h"
#include "colorcode.h"
void ReadFilePNG(CByteImage &, const char *) { throw CError("no PNG support in this driver"); }
void WriteFilePNG(CByteImage, const char *) { throw CError("no PNG support in this driver"); }
double g_printed[5];
extern "C" int capture_printf(const char *, ...);
int capture_printf(const char *fmt, ...)
{
  va_list ap; va_start(ap, fmt);
  for (int i = 0; i < 5; ++i) g_printed[i] = va_arg(ap, double);
  va_end(ap);
  return 0;
}
extern int verbose;
void MotionToColor(CFloatImage motim, CByteImage &colim, float maxmotion);
extern "C" void cc_batch(int n, const float *xy, unsigned char *rgb)
{
  for (int i = 0; i < n; ++i) {
    unsigned char bgr[3];
    computeColor(xy[2 * i], xy[2 * i + 1], bgr);
    rgb[3 * i] = bgr[2]; rgb[3 * i + 1] = bgr[1]; rgb[3 * i + 2] = bgr[0];
  }
}
extern "C" void mtc(int w, int h, const float *flow, float maxmotion, unsigned char *rgb, double *printed)
{
  verbose = 0;
  CFloatImage im(CShape(w, h, 2));
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x)
      for (int b = 0; b < 2; ++b) im.Pixel(x, y, b) = flow[((size_t)y * w + x) * 2 + b];
  CByteImage out(CShape(w, h, 3));
  MotionToColor(im, out, maxmotion);
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x)
      for (int b = 0; b < 3; ++b) rgb[((size_t)y * w + x) * 3 + b] = out.Pixel(x, y, 2 - b);
  for (int i = 0; i < 5; ++i) printed[i] = g_printed[i];
}
'''


def build(tmp):
    src = os.path.join(REF, "flow_code", "C")
    lib = os.path.join(src, "imageLib")
    drv = os.path.join(tmp, "driver.cpp")
    with open(drv, "w") as f:
        f.write(DRIVER)
    objs = []
    units = [(os.path.join(src, "color_flow.cpp"), ["-Dmain=color_flow_main", "-include", os.path.join(tmp, "decl.h")])]
    with open(os.path.join(tmp, "decl.h"), "w") as f:
        f.write('#include <stdio.h>\n#include <cstdio>\nextern "C" int capture_printf(const char *, ...);\n#define printf capture_printf\n')
    units += [(os.path.join(src, s), []) for s in ("colorcode.cpp", "flowIO.cpp")]
    units += [(os.path.join(lib, s), []) for s in ("Image.cpp", "RefCntMem.cpp", "ImageIO.cpp", "Convert.cpp")]
    units += [(drv, [])]
    for i, (cpp, extra) in enumerate(units):
        o = os.path.join(tmp, "u%d.o" % i)
        subprocess.check_call(["g++", "-O3", "-fPIC", "-w", "-fpermissive", "-I", src, "-I", lib] + extra + ["-c", cpp, "-o", o])
        objs.append(o)
    so = os.path.join(tmp, "libcolorref.so")
    subprocess.check_call(["g++", "-shared", "-o", so] + objs)
    L = C.CDLL(so)
    L.cc_batch.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    L.mtc.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]
    return L


def named_vectors():
    """(named edge cases, wheel boundaries), both (k, 2) float32"""
    f32 = np.float32
    edge = []
    for a in (0.0, -0.0):
        for b in (0.0, -0.0):
            edge.append((a, b))
    for v in (1.0, 0.5, 2.0, 1e-30, 1e-45, 7.0):
        for s in (1.0, -1.0):
            for z in (0.0, -0.0):
                edge += [(s * v, z), (z, s * v)]
    edge += [(0.6, 0.8), (-0.6, 0.8), (0.8, -0.6), (-0.8, -0.6), (f32(1) / f32(np.sqrt(2)), f32(1) / f32(np.sqrt(2)))]
    bound = []
    for k in range(55):                             # fk == k: atan2(-fy, -fx) = pi (2k / 54 - 1)
        th = np.pi * (2 * k / 54.0 - 1)
        for rad in (0.5, 1.0, 1.5):
            x, y = f32(-rad * np.cos(th)), f32(-rad * np.sin(th))
            bound.append((x, y))
            bound.append((np.nextafter(x, f32(np.inf)), y))
            bound.append((x, np.nextafter(y, f32(-np.inf))))
    return np.array(edge, dtype=f32), np.array(bound, dtype=f32)


def fields():
    """the stored fields (the alley field is the existing fixture) and the MotionToColor runs over them:
    (run name, field name, maxmotion, row step of the stored RGB)"""
    rng = np.random.default_rng(7)
    f32 = np.float32
    noisy = (rng.standard_normal((48, 64, 2)) * 6).astype(f32)
    flat = noisy.reshape(-1)
    idx = rng.choice(flat.size, 200, replace=False)
    flat[idx[:50]] = np.nan
    flat[idx[50:90]] = np.inf
    flat[idx[90:130]] = -np.inf
    flat[idx[130:170]] = 2e9
    flat[idx[170:]] = -1.5e9
    thresh = (rng.standard_normal((5, 9, 2)) * 3).astype(f32)
    thresh[2, 4] = (1e9, -1e9)                      # exactly at the threshold: known
    thresh[3, 1] = (np.nextafter(f32(1e9), f32(np.inf)), 0)     # just beyond it: unknown
    neg = np.full((9, 11, 2), -1500, f32)           # every flow below -999: the printed maxima stay at -999
    neg[..., 1] = -2000
    unknown = np.full((6, 5, 2), np.nan, f32)
    unknown[0, :, 0] = 3e9
    stored = {"noisy": noisy, "threshold": thresh, "zero": np.zeros((7, 13, 2), f32), "unknown": unknown, "below": neg}
    runs = [("alley", "alley", -1.0, 8), ("alley_max5", "alley", 5.0, 16), ("noisy", "noisy", -1.0, 1), ("noisy_max0", "noisy", 0.0, 1),
            ("threshold", "threshold", -1.0, 1), ("zero", "zero", -1.0, 1), ("unknown", "unknown", -1.0, 1), ("below", "below", -1.0, 1)]
    return stored, runs


def main():
    if not os.path.isdir(os.path.join(REF, "flow_code", "C")):
        sys.exit("make_colorcode_golden.py: the reference tree is not at %s" % REF)
    sys.path.insert(0, os.path.dirname(OUT))
    from colorcode_ref import grid_vectors
    with tempfile.TemporaryDirectory() as tmp:
        L = build(tmp)

        def cc(v):
            v = np.ascontiguousarray(v, np.float32)
            out = np.zeros((len(v), 3), np.uint8)
            L.cc_batch(len(v), v.ctypes.data, out.ctypes.data)
            return out

        edge, bound = named_vectors()
        named = np.concatenate([edge, bound])
        rec = {"cc_named_in": named, "cc_named_out": cc(named),
               "cc_named_kind": np.repeat(np.array([1, 2], np.uint8), [len(edge), len(bound)]), "cc_grid_out": cc(grid_vectors())}
        stored, runs = fields()
        alley = np.load(os.path.join(OUT, "alley_0001_flo.npz"))["flow"]
        for name, flow in stored.items():
            rec["field/%s" % name] = flow
        for name, field, mm, step in runs:
            flow = np.ascontiguousarray(alley if field == "alley" else stored[field], np.float32)
            h, w = flow.shape[:2]
            rgb = np.zeros((h, w, 3), np.uint8)
            pr = np.zeros(5, np.float64)
            L.mtc(w, h, flow.ctypes.data, mm, rgb.ctypes.data, pr.ctypes.data)
            rec["mtc/%s/field" % name] = np.array(field)
            rec["mtc/%s/maxmotion" % name] = np.float32(mm)
            rec["mtc/%s/rows" % name] = np.int32(step)
            rec["mtc/%s/rgb" % name] = rgb[::step]
            rec["mtc/%s/stats" % name] = pr.astype(np.float32)     # printed floats, promoted to double by printf: exact
            print(name, flow.shape, "stats", pr)
        rec["mtc_runs"] = np.array([r[0] for r in runs])
    path = os.path.join(OUT, "colorcode_ref.npz")
    np.savez_compressed(path, **rec)
    print("wrote %s (%d bytes, %d named vectors, %d grid vectors)" % (path, os.path.getsize(path), len(named), len(grid_vectors())))


if __name__ == "__main__":
    main()
